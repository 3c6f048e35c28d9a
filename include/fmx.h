/*
 * fmx.h — C ABI of the MI355X-native batched FM-index count/locate engine.
 *
 * This is the drop-in boundary for baku4/sview-fmindex's query hot path.  The
 * reference has no FFI of its own: its surface is the Rust generic API
 * `FmIndex<'a, P: Position, B: Block, E: TextEncoder>` (sview-fmindex/src/lib.rs:14-28)
 * over the blob byte layout written by `FmIndexBuilder::build`
 * (src/builder/mod.rs:187-264).  Each entry point below names the reference
 * item it replaces; INTEGRATION.md shows the Rust `extern "C"` binding a
 * maintainer would add to restore `FmIndex::count/locate` on top of it.
 *
 * Conventions
 *  - Plain pointers and sizes only.  "Host" buffers are ordinary CPU memory;
 *    "device" buffers are HIP device pointers on the index's device.
 *  - P-wide outputs (counts, locations) are uint32_t when layout.pos_bytes == 4
 *    and uint64_t when 8, exactly the reference's `P` (src/text_length.rs:10-129).
 *  - Locations of one pattern are emitted in suffix-array-row order, the order
 *    `FmIndex::locate` returns them in (src/locate/mod.rs:14-37).
 *  - No entry point aborts: every failure the reference reports as an error or
 *    a panic is returned as an fmx_status.
 */
#ifndef FMX_H
#define FMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMX_ABI_VERSION 8u

typedef enum fmx_status {
    FMX_OK = 0,
    FMX_E_FORMAT = 1,        /* LoadError::InvalidFormat (src/load_from_blob.rs:16-19, 31-33)          */
    FMX_E_SIZE = 2,          /* LoadError::MismatchedBlobSize(expected, actual) (load_from_blob.rs:20-23, 46-58) */
    FMX_E_ALIGN = 3,         /* misaligned blob: reference panics (bwm/mod.rs:172-181); BuildError::NotAlignedBlob */
    FMX_E_LAYOUT = 4,        /* layout tag inconsistent with the blob's headers (P/B/E are not stored in the blob) */
    FMX_E_EMPTY_PATTERN = 5, /* empty pattern: reference panics (components/count_array.rs:211)            */
    FMX_E_SYMBOL = 6,        /* PassThrough byte >= symbol_count; BuildError::SymbolCountOver (builder/mod.rs:71-73) */
    FMX_E_CAPACITY = 7,      /* locate output buffer smaller than the number of occurrences ("needed")   */
    FMX_E_DEVICE = 8,        /* HIP runtime error, or no GPU                                               */
    FMX_E_ARG = 9,           /* null pointer or invalid argument                                           */
    FMX_E_CONFIG = 10        /* BuildError::{InvalidConfig, UnmatchedTextLength, InvalidBlobSize}          */
} fmx_status;

/* The reference's type parameters, which the blob does not record
 * (only sizes are checked, src/load_from_blob.rs:40-58). */
typedef struct fmx_layout {
    uint32_t pos_bytes; /* P: 4 = u32, 8 = u64                      (src/text_length.rs:10-129)   */
    uint32_t planes;    /* B = BlockN<V>: N in 2..6                  (components/bwm/blocks/mod.rs)  */
    uint32_t vec_bits;  /* V: 32, 64 or 128 = BLOCK_LEN              (components/bwm/blocks/vector.rs:11-79) */
    uint32_t encoder;   /* E: FMX_ENC_TABLE or FMX_ENC_PASS          (components/text_encoder/)      */
} fmx_layout;

#define FMX_ENC_TABLE 0u /* EncodingTable([u8; 256])  text_encoders/encoding_table.rs:7-11 */
#define FMX_ENC_PASS 1u  /* PassThrough               text_encoders/pass_through.rs:6-12   */

/* Query flags */
#define FMX_PATTERN_REVERSED 1u /* patterns are given last byte first: the *_rev_iter forms
                                   (src/locate/with_rev_iter.rs:5-38)                          */
#define FMX_HINT_LONG_PATTERNS 2u /* performance hint: patterns average more than 64 bytes; the
                                   kernels stage each workgroup's patterns in 56 KB of LDS
                                   instead of 16 KB                                            */
/* Performance hint: stage each 256-pattern tile in kb KB of LDS (1..56): the
 * most bytes any tile's patterns span.  A tile that does not fit is read from
 * HBM instead (same results).  Less LDS per workgroup = more workgroups per
 * CU.  Overrides FMX_HINT_LONG_PATTERNS; the host-buffer calls set it exactly. */
#define FMX_HINT_STAGE_KB(kb) ((((uint32_t)(kb)) & 0xffu) << 8)
/* Performance hint: every pattern is m bytes (1..65535) and d_offsets[i] ==
 * i * m, so the kernels address each pattern's bytes without first reading
 * the offsets (one dependent HBM round trip fewer per workgroup).  The
 * offsets are still read alongside and checked: a batch that disagrees is
 * reported as FMX_E_ARG (its outputs are then undefined).  Because the bytes
 * are read before that check, a hint larger than the true length is
 * undefined behaviour for the reads: the kernels read up to n_patterns * m
 * bytes from d_bytes, which must be that large.  The host-buffer calls set
 * the hint themselves when every pattern has the same length. */
#define FMX_HINT_FIXED_LEN(m) ((((uint32_t)(m)) & 0xffffu) << 16)
/* Strand flags of the slot queries (fmx_match_batch, fmx_seeds_batch,
 * fmx_approx_batch and their _async forms; "Both strands" below).  They need a
 * complement map (fmx_set_complement), exclude each other, and are FMX_E_ARG
 * in every count and locate call. */
#define FMX_PATTERN_REVCOMP 4u /* each pattern is searched as its reverse complement only       */
#define FMX_BOTH_STRANDS 8u    /* each pattern is searched as given and as its reverse complement */

/* Load options: device-side structures derived from the blob at load time.
 * Results are identical with any combination; they trade HBM for fewer
 * dependent random reads per pattern. */
#define FMX_OCC_BLOB 0u        /* kernels read the blob's rank_checkpoints / blocks as laid out   */
#define FMX_OCC_INTERLEAVED 1u /* checkpoints + bit planes re-laid out into one HBM line per block */
#define FMX_OPT_DEEP_LUT 2u    /* a K-mer interval table (K > the blob's k), built on the GPU by
                                  breadth-first backward search; replaces the first LF steps.
                                  Indexed by the S symbols that occur in the text: K = the
                                  largest with S^K * 2P bytes <= FMX_DEEP_LUT_MB (environment;
                                  default 163840, capped at half the free HBM) */
#define FMX_OPT_FULL_SA 4u     /* the full suffix array (n x P), recovered on the GPU by walking every
                                  row to its sample: a location is one read, no walk            */
#define FMX_OPT_TEXT 8u        /* the text (n symbol indices), recovered from the full SA; once an
                                  interval is a single row, the rest of the pattern is compared
                                  against the text instead of LF-stepped (needs FMX_OPT_FULL_SA) */
#define FMX_OPT_ROW_CONTEXT 16u /* full SA stored as row records {SA[r], ctx[r]} (2P per row), ctx =
                                  the up to context_len symbols preceding the suffix, packed base
                                  sigma+1; an interval of at most FMX_SCAN_ROWS rows (environment,
                                  default 32) is finished by one contiguous scan of its records
                                  instead of LF steps (implies FMX_OPT_FULL_SA | FMX_OPT_TEXT)    */
#define FMX_OPT_LUT_ROWS 32u   /* deep-table entries whose interval is a single row hold that row's
                                  SA value and the symbols preceding its suffix instead of the
                                  interval: such a pattern is settled by that one read (plus a
                                  text compare beyond the packed symbols).  Needs FMX_OPT_DEEP_LUT
                                  and FMX_OPT_TEXT, and n < 2^31 for u32 positions            */
/* The default: the blob's own structures, its occ planes and checkpoints
 * re-laid out as one record per block — the reference's index and algorithm
 * (FmIndex::load is a zero-copy view, load_from_blob.rs:28-85; this is one
 * device copy plus a 1/2.7 size re-layout, milliseconds at 1 Gbp). */
#define FMX_OPT_DEFAULT FMX_OCC_INTERLEAVED
/* Every derived structure: ~55x the blob's HBM at C2 (147 GB) and seconds of
 * load time, paid back only after ~10^10 patterns (bench.py "derived"). */
#define FMX_OPT_DERIVED (FMX_OCC_INTERLEAVED | FMX_OPT_DEEP_LUT | FMX_OPT_FULL_SA | FMX_OPT_TEXT | \
                         FMX_OPT_ROW_CONTEXT | FMX_OPT_LUT_ROWS)
/* The text (n + 16 bytes of symbol indices, the buffer of FMX_OPT_TEXT) kept in
 * HBM for fmx_verify_async / fmx_map_batch ONLY: no search reads it, and the
 * index stays the one the other options make — with FMX_OPT_DEFAULT still the
 * faithful one: grouped and fused launches, every query's path and bytes, and
 * everything fmx_info reports but `options` (this bit, when the text is held)
 * and `device_bytes` (+ n + 16) are unchanged.  Not part of FMX_OPT_DERIVED.
 * The text is recovered through the full suffix array: without FMX_OPT_FULL_SA
 * / FMX_OPT_TEXT that array is a temporary of the load, freed before it
 * returns — the load's PEAK HBM is n * P + 64 bytes (4 GB at 1 Gbp and u32
 * positions) above what the loaded index keeps.  With them the array stays and
 * the one text buffer is shared.  (An index loaded with FMX_OPT_TEXT serves
 * the verify calls without this bit.) */
#define FMX_OPT_VERIFY_TEXT 64u
/* fmx_load_file only: read the blob's body with O_DIRECT, bypassing the page
 * cache — a cold load from storage, what the reference bench measures after
 * dropping the caches (bench/run_benchmark.sh:53-56).  FMX_E_ARG if the
 * file system refuses O_DIRECT (tmpfs does). */
#define FMX_LOAD_DIRECT (1u << 16)

typedef struct fmx_index fmx_index; /* opaque; one per (blob, device) */

typedef struct fmx_index_info {
    uint64_t text_len;       /* C[symbol_count]                                   */
    uint64_t sentinel_index; /* BwmView.sentinel_index                            */
    uint64_t blob_len;
    uint64_t device_bytes;   /* HBM held by the index (blob + derived structures) */
    uint32_t symbol_count;
    uint32_t kmer_size;      /* lookup_table_kmer_size                            */
    uint32_t sampling_ratio;
    uint32_t block_len;      /* BLOCK_LEN = vec_bits                              */
    uint32_t options;        /* FMX_OCC_* | FMX_OPT_* in effect                   */
    uint32_t deep_lut_k;     /* K of the deep k-mer table (0 = none)              */
    int32_t device;
    uint32_t context_len;    /* symbols per row context (0 = no row records)      */
    uint32_t scan_rows;      /* largest interval finished by a record scan        */
    uint32_t occ_record;     /* occ record encoding: 0 blob layout, 64/128 interleaved
                                records, | 1 paired-chunk, | 2 symbol-mask records
                                                                     */
    uint32_t group_key_len;  /* grouped launches: the key's last symbols (0: none) */
    uint32_t group_key_base; /* ... as digits over this many symbols               */
    uint64_t grouped_min;    /* fixed-length launches of at least this many
                                patterns are grouped (UINT64_MAX: never)            */
    uint64_t launches_grouped;      /* locate launches of this index so far, by the
                                       path they took: grouped with packed records, */
    uint64_t launches_grouped_raw;  /* grouped with id-only records,                  */
    uint64_t launches_ordered;      /* in launch order,                               */
    uint64_t launches_fused;        /* of those, as one kernel (k_locate: search,
                                       offsets and locations; FMX_FUSED=0: never)   */
    uint64_t launches_chained;      /* grouped launches ended by k_emit_chain (tile
                                       counts handed from tile to tile in-kernel)    */
} fmx_index_info;

typedef struct fmx_kernel_timing {
    char name[32];
    uint64_t launches;
    double total_ms;         /* summed hipEvent durations on the launch stream    */
    uint64_t units;          /* patterns (count) or occurrences (locate) processed */
} fmx_kernel_timing;

/* ---------------------------------------------------------------- version */
uint32_t fmx_abi_version(void);
const char *fmx_status_str(fmx_status s);
int fmx_device_count(void);

/* ------------------------------------------------------------------- load */

/* FmIndex::load (src/load_from_blob.rs:28-85).  Validates the blob exactly as
 * the reference does (magic + version, header sizes, exact body size) plus the
 * consistency checks the reference leaves to the type system, then copies the
 * blob to HBM of `device` once.  The host blob is borrowed for fmx_blob() only.
 * On FMX_E_SIZE, *expected_total / *actual_total receive the two sizes.
 * options: FMX_OCC_* | FMX_OPT_* (FMX_OPT_DEFAULT: the blob's own structures). */
fmx_status fmx_load(const uint8_t *blob, uint64_t blob_len, fmx_layout layout, int device,
                    uint32_t options, fmx_index **out, uint64_t *expected_total,
                    uint64_t *actual_total);

/* Same, for a blob already resident in HBM of `device` (e.g. written by
 * fmx_build_device).  The device blob is borrowed and must outlive the index.
 * Starts after all work already queued on the device: it calls
 * hipDeviceSynchronize, which also waits for unrelated work on other streams
 * (other threads' queries, pending collectives) — load before serving starts,
 * or order the blob's writer yourself and accept that wait once. */
fmx_status fmx_load_device(const uint8_t *d_blob, uint64_t blob_len, fmx_layout layout, int device,
                           uint32_t options, fmx_index **out, uint64_t *expected_total,
                           uint64_t *actual_total);

/* Blob ingest from a file (the bench's mmap / read-whole-file loaders,
 * bench/src/locate/sview_mmap.rs:17-45 and sview_memory.rs:17-20, then
 * FmIndex::load).  The header is read and validated first (same checks and
 * codes as fmx_load; the file size is the blob length); the body is then
 * streamed file -> a ring of four pinned host chunks -> HBM, each chunk read
 * by several threads while earlier chunks are in flight, so no host copy of
 * the whole blob is ever held.  chunk_bytes = 0 picks the default (16 MiB:
 * pinning larger buffers costs more than it saves).  FMX_E_ARG if the file cannot
 * be opened or read.  fmx_blob() returns NULL for such an index. */
fmx_status fmx_load_file(const char *path, fmx_layout layout, int device, uint32_t options,
                         uint64_t chunk_bytes, fmx_index **out, uint64_t *expected_total,
                         uint64_t *actual_total);

void fmx_free(fmx_index *ix);

/* FmIndex::blob (src/reference_to_source_blob.rs:9-11).  NULL for device loads. */
const uint8_t *fmx_blob(const fmx_index *ix, uint64_t *len);

fmx_status fmx_info(const fmx_index *ix, fmx_index_info *out);

/* Both strands.  The complement map of the strand flags: map[b] is the
 * complement of input byte b (256 bytes, byte to byte; NULL removes the map).
 * Any map is legal: it need not be an involution, and bytes outside the
 * alphabet map wherever the caller says.  The index keeps the 256-byte device
 * table enc_rc[b] = enc[map[b]] (enc: the index's encoding table; PassThrough:
 * the identity, so enc_rc = map and a map[b] >= symbol_count ends a match as
 * such a byte of a pattern does).  Synchronous; applies to launches queued
 * after it returns.  Calling it while strand launches of this index are in
 * flight leaves it undefined which of the two tables each of them uses — never
 * a fault: the table is always 256 entries indexed by a byte.
 * fmx_get_complement copies the map that was set to map_out (256 bytes);
 * FMX_E_ARG when none is set.
 *
 * The contract, with pattern i in logical order p[0..m) (FMX_PATTERN_REVERSED
 * still only says how its bytes arrive) and rc(p)[j] = map[p[m-1-j]], j in
 * 0..m: a call with FMX_PATTERN_REVCOMP returns exactly what the same call
 * without the flag returns for the batch rc(p_0), ..., rc(p_{n-1}); a call
 * with FMX_BOTH_STRANDS returns exactly what it returns for the 2n-pattern
 * batch p_0, rc(p_0), p_1, rc(p_1), ...: virtual pattern v = 2 i + s is strand
 * s of read i.  Under FMX_BOTH_STRANDS every per-pattern output array has 2n
 * entries, every per-slot array 2n * per (per = 1, max_seeds or max_hits),
 * loc_offsets 2n * per + 1, the workspace is fmx_locate_workspace_size(2n *
 * per) bytes, and the slot limit and the timer units count 2n patterns.
 * Positions reported for strand 1 (seed spans, approx substitutions) are in
 * rc(p)'s own coordinates: a seed covering rc(p)[e-L..e) is p[m-e..m-e+L) of
 * the read.  Ranges-only mode, the capacity contract, min_len / max_occ /
 * FMX_APPROX_BEST hold unchanged on the virtual batch; FMX_HINT_FIXED_LEN and
 * the offsets are the n reads' (a disagreement is still FMX_E_ARG), and the
 * reads' bytes are uploaded and read once.  FMX_E_ARG: both flags together,
 * either flag on an index without a map, either flag in fmx_count_batch,
 * fmx_locate_batch, their _async forms, fmx_locate_jobs_async or
 * fmx_locate_group_async. */
fmx_status fmx_set_complement(fmx_index *ix, const uint8_t *map);
fmx_status fmx_get_complement(const fmx_index *ix, uint8_t *map_out);

/* ---------------------------------------------- queries on host buffers
 * Synchronous.  Patterns are ragged: pattern i is bytes[offsets[i] .. offsets[i+1]). */

/* FmIndex::count / count_rev_iter (locate/with_slice.rs:5-8, with_rev_iter.rs:5-9), batched. */
fmx_status fmx_count_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                           uint64_t n_patterns, uint32_t flags, void *out_counts);

/* FmIndex::locate / locate_rev_iter (with_slice.rs:10-13, with_rev_iter.rs:10-14),
 * batched: the locations of pattern i are out_locs[out_loc_offsets[i] ..
 * out_loc_offsets[i+1]) in suffix-array-row order.  *needed receives the total;
 * if it exceeds cap, nothing past cap is written and FMX_E_CAPACITY is returned. */
fmx_status fmx_locate_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                            uint64_t n_patterns, uint32_t flags, uint64_t *out_loc_offsets,
                            void *out_locs, uint64_t cap, uint64_t *needed);

/* ---------------------------------------------- queries on device buffers
 * Asynchronous on `stream` (a hipStream_t; NULL = the index's own stream).
 * Inputs and outputs live in HBM of the index's device.  Errors detected on
 * the device (empty pattern, PassThrough symbol) are latched in a status word
 * read by fmx_sync().  Only `stream` orders the launch: the index's own
 * stream is non-blocking (not ordered with the caller's streams, nor with the
 * legacy default stream), so buffers written on another stream must be
 * complete first — pass the writers' stream, or synchronise.
 *
 * Alignment, sizes and padding of the device pointers (every call below):
 *  - d_bytes needs no alignment and no padding past d_offsets[n_patterns].
 *    The kernels read it in whole vectors aligned by ADDRESS (16 B; a grouped
 *    launch's key pass 4 B), and only vectors that hold at least one byte of
 *    the batch: up to 15 bytes before d_bytes and after its last byte are
 *    read and ignored, never anything outside the aligned 16-B lines the
 *    batch itself touches, so never another page.  Nothing is written to it.
 *  - the uint64_t arrays (d_offsets, d_loc_offsets, d_needed): 8-B aligned;
 *    d_lens: 4; the P-wide arrays (d_counts, d_locs, d_ranges): P.  Each is
 *    accessed as elements of its own type only: exactly n_patterns + 1
 *    offsets, n_patterns counts and lens, 2 n_patterns range words, one
 *    needed word and at most cap locations — an array of exactly that size
 *    is enough, and no byte outside it is read or written.
 *    fmx_seeds_batch_async, with S = n_patterns * max_seeds slots: d_nseeds,
 *    d_rest and d_spans 4-B aligned (n_patterns, n_patterns and 2 S words),
 *    d_ranges P-aligned (2 S words), d_loc_offsets S + 1 offsets; the same
 *    rule: exactly that size, no byte outside it touched.
 *    fmx_approx_batch_async, with S = n_patterns * max_hits slots: d_nhits,
 *    d_more, d_mm and d_subs 4-B aligned (n_patterns, n_patterns, S and 6 S
 *    words), d_ranges P-aligned (2 S words), d_loc_offsets S + 1 offsets;
 *    the same rule again.
 *  - the workspace: 16-B aligned, fmx_locate_workspace_size(n_patterns)
 *    bytes (fmx_seeds_batch_async: of n_patterns * max_seeds, and
 *    fmx_approx_batch_async: of n_patterns * max_hits, one "pattern" per
 *    slot); a launch may write any of it and nothing outside it.
 *  - FMX_BOTH_STRANDS: d_bytes and d_offsets are the n_patterns reads' (read
 *    by the rule above, once), and every size above that is counted in
 *    patterns or slots is taken with 2 n_patterns for n_patterns: 2 n lens
 *    and 4 n range words for a match, 2 n counts (d_nseeds, d_rest, d_nhits,
 *    d_more) and S = 2 n * per slots for seeds and approx, S + 1 location
 *    offsets, a workspace of fmx_locate_workspace_size(S) bytes.  Exactly
 *    that size, no byte outside it touched.  To stage both strands' copies
 *    of a tile (128 reads) FMX_HINT_STAGE_KB must cover twice the bytes the
 *    tile's reads span; a tile that does not fit is read from HBM.
 *    FMX_PATTERN_REVCOMP changes no size.
 *  - cap = 0 with d_locs = NULL sizes an output: the offsets, the counts and
 *    *d_needed are written, no location is. */

fmx_status fmx_count_batch_async(fmx_index *ix, const uint8_t *d_bytes, const uint64_t *d_offsets,
                                 uint64_t n_patterns, uint32_t flags, void *d_counts, void *stream);

/* Workspace for fmx_locate_batch_async, in bytes, for up to n_patterns patterns:
 * [256 B][32 KiB of key counters][58 KiB batch table of a grouped launch]
 * [tile counts][tile offsets][one search record per pattern][to 16 B][one
 * 16-B sorted-order record per pattern].
 * The workspace must be 16-byte aligned (FMX_E_ARG otherwise: the grouped
 * passes read and write it as 16-B vectors; hipMalloc gives 256-B alignment).
 * A workspace needs no initialisation (a grouped launch zeroes its key
 * counters on its stream first) and belongs to this index: its launches are
 * ordered on one stream at a time.  A locate is k_search + k_emit.  A
 * grouped locate first deals the launch's patterns out in the order of their
 * last symbols, so that patterns whose backward searches share their first
 * LF steps run side by side, and searches them in that order — same
 * results.  Grouped by default: launches (a group call's batches together) of
 * at least 3 x 2^20 fixed-length patterns that pack into 96 bits, on the
 * faithful index, when the key spans at least 5 symbols (DNA: 6), of at
 * least 2^26 when it spans fewer (20 residues: 3; environment
 * at load: FMX_GROUPED=0 never, =1 always — longer patterns too, with
 * id-only records —, FMX_GROUPED_MIN=<patterns>, FMX_GROUPED_RAW=1 id-only
 * records, FMX_GROUP_REFINE_MIN=<patterns> re-sorts each key's run by the
 * next symbols, FMX_GROUPED_WSORT=0 turns off the search's in-workgroup sort
 * by the next symbols, FMX_GROUP_CHECK=1 checks each launch's sorted order on
 * the device before its search — a violation is FMX_E_DEVICE; debug).  One
 * kernel makes workgroups wait on others: the fused launch in launch order
 * (k_locate, fmx_index_info.launches_fused; FMX_FUSED=0 never) — a workgroup
 * answers the tile of its ticket (the number of its batch's workgroups that
 * started before it) and waits only for the earlier tiles of its batch, whose
 * workgroups are therefore already running; bounded (FMX_FUSED_TIMEOUT_MS,
 * default 4 s, then FMX_E_DEVICE).  The key counters and the batch table of a
 * grouped launch are in its first batch's workspace. */
fmx_status fmx_locate_workspace_size(fmx_index *ix, uint64_t n_patterns, uint64_t *bytes);

/* The same size without an index (ABI 8): for n_patterns patterns of an
 * index with pos_bytes-wide positions (4 or 8; FMX_E_ARG otherwise) — what a
 * caller sizing HBM before it loads an index (e.g. the per-rank accounting of
 * a sharded job) needs.  Equal to fmx_locate_workspace_size on such an index. */
fmx_status fmx_workspace_bytes(uint64_t n_patterns, uint32_t pos_bytes, uint64_t *bytes);

/* d_loc_offsets has n_patterns+1 entries; d_counts (optional, may be NULL)
 * receives P-wide counts; d_needed (device uint64) receives the total. */
fmx_status fmx_locate_batch_async(fmx_index *ix, const uint8_t *d_bytes, const uint64_t *d_offsets,
                                  uint64_t n_patterns, uint32_t flags, void *d_counts,
                                  uint64_t *d_loc_offsets, void *d_locs, uint64_t cap,
                                  uint64_t *d_needed, void *d_workspace, uint64_t workspace_bytes,
                                  void *stream);

/* A queue of locate batches submitted in one call (a serving loop's batches
 * in flight): job i is exactly fmx_locate_batch_async(ix, jobs[i].d_bytes,
 * ...), issued in order, each on its own stream; the call returns after the
 * last launch is queued (or at the first error, which it returns). */
typedef struct fmx_locate_job {
    const uint8_t *d_bytes;
    const uint64_t *d_offsets;
    uint64_t n_patterns;
    uint32_t flags;
    uint32_t reserved;         /* 0 */
    void *d_counts;            /* optional */
    uint64_t *d_loc_offsets;
    void *d_locs;
    uint64_t cap;
    uint64_t *d_needed;
    void *d_workspace;
    uint64_t workspace_bytes;
    void *stream;              /* hipStream_t; NULL = the index's own stream */
} fmx_locate_job;

fmx_status fmx_locate_jobs_async(fmx_index *ix, const fmx_locate_job *jobs, uint64_t n_jobs);

/* The same batches run together: up to 1,024 per launch on `stream` (each
 * batch keeps its own patterns, outputs and workspace; the jobs' own stream
 * fields are ignored), so that small batches fill the GPU the way one large
 * batch does — a grouped launch searches all of them in one order (kernels
 * take at most 256 batches as arguments: the launch-order path runs one
 * launch per 256).  The jobs' workspaces must be distinct and no two jobs may share
 * an output buffer (they run concurrently).  The results are those of
 * fmx_locate_batch_async on each job. */
fmx_status fmx_locate_group_async(fmx_index *ix, const fmx_locate_job *jobs, uint64_t n_jobs, void *stream);

/* ------------------------------------------------- longest-suffix match
 * Greedy backward seeding, what a read mapper asks of a batched FM-index (no
 * reference counterpart: FmIndex::count / locate answer only whether a whole
 * pattern occurs).  Added within ABI 8: the additions are backward
 * compatible, FMX_ABI_VERSION is unchanged.
 * With pattern i in logical order p[0..m) (FMX_PATTERN_REVERSED as for locate:
 * the bytes arrive last symbol first) and c = idx_of(byte):
 *  - lens[i] = the largest L <= m for which the last L symbols S = p[m-L..m)
 *    occur in the encoded text; 0 if the last symbol does not (or m = 0);
 *  - ranges[2i], ranges[2i+1] = (lo, hi), P-wide: the interval of S in the
 *    reduced row coordinates of get_pos_range (locate/with_slice.rs:21-33), so
 *    hi - lo is the count of S; (0, 0) when L = 0;
 *  - pattern i REPORTS when L >= max(min_len, 1) and hi - lo <= max_occ.  lens
 *    and ranges are the true values either way; locations are emitted for
 *    reporting patterns only: loc_offsets[i+1] - loc_offsets[i] is hi - lo for
 *    them and 0 for the rest, in suffix-array-row order — what
 *    fmx_locate_batch returns for S.
 * Nothing here is an error of its own: an empty pattern gives L = 0, and a
 * PassThrough byte >= symbol_count ends the match before it, like any symbol
 * that does not extend the interval (a disagreeing FMX_HINT_FIXED_LEN is still
 * FMX_E_ARG).  The search reads the blob's own k-mer table (the seed; suffixes
 * shorter than k through its m < k form, count_array.rs:203-223) and the
 * index's occ records in whichever encoding it was loaded with; derived
 * structures do not shorten it (a loaded full SA serves the locations).
 * out_loc_offsets == NULL (d_loc_offsets == NULL) selects lengths and
 * intervals only: the location arguments and the workspace are ignored.
 * Otherwise the capacity contract is fmx_locate_batch's (*needed written,
 * FMX_E_CAPACITY if it exceeds cap; lens, ranges and offsets are written
 * either way), and the device call's workspace has the size of
 * fmx_locate_workspace_size and the same 16-B alignment rule.  The host call
 * sets the staging and fixed-length hints itself.  A match runs in launch
 * order: k_match, then the locate's k_emit.  Timer: "match".
 * FMX_PATTERN_REVCOMP / FMX_BOTH_STRANDS (here, in fmx_seeds_batch and in
 * fmx_approx_batch): "Both strands" above — the same call on rc(p_i), or on
 * the 2n patterns p_0, rc(p_0), p_1, ..., with every output shaped for them. */
fmx_status fmx_match_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                           uint64_t n_patterns, uint32_t flags, uint32_t min_len, uint64_t max_occ,
                           uint32_t *out_lens, void *out_ranges, uint64_t *out_loc_offsets,
                           void *out_locs, uint64_t cap, uint64_t *needed);
fmx_status fmx_match_batch_async(fmx_index *ix, const uint8_t *d_bytes, const uint64_t *d_offsets,
                                 uint64_t n_patterns, uint32_t flags, uint32_t min_len, uint64_t max_occ,
                                 uint32_t *d_lens, void *d_ranges, uint64_t *d_loc_offsets, void *d_locs,
                                 uint64_t cap, uint64_t *d_needed, void *d_workspace,
                                 uint64_t workspace_bytes, void *stream);

/* ------------------------------------------------------ greedy seed chains
 * The match above, repeated on the device until the pattern is used up: what
 * a read mapper does with a read after its first seed (no reference
 * counterpart).  Added within ABI 8: FMX_ABI_VERSION is unchanged.
 * Pattern i is p[0..m) in logical order (FMX_PATTERN_REVERSED as for locate).
 * Parameters: max_seeds (1..32), min_len, skip, max_occ.  With e = m, j = 0,
 * while e > 0 and j < max_seeds:
 *  1. (L, lo, hi) = the longest-suffix match of the prefix p[0..e): exactly
 *     what fmx_match_batch returns for that prefix, same row coordinates.  A
 *     PassThrough byte >= symbol_count ends a match like any symbol that does
 *     not occur; nothing is an error of its own (a disagreeing
 *     FMX_HINT_FIXED_LEN is still FMX_E_ARG).
 *  2. if L >= max(min_len, 1) this is seed j, covering p[e-L..e): with slot
 *     s = i * max_seeds + j, spans[2s] = e (its end, exclusive), spans[2s+1] =
 *     L, ranges[2s], ranges[2s+1] = lo, hi (P-wide); j += 1.
 *  3. e -= min(e, max(L + skip, 1)).  skip = 0: the non-overlapping cover of
 *     the pattern; skip = 1 steps over the symbol that failed to extend (a
 *     substitution); any skip is legal.
 * Then nseeds[i] = j and rest[i] = e: 0 when the whole pattern was parsed,
 * else the slots ran out and the caller may resubmit the first rest[i]
 * symbols.  Every slot j >= nseeds[i] is written as zeros in spans and ranges:
 * the outputs are fully defined.  An empty pattern: 0 seeds, rest = 0.
 * out_loc_offsets == NULL (d_loc_offsets == NULL) selects spans and ranges
 * only: the location arguments and the workspace are ignored.  Otherwise
 * loc_offsets has n_patterns * max_seeds + 1 entries, one per slot: a stored
 * seed REPORTS when hi - lo <= max_occ (min_len was applied when it was
 * stored) and its slot then holds its hi - lo locations in suffix-array-row
 * order — what fmx_locate_batch returns for that substring; every other slot
 * holds none.  The capacity contract is fmx_locate_batch's: *needed is always
 * exact, FMX_E_CAPACITY when it exceeds cap, nothing written past cap; nseeds,
 * rest, spans, ranges and the offsets are written either way.  The host call
 * makes one launch with the caller's cap (no retry) and sets the staging and
 * fixed-length hints itself.  The device call's workspace is
 * fmx_locate_workspace_size(ix, n_patterns * max_seeds) bytes, 16-B aligned.
 * FMX_E_ARG: max_seeds outside 1..32, a required pointer that is null, more
 * slots than a launch's 2^31 - 1 tiles of 256 hold.
 * One kernel, k_seeds (a lane per pattern, the pattern staged once, the match
 * restarted on ever shorter prefixes), then the locate's k_emit over the
 * slots; launch order only; derived structures do not shorten the search (a
 * loaded full SA serves the locations).  Timer: "seeds", one unit per slot
 * (n_patterns * max_seeds: how many seeds were stored is not known to the
 * host when the launch is queued). */
fmx_status fmx_seeds_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                           uint64_t n_patterns, uint32_t flags,
                           uint32_t max_seeds, uint32_t min_len, uint32_t skip, uint64_t max_occ,
                           uint32_t *out_nseeds, uint32_t *out_rest,
                           uint32_t *out_spans, void *out_ranges,
                           uint64_t *out_loc_offsets, void *out_locs, uint64_t cap,
                           uint64_t *needed);
fmx_status fmx_seeds_batch_async(fmx_index *ix, const uint8_t *d_bytes, const uint64_t *d_offsets,
                                 uint64_t n_patterns, uint32_t flags,
                                 uint32_t max_seeds, uint32_t min_len, uint32_t skip, uint64_t max_occ,
                                 uint32_t *d_nseeds, uint32_t *d_rest,
                                 uint32_t *d_spans, void *d_ranges,
                                 uint64_t *d_loc_offsets, void *d_locs, uint64_t cap,
                                 uint64_t *d_needed, void *d_workspace, uint64_t workspace_bytes,
                                 void *stream);

/* ------------------------------------------------------- k-mismatch search
 * Search within a Hamming radius: what a read mapper's -v mode asks of an
 * FM-index (no reference counterpart).  Added within ABI 8: FMX_ABI_VERSION
 * is unchanged.
 * Pattern i is p[0..m) in logical order (FMX_PATTERN_REVERSED as for locate),
 * c_q = idx_of(p[q]).  Parameters: max_mm (0..3), max_hits (1..32), max_occ,
 * mode (0 or FMX_APPROX_BEST).
 * A VARIANT is a string v of m symbol indices that differs from the pattern
 * in d <= max_mm positions and occurs in the encoded text.  Substitutions
 * only, no insertions or deletions.  A position with c_q >= symbol_count (a
 * PassThrough byte out of range) can only be matched by substituting it; like
 * every other case here it is no error of its own (a disagreeing
 * FMX_HINT_FIXED_LEN is still FMX_E_ARG).  A substituted symbol ranges over
 * all of 0..symbol_count-1 except c_q; symbols that do not occur in the text
 * simply give no variant.  m = 0 gives no variant, and neither does an m
 * longer than the text.
 * ORDER: by d ascending; within one d, scan the positions from m-1 down to 0:
 * at the first position where two variants differ, the one that holds a
 * substituted symbol comes before the one that holds the pattern's own, and
 * of two substituted symbols the smaller index comes first.  (The order in
 * which a right-to-left depth-first search meets them when it tries the
 * substitutions of a position in ascending symbol order before the pattern's
 * own symbol.)
 * FMX_APPROX_BEST keeps only the variants of the smallest d that has any (a
 * mapper's "best stratum").  With H variants after that filter, nhits[i] =
 * min(H, max_hits) and more[i] = (H > max_hits); the search stops at the
 * (max_hits+1)-th variant and never computes H.
 * Pattern i owns slots s = i * max_hits + j, j < nhits[i] in the order above:
 * ranges[2s], ranges[2s+1] = lo, hi (P-wide, the reduced row coordinates of
 * get_pos_range: what fmx_match_batch reports for a pattern equal to v);
 * mm[s] = d; substitution t < d, listed by decreasing position, is subs[2(3s +
 * t)] = its position (logical order) and subs[2(3s+t)+1] = the substituted
 * symbol index.  Everything else in a pattern's slots is written as zeros —
 * t >= d and j >= nhits[i], in mm, subs and ranges: the outputs are fully
 * defined.
 * Locations follow the rules of seeds.  out_loc_offsets == NULL
 * (d_loc_offsets == NULL) selects intervals only: the location arguments and
 * the workspace are ignored.  Otherwise loc_offsets has n_patterns * max_hits
 * + 1 entries: a stored hit REPORTS when hi - lo <= max_occ, and its slot then
 * holds its hi - lo locations in suffix-array-row order — what
 * fmx_locate_batch returns for v; every other slot holds none.  The capacity
 * contract is fmx_locate_batch's: *needed is always exact, FMX_E_CAPACITY when
 * it exceeds cap, nothing written past cap; all other outputs are written
 * either way.  The host call makes one launch with the caller's cap (no
 * retry) and sets the staging and fixed-length hints itself.  The device
 * call's workspace is fmx_locate_workspace_size(ix, n_patterns * max_hits)
 * bytes, 16-B aligned.
 * FMX_E_ARG: max_mm > 3, max_hits outside 1..32, unknown mode bits, a required
 * pointer that is null, more slots than a launch's 2^31 - 1 tiles of 256 hold.
 * COST: a bounded backtracking walk per pattern.  On repetitive text the work
 * grows like (m * symbol_count)^max_mm LF steps per pattern; the caller bounds
 * it with max_mm and max_hits (a search ends at its (max_hits+1)-th variant).
 * There is no step budget in this version.
 * One kernel, k_approx (a lane per pattern, the pattern staged once, stratum
 * by stratum), then the locate's k_emit over the slots; launch order only;
 * derived structures do not shorten the search (a loaded full SA serves the
 * locations).  Timer: "approx", one unit per slot. */
#define FMX_APPROX_BEST 1u /* mode: only the variants of the smallest d that has any */
fmx_status fmx_approx_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                            uint64_t n_patterns, uint32_t flags,
                            uint32_t max_mm, uint32_t max_hits, uint32_t mode, uint64_t max_occ,
                            uint32_t *out_nhits, uint32_t *out_more,
                            uint32_t *out_mm, uint32_t *out_subs, void *out_ranges,
                            uint64_t *out_loc_offsets, void *out_locs, uint64_t cap,
                            uint64_t *needed);
fmx_status fmx_approx_batch_async(fmx_index *ix, const uint8_t *d_bytes, const uint64_t *d_offsets,
                                  uint64_t n_patterns, uint32_t flags,
                                  uint32_t max_mm, uint32_t max_hits, uint32_t mode, uint64_t max_occ,
                                  uint32_t *d_nhits, uint32_t *d_more,
                                  uint32_t *d_mm, uint32_t *d_subs, void *d_ranges,
                                  uint64_t *d_loc_offsets, void *d_locs, uint64_t cap,
                                  uint64_t *d_needed, void *d_workspace, uint64_t workspace_bytes,
                                  void *stream);

/* ------------------------------------------------- placing reads: the vote
 * What a read mapper does with a seed chain: every seed occurrence says where
 * the READ would start in the text, occurrences that agree are grouped, and
 * the few starts most of the read's seeds vote for are kept (no reference
 * counterpart).  Added within ABI 8: FMX_ABI_VERSION is unchanged.
 * fmx_vote_async reads exactly what a seeds launch with locations wrote for
 * n_chains patterns at max_seeds slots each — d_nseeds, d_spans,
 * d_loc_offsets, d_locs and the cap that launch was given; under
 * FMX_BOTH_STRANDS the caller passes its 2n: a chain is a virtual pattern.
 * Chain i owns slots s = i * max_seeds + j, j < nseeds[i]; seed j covers
 * p[e-L..e) with e = spans[2s], L = spans[2s+1], and its locations are
 * locs[loc_offsets[s] .. loc_offsets[s+1]), P-wide (none for a seed that did
 * not report).
 * HITS: the pairs (j, x), x a location of seed j, each with the DIAGONAL
 * d = (int64)x - (int64)(e_j - L_j): where the read would start, negative when
 * it would overhang the text's start.  H_i = loc_offsets[(i+1) max_seeds] -
 * loc_offsets[i max_seeds].
 * CLUSTERS: with the chain's hits sorted by (d, j), a new cluster starts at the
 * first hit and wherever d[k] - d[k-1] > band (single linkage; band = 0: exact
 * diagonals).  A cluster has pos = its smallest d, mask = the OR of 1u << j
 * over its hits, and cover = the sum of L_j over the bits of mask: a seed with
 * two hits in a cluster counts once, and as the seeds of a chain never overlap
 * cover is the number of the read's symbols the cluster explains.  A cluster
 * QUALIFIES when cover >= min_cover.
 * OUTPUTS: the qualifying clusters by cover descending, then pos ascending
 * (pos is unique per cluster: the order is total).  With Q of them, ncands[i]
 * = min(Q, max_cands), flags[i] has FMX_VOTE_MORE iff Q > max_cands, and
 * candidate k sits at c = i * max_cands + k: pos[c], cover[c], mask[c].  Every
 * unused candidate slot is written as zeros: the outputs are fully defined.
 * A chain with H_i > FMX_VOTE_MAX_HITS, or with loc_offsets[(i+1) max_seeds] >
 * cap (its locations were not all written), gets ncands = 0, flags =
 * FMX_VOTE_OVERFLOW and zeros; d_locs is never read at or past cap.  A chain
 * with no hit: ncands = 0, flags = 0.
 * Sizes and alignment: the rule of the device calls above — n_chains words for
 * d_nseeds, d_ncands and d_flags, 2 n_chains max_seeds for d_spans, n_chains
 * max_seeds + 1 offsets (8-B aligned), n_chains max_cands each for d_pos (8-B
 * aligned), d_cover and d_mask (4), d_locs P-aligned; each accessed as
 * elements of its own type only, exactly that size is enough.  No workspace,
 * and nothing is latched in the status word.  n_chains = 0 is FMX_OK and
 * launches nothing.  FMX_E_ARG: max_seeds outside 1..32, max_cands outside
 * 1..16, a null pointer (d_locs may be null only when cap = 0), a misaligned
 * pointer, more chains than a launch's 2^31 - 1 workgroups of four hold, an
 * index whose text_len >= 2^58 (so that (d + 2^32) << 5 | j packs into one
 * 64-bit sort key).
 * One kernel, k_vote: a wavefront per chain, its up to 1,024 keys held 16 to a
 * lane and sorted by a bitonic network (lanes exchange by shuffles, a lane's
 * own keys in registers), clusters and their masks by segmented shuffle scans,
 * the best max_cands by rounds of a wave arg-max; no LDS, no barrier.  Timer:
 * "vote", one unit per chain. */
#define FMX_VOTE_MAX_HITS 1024u   /* most seed occurrences one chain may bring to a vote */
#define FMX_VOTE_OVERFLOW 1u      /* flags[i] bit: the chain had more (or reached past cap): no candidates */
#define FMX_VOTE_MORE     2u      /* flags[i] bit: more than max_cands clusters qualified */
fmx_status fmx_vote_async(fmx_index *ix, uint64_t n_chains, uint32_t max_seeds,
                          const uint32_t *d_nseeds, const uint32_t *d_spans,
                          const uint64_t *d_loc_offsets, const void *d_locs, uint64_t cap,
                          uint32_t band, uint32_t min_cover, uint32_t max_cands,
                          uint32_t *d_ncands, uint32_t *d_flags,
                          int64_t *d_pos, uint32_t *d_cover, uint32_t *d_mask, void *stream);

/* Host buffers, synchronous: seeds -> locations -> vote on the device.  The
 * result is exactly fmx_vote_async applied to what fmx_seeds_batch returns
 * for the same arguments with a large enough cap.  Strand flags are those of
 * seeds: under FMX_BOTH_STRANDS every output is shaped for 2n chains, and a
 * strand-1 candidate's pos is where rc(p) starts in the text.  Nothing but the
 * reads goes up and nothing but the candidates comes down: seeds, locations
 * and the workspace live in temporary HBM, bounded by running the batch in
 * chunks of at most 65,536 reads (FMX_PLACE_CHUNK=<reads> in the environment
 * at load overrides; the results are identical whatever the chunk).
 * FMX_E_ARG when max_seeds * max_occ > FMX_VOTE_MAX_HITS (beside the argument
 * checks of seeds and of the vote): no chain can then overflow, and the
 * locations' capacity slots * max_occ is exact-or-over by construction, so
 * there is no FMX_E_CAPACITY and no retry.  The call sets the staging and
 * fixed-length hints itself, per chunk. */
fmx_status fmx_place_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                           uint64_t n_patterns, uint32_t flags,
                           uint32_t max_seeds, uint32_t min_len, uint32_t skip, uint64_t max_occ,
                           uint32_t band, uint32_t min_cover, uint32_t max_cands,
                           uint32_t *out_ncands, uint32_t *out_flags,
                           int64_t *out_pos, uint32_t *out_cover, uint32_t *out_mask);

/* ----------------------------------------------------- verifying placements
 * What a read mapper does with a candidate: align the read against the text
 * around it, to learn whether the candidate is real, how many edits it costs
 * and where the alignment starts and ends (no reference counterpart).  Added
 * within ABI 8: FMX_ABI_VERSION is unchanged.  The index must hold the text:
 * FMX_OPT_VERIFY_TEXT (or FMX_OPT_TEXT) at load.
 * fmx_verify_async takes the reads exactly as a seeds launch takes them —
 * FMX_PATTERN_REVERSED, FMX_PATTERN_REVCOMP and FMX_BOTH_STRANDS mean what
 * they mean there (nv = 2n virtual patterns v = 2i + s under the last); the
 * staging and fixed-length hints are accepted and ignored, the kernel always
 * reads the offsets — and the candidates fmx_vote_async wrote for those nv
 * chains at max_cands (1..16): d_ncands[nv], d_pos[nv * max_cands].  An
 * ncands[v] above max_cands counts as max_cands.
 * Per candidate slot c = v * max_cands + k: q[0..m) is virtual pattern v as
 * symbol indices in its logical order (strand 0: q[i] = enc[p[i]], strand 1:
 * q[i] = enc_rc[p[m-1-i]]), t[0..n) the text's symbol indices, P = pos[c]
 * (it may be negative).  Cells (i, j), 0 <= i <= m, are ALLOWED when j is in
 * A(i) = [max(0, i+P-band), min(n, i+P+band)]: the diagonals within `band` of
 * the candidate's, inside the text.  Unit costs: a substitution, an insertion
 * and a deletion cost 1 each; symbols compare by index, and a q[i] >=
 * symbol_count never matches.
 * FORWARD: F[0][j] = 0 on A(0); F[i][j] = min(F[i-1][j-1] + [q[i-1] != t[j-1]],
 * F[i-1][j] + 1, F[i][j-1] + 1) over allowed predecessors, infinite with none;
 * D = min over A(m) of F[m][j], tend = the smallest j attaining it.
 * BACKWARD (the same cells and costs, anchored): G[m][tend] = 0; G[i][j] =
 * min(G[i+1][j+1] + [q[i] != t[j]], G[i+1][j] + 1, G[i][j+1] + 1); tstart =
 * the largest j in A(0) with G[0][j] = D (one exists: both passes range over
 * the same paths).  So q aligns to t[tstart..tend) at cost D: the shortest of
 * the cheapest alignments that end at the earliest cheapest end.
 * OUTPUTS, fully defined: k < ncands[v], D finite and <= max_dist: dist[c] =
 * D, tstart[c], tend[c].  k < ncands[v] and D infinite, or D > max_dist, or
 * m > FMX_VERIFY_MAX_LEN: dist[c] = FMX_VERIFY_NONE, tstart = tend = 0.
 * k >= ncands[v]: three zeros.  (The row minimum of F never decreases with i:
 * a candidate is dropped at the first row whose minimum exceeds max_dist.)
 * m = 0 follows the rules as written: D = 0 when A(0) is not empty.
 * Sizes and alignment: the rule of the device calls above — nv words for
 * d_ncands, nv max_cands elements for d_pos, d_tstart, d_tend (8-B aligned)
 * and d_dist (4); d_bytes and d_offsets as for seeds.  No workspace, and
 * nothing is latched in the status word.  n_patterns = 0 is FMX_OK and
 * launches nothing.  FMX_E_ARG: an index that holds no text, band >
 * FMX_VERIFY_MAX_BAND, max_cands outside 1..16, strand flags misused (as for
 * seeds), a null or misaligned pointer, more slots than a launch's 2^31 - 1
 * workgroups of four hold.
 * One kernel, k_verify: a wavefront per candidate slot, lane k <= 2 band
 * owning diagonal P - band + k, a row of F per step — the read's symbols
 * fetched 64 at a time and broadcast, the text shifted along the lanes, the
 * in-row term a prefix-min scan over the lanes —, both passes one routine; no
 * LDS, no barrier.  Timer: "verify", one unit per candidate slot. */
#define FMX_VERIFY_MAX_BAND 31u
#define FMX_VERIFY_MAX_LEN  65535u
#define FMX_VERIFY_NONE     0xFFFFFFFFu
fmx_status fmx_verify_async(fmx_index *ix, const uint8_t *d_bytes, const uint64_t *d_offsets,
                            uint64_t n_patterns, uint32_t flags,
                            uint32_t max_cands, const uint32_t *d_ncands, const int64_t *d_pos,
                            uint32_t band, uint32_t max_dist,
                            uint32_t *d_dist, int64_t *d_tstart, int64_t *d_tend, void *stream);

/* Host buffers, synchronous: fmx_place_batch with the verify launch appended
 * on the same stream, in the same chunk loop (the reads are already in the
 * chunk's HBM; FMX_PLACE_CHUNK applies).  The first five outputs are exactly
 * fmx_place_batch's for the same arguments; out_dist, out_tstart and out_tend
 * (nv * max_cands each) are fmx_verify_async applied to them with align_band
 * and max_dist.  FMX_E_ARG as for both calls. */
fmx_status fmx_map_batch(fmx_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                         uint64_t n_patterns, uint32_t flags,
                         uint32_t max_seeds, uint32_t min_len, uint32_t skip, uint64_t max_occ,
                         uint32_t band, uint32_t min_cover, uint32_t max_cands,
                         uint32_t align_band, uint32_t max_dist,
                         uint32_t *out_ncands, uint32_t *out_flags,
                         int64_t *out_pos, uint32_t *out_cover, uint32_t *out_mask,
                         uint32_t *out_dist, int64_t *out_tstart, int64_t *out_tend);

/* Wait for `stream` and return (and clear) the latched device status. */
fmx_status fmx_sync(fmx_index *ix, void *stream);

/* The caller is done with `stream` (e.g. before hipStreamDestroy): wait for it,
 * return (and clear) its latched status like fmx_sync, and free its status
 * word for reuse.  Optional: an index holds 1024 status words and recycles
 * the least recently used one whose stream has no launch in flight, so a
 * caller that makes a stream per request never runs out; bits latched on a
 * recycled word and never read are dropped.  A destroyed stream's handle may
 * be reused by a new stream, which then shares the old status word — release
 * (or sync) a stream before destroying it. */
fmx_status fmx_stream_release(fmx_index *ix, void *stream);

/* ----------------------------------------------------- several GPUs, one handle
 * The device mask of SURVEY §8(b) for a single-process caller (no process
 * group): one replica of the index per entry of `devices` (a device may be
 * listed more than once: replicas on one GPU run concurrently).  The blob is
 * validated like fmx_load (same codes), copied to HBM of devices[0] once and
 * from there device-to-device to the other replicas (hipMemcpyPeer: xGMI
 * between MI355X GPUs); each replica is an fmx_load_device index.  A host
 * batch is cut into n_replicas contiguous shards (sizes differ by at most
 * one) answered concurrently, and the results are concatenated in order:
 * exactly what fmx_count_batch / fmx_locate_batch on one device return for
 * the whole batch (same capacity contract: offsets and *needed are written,
 * FMX_E_CAPACITY if the total exceeds cap). */
typedef struct fmx_multi fmx_multi;

fmx_status fmx_multi_load(const uint8_t *blob, uint64_t blob_len, fmx_layout layout, const int *devices,
                          int n_devices, uint32_t options, fmx_multi **out, uint64_t *expected_total,
                          uint64_t *actual_total);
void fmx_multi_free(fmx_multi *m);
int fmx_multi_replicas(const fmx_multi *m);
/* Replica i's own index (for the device-buffer calls on its device); owned by m. */
fmx_index *fmx_multi_replica(fmx_multi *m, int i);
fmx_status fmx_multi_count_batch(fmx_multi *m, const uint8_t *bytes, const uint64_t *offsets,
                                 uint64_t n_patterns, uint32_t flags, void *out_counts);
fmx_status fmx_multi_locate_batch(fmx_multi *m, const uint8_t *bytes, const uint64_t *offsets,
                                  uint64_t n_patterns, uint32_t flags, uint64_t *out_loc_offsets,
                                  void *out_locs, uint64_t cap, uint64_t *needed);

/* --------------------------------------------------------------- timing
 * enable = k > 0: every k-th kernel launch (k = 1: every launch) is bracketed
 * by hipEvents on its stream; 0: off.  fmx_timing_read sums the bracketed
 * durations per kernel since timing was last enabled (enabling resets the
 * totals; fmx_timing_read synchronises).  An event pair costs the stream
 * several microseconds, so throughput runs sample (k > 1).  Timers: "count",
 * "locate" (a whole locate launch), "match" (a whole match launch), "seeds"
 * (a whole seed-chain launch, a unit per slot), "approx" (a whole k-mismatch
 * launch, a unit per slot), "vote" (k_vote, a unit per chain), "verify"
 * (k_verify, a unit per candidate slot) and, for
 * fmx_locate_group_async, its two kernels "locate.search" (k_search) and
 * "locate.emit" (k_emit). */
fmx_status fmx_timing_enable(fmx_index *ix, int enable);
fmx_status fmx_timing_read(fmx_index *ix, fmx_kernel_timing *out, int max_entries, int *n_entries);

/* --------------------------------------------------------------- builder
 * FmIndexBuilder (src/builder/mod.rs): blob_size (:165-181) and build (:187-264),
 * on the GPU.  kmer_size 1 = LookupTableConfig::None, >= 2 = KmerSize(k);
 * sampling_ratio 1 = SuffixArrayConfig::Uncompressed, >= 2 = Compressed(r).
 * table: 256-byte EncodingTable (host memory), or NULL for PassThrough. */
fmx_status fmx_build_blob_size(uint64_t text_len, uint32_t symbol_count, fmx_layout layout,
                               uint32_t kmer_size, uint32_t sampling_ratio, uint64_t *out_size);

/* d_text and d_blob are device buffers on `device`; d_blob must be 16-B aligned
 * and exactly fmx_build_blob_size bytes.  Synchronous: starts after all work
 * already queued on the device (whichever stream wrote d_text) and returns
 * when the blob is complete. */
fmx_status fmx_build_device(const uint8_t *d_text, uint64_t text_len, const uint8_t *table,
                            uint32_t symbol_count, fmx_layout layout, uint32_t kmer_size,
                            uint32_t sampling_ratio, uint8_t *d_blob, uint64_t blob_len, int device);

/* Host-buffer convenience: uploads the text, builds on `device`, downloads the blob. */
fmx_status fmx_build(const uint8_t *text, uint64_t text_len, const uint8_t *table,
                     uint32_t symbol_count, fmx_layout layout, uint32_t kmer_size,
                     uint32_t sampling_ratio, uint8_t *blob, uint64_t blob_len, int device);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H */
