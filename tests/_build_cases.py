"""The blob builder (fmx_build / fmx_build_device: fmx_build.hip): the cases,
their bodies and the floors the emulator tests (test_build_simt.py) and the GPU
tests (test_gpu_build.py) share.  The reference throughout is the oracle's
builder (O.build), compared blob byte for byte; where a case loads the blob,
the oracle's counts and locations are compared element-wise (check_parity,
which tests/test_gpu.py uses too).

Every class floor is asserted on the inputs and the reference alone, before
the engine is called:
  * the doubling depth of a text is max_lcp(): the longest common prefix of
    two neighbouring suffixes in a plainly sorted suffix list (Python's sort of
    the byte strings).  The builder's first sort settles K0 = 64 // bits
    symbols; a text needs no doubling round when max_lcp < K0, and round r
    (h = K0 * 2^r) settles every group whose common prefix is below 2 * h;
  * the 64-bit path's first-two-symbol buckets are counted by bucket_sizes()
    from the encoded text (the sentinel's own bucket and the last symbol's
    included, as the builder counts them);
  * block counts, k-mer table sizes and sampled lengths come from the blob
    size formula restated here (blocks_len = n // V + 1, kt_len = (sigma+1)^k,
    sa_len = ceil(n / sr)) and are then read back from the reference's header.
"""
import ctypes as C
import os

import numpy as np
import pytest

from _util import (SIMT_LAYOUTS, block_of, pos_of, rand_chr_list, rand_pattern, rand_text, table_from_symbols)

WIDE_LAYOUT = (8, 6, 32)  # sigma above 32 (no SIMT_LAYOUTS entry has six planes)
DOUBLING_SIGMAS = (2, 4, 21, 64)
# the texts of one alphabet size, in groups (planted{r}: one repeat of K0 * 2^r - 1, K0 * 2^r and K0 * 2^r + 1)
DOUBLING_GROUPS = ("runs", "periodic", "planted0", "planted1", "planted3", "tails")
OCC_MODES = (0, 1, 63)


# ----------------------------------------------------- the engine's builder

def engine_build(pkg, text, sigma, pb, planes, vb, k, sr, table):
    """FmIndexBuilder.build of the engine library in use (the GPU's, or the
    emulator's while a `simt` fixture is active)."""
    enc = pkg.text_encoders.EncodingTable(table) if table is not None else pkg.text_encoders.PassThrough()
    LT = pkg.build_config.LookupTableConfig.KmerSize(k) if k > 1 else pkg.build_config.LookupTableConfig.None_()
    SA = pkg.build_config.SuffixArrayConfig.Compressed(sr) if sr > 1 else pkg.build_config.SuffixArrayConfig.Uncompressed()
    b = (pkg.FmIndexBuilder(len(text), sigma, enc, pos_of(pkg, pb), block_of(pkg, planes, vb))
         .set_lookup_table_config(LT).set_suffix_array_config(SA))
    blob = pkg.aligned_buffer(b.blob_size())
    b.build(np.frombuffer(bytes(text), np.uint8), blob)
    return blob


def raw_build(pkg, text, sigma, pb, planes, vb, k, sr, table, blob=None, blob_len=None):
    """fmx_build through the C ABI alone: (status, blob).  blob / blob_len: a
    caller's buffer (any alignment) and the length to claim for it."""
    n_ = pkg._native
    L = n_.fmx_layout(pb, planes, vb, n_.FMX_ENC_TABLE if table is not None else n_.FMX_ENC_PASS)
    size = C.c_uint64()
    assert n_.lib().fmx_build_blob_size(len(text), sigma, L, k, sr, C.byref(size)) == 0
    if blob is None:
        blob = pkg.aligned_buffer(size.value)
    t = np.frombuffer(bytes(text), np.uint8)
    tb = None if table is None else C.create_string_buffer(bytes(table), 256)
    st = n_.lib().fmx_build(t.ctypes.data if t.size else None, t.size, tb, sigma, L, k, sr, blob.ctypes.data,
                            size.value if blob_len is None else blob_len, 0)
    return st, blob


def assert_blob(pkg, O, text, sigma, lay, k, sr, table, what=""):
    """The engine's blob equals the oracle's, byte for byte; returns it."""
    pb, planes, vb = lay
    ref = O.build(text, sigma, O.layout(pb, planes, vb), k, sr, table)
    blob = engine_build(pkg, text, sigma, pb, planes, vb, k, sr, table)
    if not np.array_equal(blob, ref):
        at = np.flatnonzero(np.asarray(blob) != ref)
        pytest.fail(f"builder differs {what} n={len(text)} sigma={sigma} layout={lay} k={k} sr={sr}: {at.size} bytes, "
                    f"first at {int(at[0])} of {ref.size}")
    return blob


class sa_path:
    """FMX_BUILD_SA64 set ("64") or unset ("32") inside the block."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        self.saved = os.environ.pop("FMX_BUILD_SA64", None)
        if self.path == "64":
            os.environ["FMX_BUILD_SA64"] = "1"

    def __exit__(self, *a):
        os.environ.pop("FMX_BUILD_SA64", None)
        if self.saved is not None:
            os.environ["FMX_BUILD_SA64"] = self.saved


# ------------------------------------------------- parity of a loaded blob

class BufferWatch:
    """Copies of the caller's buffers (patterns, offsets, blob) taken before
    the oracle reads them, compared after the oracle call and after every GPU
    call: a recurrence of the round-4 failure (the GPU answered
    as if a few pattern bytes differed from the caller's buffer) classifies
    itself — the message names the first call after which a buffer differed
    from its copy, and where, or says that every buffer was intact."""

    def __init__(self, **bufs):
        self.bufs = bufs
        self.copies = {k: np.array(v, copy=True) for k, v in bufs.items()}
        self.first_change = None

    def check(self, after):
        if self.first_change:
            return
        for k, v in self.bufs.items():
            if not np.array_equal(v, self.copies[k]):
                at = np.flatnonzero(np.asarray(v).view(np.uint8) != self.copies[k].view(np.uint8))
                self.first_change = f"{k} changed after {after} at bytes {at[:8].tolist()}"
                return

    def report(self):
        return self.first_change or "caller's buffers intact after every call"


def diagnose(pkg, ix, load, data, offsets, pats, goff, ooff):
    """On a count mismatch, what the failure looks like (kept in the assert
    message): the patterns that differ, whose count they got, the count path's
    answer for them, whether the same call differs again (three reruns on this
    index) and the answer of a fresh index in launch order (FMX_GROUPED=0)."""
    oc = np.diff(ooff.astype(np.int64))
    bad = np.flatnonzero(np.diff(goff.astype(np.int64)) != oc)
    gc = np.diff(goff.astype(np.int64))
    out = [f"{bad.size} of {len(pats)} patterns differ"]
    for b in bad[:6]:
        same = sorted({pats[j] for j in np.flatnonzero(oc == gc[b])})[:3]
        out.append(f"pat {b} {pats[b]!r}: gpu {gc[b]} oracle {oc[b]} (the oracle count of {same!r})")
    try:
        d2, o2 = pkg.pack_patterns(pats)
        if not (np.array_equal(d2, data) and np.array_equal(o2, offsets)):
            diff = np.flatnonzero(d2 != data)
            out.append(f"the caller's pattern buffer changed since packing at bytes {diff[:8].tolist()}")
        c2 = ix.count_batch((d2.copy(), o2.copy())).astype(np.int64)
        out.append(f"count path on a fresh copy: {np.flatnonzero(c2 != oc).size} differ")
        cnt = ix.count_batch((data, offsets)).astype(np.int64)
        out.append(f"count path on those: {cnt[bad[:6]].tolist()}")
        for r in range(3):
            g2, _ = ix.locate_batch((data, offsets))
            b2 = np.flatnonzero(np.diff(g2.astype(np.int64)) != oc)
            out.append(f"rerun {r}: {b2.size} differ {b2[:6].tolist()}")
        saved = os.environ.get("FMX_GROUPED")
        os.environ["FMX_GROUPED"] = "0"
        try:
            ix2 = load()
            g3, _ = ix2.locate_batch((data, offsets))
            ix2.close()
        finally:
            if saved is None:
                os.environ.pop("FMX_GROUPED", None)
            else:
                os.environ["FMX_GROUPED"] = saved
        b3 = np.flatnonzero(np.diff(g3.astype(np.int64)) != oc)
        out.append(f"fresh index, launch order: {b3.size} differ {b3[:6].tolist()}")
    except Exception as e:  # (the diagnosis must not hide the original failure)
        out.append(f"diagnosis stopped: {e!r}")
    return "; ".join(out)


def check_parity(pkg, O, blob, pb, planes, vb, enc, pats, occ, reversed_too=True, expect_path=None):
    """Counts and locations of `pats` on the GPU against the oracle, forward
    (and reversed).  expect_path: "grouped" / "grouped_raw" / "ordered" —
    the launch path the first locate must have taken (fmx_index_info's
    launch counters)."""
    L = O.layout(pb, planes, vb, enc)
    data, offsets = pkg.pack_patterns(pats)
    watch = BufferWatch(data=data, offsets=offsets, blob=blob)
    orc = O.OracleIndex(blob, L)
    encoder = pkg.text_encoders.EncodingTable if enc == 0 else pkg.text_encoders.PassThrough

    def load():
        return pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), encoder, options=occ)
    ooff, olocs = orc.locate_batch(data, offsets)
    watch.check("the oracle")
    ix = load()
    watch.check("FmIndex.load")
    goff, glocs = ix.locate_batch((data, offsets))
    watch.check("locate_batch")
    if expect_path is not None:
        info = ix.info()
        took = {k: info["launches_" + k] for k in ("grouped", "grouped_raw", "ordered")}
        assert took[expect_path] >= 1 and sum(took.values()) == took[expect_path], \
            f"the locate did not run {expect_path} alone: {took}"
    if not np.array_equal(goff, ooff):
        pytest.fail("per-pattern counts / offsets differ: " + diagnose(pkg, ix, load, data, offsets, pats, goff,
                                                                        ooff) + "; " + watch.report())
    assert np.array_equal(glocs, olocs), "locations differ (SA-row order); " + watch.report()
    cnt = ix.count_batch((data, offsets))
    watch.check("count_batch")
    assert np.array_equal(cnt.astype(np.uint64), np.diff(ooff)), "count path differs; " + watch.report()
    if reversed_too:
        rpats = [p[::-1] for p in pats]
        rc = ix.count_batch(rpats, reversed=True)
        assert np.array_equal(rc, cnt)
        roff, rlocs = ix.locate_batch(rpats, reversed=True)
        assert np.array_equal(roff, ooff) and np.array_equal(rlocs, olocs)
    ix.close()
    watch.check("close")
    assert watch.first_change is None, watch.report()
    return ooff, olocs


# -------------------------------------------------- (a) the layout sweep's inputs

def every_layout_inputs(pb, planes, vb, min_len=300, max_len=2000, n_sub=300, n_absent=50):
    """The inputs of the get_accurate_result-style sweep of one layout
    (tests/test_gpu.py::test_builder_and_queries_every_layout), one tuple per
    alphabet size: (sigma, chars, table, text, k, sr, patterns).  One generator,
    seeded by the layout; the draws come in this order whoever asks."""
    rng = np.random.default_rng(pb * 1000 + planes * 100 + vb)
    for sigma in sorted({2, 3, (1 << planes) // 2 + 1, 1 << planes}):
        chars = rand_chr_list(rng, sigma)
        table = table_from_symbols([bytes([c]) for c in chars])
        text = rand_text(rng, chars, min_len, max_len)
        k, sr = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        if (sigma + 1) ** k > 1 << 20:
            k = 2
        pats = [rand_pattern(rng, text, 1, 24) for _ in range(n_sub)]
        pats += [bytes(rng.choice(np.frombuffer(chars, np.uint8), size=int(rng.integers(1, 12))))
                 for _ in range(n_absent)]                              # mostly absent
        pats += [b"\x00", b"\x7f\x7f", chars[:1] * 2]              # wildcard bytes, short repeats
        yield sigma, chars, table, text, k, sr, pats


def every_layout(pkg, O, pb, planes, vb, load=True):
    """(a): texts of 300 to 600 bytes over sigma in {2, 3, 2^planes / 2 + 1,
    2^planes}, k and sr as the GPU sweep draws them: the blob's bytes, and —
    load — 60 patterns on the blob the engine built, at options 0 and 1."""
    for sigma, chars, table, text, k, sr, pats in every_layout_inputs(pb, planes, vb, 300, 600, 50, 7):
        assert 300 <= len(text) <= 600 and len(pats) == 60
        blob = assert_blob(pkg, O, text, sigma, (pb, planes, vb), k, sr, table)
        if load:
            for occ in (0, 1):
                check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)


# -------------------------------------------------------- (b) doubling depth

def k0_of(sigma):
    """Symbols packed into the builder's first 64-bit key: 64 // bits(sigma + 1)."""
    b = 1
    while (1 << b) < sigma + 1:
        b += 1
    return 64 // b


assert [k0_of(s) for s in DOUBLING_SIGMAS] == [32, 21, 12, 9]


def layout_for(sigma):
    return WIDE_LAYOUT if sigma > 32 else {2: SIMT_LAYOUTS[1], 4: SIMT_LAYOUTS[0], 21: SIMT_LAYOUTS[2]}.get(
        sigma, SIMT_LAYOUTS[3] if sigma <= 16 else SIMT_LAYOUTS[2])


def max_lcp(idx):
    """The longest common prefix of two neighbouring suffixes of the symbol
    string `idx` (bytes), from Python's sort of the suffixes themselves."""
    e = bytes(idx)
    n = len(e)
    sa = sorted(range(n), key=lambda i: e[i:])
    a = np.frombuffer(e, np.uint8)
    best = 0
    for x, y in zip(sa, sa[1:]):
        m = n - max(x, y)
        if m <= best:
            continue
        ne = np.flatnonzero(a[x:x + m] != a[y:y + m])
        best = max(best, int(ne[0]) if ne.size else m)
    return best


def _planted(rng, sigma, L):
    """A random text with one repeat of exactly L symbols: the copies' left
    and right neighbours differ, so the repeat is not part of a longer one."""
    n = 2 * L + 260
    x = rng.integers(0, sigma, size=n).astype(np.uint8)
    a, b = 50, 50 + L + 150
    x[b:b + L] = x[a:a + L]
    x[b - 1] = (x[a - 1] + 1) % sigma
    x[b + L] = (x[a + L] + 1) % sigma
    return x


def _fibonacci(count):
    a, b = [1], [0]
    while len(b) < count:
        a, b = b, b + a
    return np.array(b[:count], np.uint8)


_DOUBLING = {}


def doubling_texts(sigma):
    """(b): {group: [(name, text bytes, symbol indices)]} for one alphabet size,
    the table (None: PassThrough, for sigma 4 and 64) and every text's max_lcp;
    floors asserted here.  Built once."""
    if sigma in _DOUBLING:
        return _DOUBLING[sigma]
    rng = np.random.default_rng(7000 + sigma)
    K0 = k0_of(sigma)
    groups = {g: [] for g in DOUBLING_GROUPS}
    mid = np.uint8(sigma // 2)
    for n in (1, 2, 255, 256, 257, 777):
        groups["runs"].append((f"run{n}", np.full(n, mid, np.uint8)))
    per = groups["periodic"]
    per.append(("period2", np.tile(np.array([0, sigma - 1], np.uint8), 300)))
    for p in (K0 - 1, K0, K0 + 1):
        w = rng.integers(0, sigma, size=p).astype(np.uint8)
        w[0], w[-1] = 0, sigma - 1  # (its period is p, not a divisor of p)
        w[1:-1] = np.where(w[1:-1] == 0, 1 % sigma, w[1:-1]) if sigma > 2 else 1
        per.append((f"period{p}", np.tile(w, 700 // p + 1)[:700]))
    half = rng.integers(0, sigma, size=400).astype(np.uint8)
    per.append(("halves", np.concatenate([half, half])))
    per.append(("fibonacci", _fibonacci(987) * np.uint8(sigma - 1)))
    for r in (0, 1, 3):
        for d in (-1, 0, 1):
            L = K0 * (1 << r) + d
            groups[f"planted{r}"].append((f"planted{K0}x{1 << r}{d:+d}", _planted(rng, sigma, L), L))
    body = rng.integers(0, sigma, size=500).astype(np.uint8)
    groups["tails"].append(("tail-smallest", np.concatenate([body, np.zeros(300, np.uint8)])))
    groups["tails"].append(("tail-largest", np.concatenate([body, np.full(300, sigma - 1, np.uint8)])))
    table = None
    if sigma in (2, 21):
        chars = rand_chr_list(rng, sigma)
        table = table_from_symbols([bytes([c]) for c in sorted(chars)])
        lut = np.array(sorted(chars), np.uint8)
    out, lcps = {}, {}
    for g, items in groups.items():
        out[g] = []
        for it in items:
            name, idx = it[0], it[1]
            assert idx.size <= 4096 and int(idx.max()) < sigma
            lcp = max_lcp(idx.tobytes())
            if len(it) == 3:
                assert lcp == it[2], f"{name}: the planted repeat of {it[2]} is not the longest ({lcp})"
            lcps[name] = lcp
            out[g].append((name, (lut[idx] if table is not None else idx).tobytes()))
    # the floors: no round, one round, and four or more (h = K0, 2 K0, 4 K0, 8 K0)
    v = sorted(lcps.values())
    assert v[0] < K0 and any(K0 <= x < 2 * K0 for x in v) and v[-1] >= 8 * K0, (sigma, K0, lcps)
    for edge in (K0, 2 * K0, 8 * K0):   # either side of every K0 * 2^r visited
        assert {edge - 1, edge, edge + 1} <= set(v), (sigma, edge, v)
    _DOUBLING[sigma] = (out, table, lcps)
    return _DOUBLING[sigma]


def doubling(pkg, O, sigma, group, path):
    """(b) and (c): every text of one group on one suffix-array path."""
    texts, table, _ = doubling_texts(sigma)
    lay = layout_for(sigma)
    with sa_path(path):
        for i, (name, text) in enumerate(texts[group]):
            assert_blob(pkg, O, text, sigma, lay, 1 + i % 3 if sigma < 21 else 1 + i % 2, 1 + i % 4, table, name)


# ------------------------------------------------ (c) the 64-bit path's buckets

def bucket_sizes(idx, sigma):
    """Suffixes per first-two-symbol bucket as suffix_array64 counts them: the
    symbols are index + 1, the sentinel and everything past it 0."""
    t = np.concatenate([np.frombuffer(bytes(idx), np.uint8).astype(np.int64) + 1, np.zeros(2, np.int64)])
    W = sigma + 1
    return np.bincount(t[:-1] * W + t[1:], minlength=W * W)


def bucket_cases():
    """[(name, sigma, symbol indices)]: one non-empty bucket (the empty text:
    the sentinel's), the fewest a non-empty text can have, buckets of exactly
    one suffix next to full ones, and 1,000 or more of sigma 64's 4,225."""
    rng = np.random.default_rng(6464)
    out = [("one-bucket", 4, np.zeros(0, np.uint8))]
    assert np.count_nonzero(bucket_sizes(out[0][2], 4)) == 1
    run = np.full(300, 2, np.uint8)
    b = bucket_sizes(run, 4)
    assert np.count_nonzero(b) == 3 and sorted(b[b > 0]) == [1, 1, 299]
    out.append(("three-buckets", 4, run))
    x = rng.integers(0, 3, size=400).astype(np.uint8)
    x[200], x[201] = 3, 3   # the only 3s: buckets (3,3) and (3,x) hold one suffix each
    b = bucket_sizes(x, 4)
    assert b[4 * 5 + 4] == 1 and (b == 1).sum() >= 3 and b.max() >= 30
    out.append(("single-suffix-buckets", 4, x))
    # every (a, b) with a < 16 once, in an order that makes each joint a new pair too
    wide = np.array([s for a in range(16) for b in range(64) for s in (a, b)], np.uint8)[:1100]
    nb = int(np.count_nonzero(bucket_sizes(wide, 64)))
    assert nb >= 1000, nb
    out.append(("thousand-buckets", 64, wide))
    return out


def buckets(pkg, O, name):
    sigma, idx = next((s, x) for n_, s, x in bucket_cases() if n_ == name)
    with sa_path("64"):
        assert_blob(pkg, O, idx.tobytes(), sigma, layout_for(sigma), 2, 2, None, name)


# ------------------------------------------------------------ (d) size edges

def header_fields(blob, lay, table):
    """kt_len, sa_len, ckpt_len, blocks_len from a blob's headers (the layout
    fmx_build.hip's build_typed writes: magic, table, count-array header,
    suffix-array header, bwm header, each padded to the vector's alignment)."""
    A = 16 if lay[2] == 128 else 8
    up = lambda x: -(-x // A) * A  # noqa: E731
    o = up(8) + (up(256) if table is not None else 0)
    b = np.asarray(blob)
    kt_len = int(b[o + 16:o + 24].view(np.uint64)[0])
    o += up(24)
    sa_len = int(b[o + 8:o + 16].view(np.uint64)[0])
    o += up(16)
    return dict(kt_len=kt_len, sa_len=sa_len, ckpt_len=int(b[o + 8:o + 16].view(np.uint64)[0]),
                blocks_len=int(b[o + 16:o + 24].view(np.uint64)[0]))


ACGT = b"ACGT"
ACGT_TABLE = table_from_symbols([b"A", b"C", b"G", b"T"])


def small_sizes(pkg, O, path):
    """n + 1 = 255, 256, 257 (one workgroup, exactly, and one symbol more), n = 0 and n = 1; both encoders."""
    rng = np.random.default_rng(255)
    with sa_path(path):
        for n in (0, 1, 254, 255, 256):
            text = bytes(rng.choice(np.frombuffer(ACGT, np.uint8), size=n)) if n else b""
            assert_blob(pkg, O, text, 4, SIMT_LAYOUTS[0], 3, 2, ACGT_TABLE)
            idx = bytes(rng.integers(0, 5, size=n).astype(np.uint8))
            assert_blob(pkg, O, idx, 5, SIMT_LAYOUTS[3], 2, 3, None)


# blocks_len -> n at vector width 32 (blocks_len = n // 32 + 1: n % 32 == 0 appends an empty block, which for
# 1,024 is the chunk's last block and for 1,025 the only block of a second chunk)
BLOCK_EDGES = {1023: 32 * 1022 + 31, 1024: 32 * 1023, 1025: 32 * 1024, 2049: 32 * 2048 + 7}
assert all(n // 32 + 1 == b for b, n in BLOCK_EDGES.items())


def block_edge(pkg, O, blocks_len):
    """k_chunk_totals / k_ckpt at their chunk of 1,024 blocks."""
    n = BLOCK_EDGES[blocks_len]
    lay = SIMT_LAYOUTS[1]
    assert lay[2] == 32
    rng = np.random.default_rng(blocks_len)
    text = bytes(rng.choice(np.frombuffer(ACGT, np.uint8), size=n))
    ref = O.build(text, 4, O.layout(*lay), 2, 4, ACGT_TABLE)
    assert header_fields(ref, lay, ACGT_TABLE)["blocks_len"] == blocks_len
    assert_blob(pkg, O, text, 4, lay, 2, 4, ACGT_TABLE)


def kt_edges():
    """((sigma, k) of the largest (sigma + 1)^k <= 8192, ... of the smallest > 8192), over every alphabet
    a block holds and every k the builder takes."""
    sizes = {(s + 1) ** k: (s, k) for s in range(64, 0, -1) for k in range(40, 0, -1) if (s + 1) ** k < 1 << 32}
    below, above = max(x for x in sizes if x <= 8192), min(x for x in sizes if x > 8192)
    return (below,) + sizes[below], (above,) + sizes[above]


def kmer_counts(idx, sigma, k):
    """The k-mer histogram of count_array.rs:110-123 (digits index + 1, 0 past the end), plainly."""
    t = np.concatenate([np.frombuffer(bytes(idx), np.uint8).astype(np.int64) + 1, np.zeros(k, np.int64)])
    code = np.zeros(len(idx), np.int64)
    for j in range(k):
        code = code * (sigma + 1) + t[j:j + len(idx)]
    return np.bincount(code, minlength=(sigma + 1) ** k)


def kt_edge(pkg, O, side):
    """k_kmer_hist on either side of its switch from an LDS histogram to
    global atomics (kt_len > 8192), with a bin that counts past 255.  Returns
    kt_len."""
    (lo, s_lo, k_lo), (hi, s_hi, k_hi) = kt_edges()
    assert (lo, s_lo, k_lo) == (8192, 1, 13) and (hi, s_hi, k_hi) == (9261, 20, 3)
    kt_len, sigma, k = (lo, s_lo, k_lo) if side == "lds" else (hi, s_hi, k_hi)
    rng = np.random.default_rng(kt_len)
    if sigma == 1:
        idx = np.zeros(420, np.uint8)
    else:
        idx = np.concatenate([rng.integers(0, sigma, size=300), np.full(300, 3), rng.integers(0, sigma, size=200)])
        idx = idx.astype(np.uint8)
    assert kmer_counts(idx, sigma, k).max() > 255
    lay = SIMT_LAYOUTS[1] if sigma == 1 else SIMT_LAYOUTS[2]
    ref = O.build(idx.tobytes(), sigma, O.layout(*lay), k, 2, None)
    assert header_fields(ref, lay, None)["kt_len"] == kt_len
    assert_blob(pkg, O, idx.tobytes(), sigma, lay, k, 2, None)
    return kt_len


def sampling_edges(pkg, O):
    """sr = 1, above n, and sa_len on either side of a change (n % sr == 0 and +- 1)."""
    rng = np.random.default_rng(10)
    lay = SIMT_LAYOUTS[3]
    want = {(300, 1): 300, (300, 305): 1, (299, 10): 30, (300, 10): 30, (301, 10): 31}
    for (n, sr), sa_len in want.items():
        text = bytes(rng.choice(np.frombuffer(ACGT, np.uint8), size=n))
        ref = O.build(text, 4, O.layout(*lay), 2, sr, ACGT_TABLE)
        assert header_fields(ref, lay, ACGT_TABLE)["sa_len"] == sa_len == -(-n // sr)
        assert_blob(pkg, O, text, 4, lay, 2, sr, ACGT_TABLE)


# ---------------------------------------------------------------- (e) errors

ERROR_LAYOUT = (4, 3, 64)
ERROR_CASES = [(enc, at) for enc in ("table", "pass") for at in ("first", "last", "middle")] + ["blob_len", "align"]


def error_case(pkg, O, case, path):
    """A failing build, its status, then a correct build in the same process,
    byte exact.  case: (encoder, where the one bad byte sits), "blob_len"
    (FMX_E_CONFIG) or "align" (FMX_E_ALIGN)."""
    n_ = pkg._native
    pb, planes, vb = ERROR_LAYOUT
    rng = np.random.default_rng(600)
    good = bytes(rng.choice(np.frombuffer(ACGT, np.uint8), size=600))
    with sa_path(path):
        if case == "blob_len":
            st, _ = raw_build(pkg, good, 4, pb, planes, vb, 2, 2, ACGT_TABLE, blob_len=16)
            assert st == n_.FMX_E_CONFIG, st
            ref_args = (good, 4, (pb, planes, vb), 2, 2, ACGT_TABLE)
        elif case == "align":
            size = O.blob_size(600, 4, O.layout(pb, planes, vb, 0), 2, 2)
            raw = pkg.aligned_buffer(size + 16)
            st, _ = raw_build(pkg, good, 4, pb, planes, vb, 2, 2, ACGT_TABLE, blob=raw[4:4 + size])
            assert raw[4:].ctypes.data % 8 == 4 and st == n_.FMX_E_ALIGN, st
            ref_args = (good, 4, (pb, planes, vb), 2, 2, ACGT_TABLE)
        else:
            enc, where = case
            at = {"first": 0, "last": 599, "middle": 300}[where]   # 300: the second workgroup's
            if enc == "table":
                table = bytearray(ACGT_TABLE)
                table[ord("!")] = 4       # an index >= symbol_count
                table, bad, ok = bytes(table), bytearray(good), good
                bad[at] = ord("!")
            else:
                table, ok = None, bytes(rng.integers(0, 4, size=600).astype(np.uint8))
                bad = bytearray(ok)
                bad[at] = 4
            st, _ = raw_build(pkg, bytes(bad), 4, pb, planes, vb, 2, 2, table)
            assert st == n_.FMX_E_SYMBOL, (case, st)
            ref_args = (ok, 4, (pb, planes, vb), 2, 2, table)
        assert_blob(pkg, O, *ref_args, what=f"after {case}")


# ------------------------------------------ (f) guard bands of fmx_build_device

def device_guard(pkg, O, mem_cls, lay, n, skew):
    """fmx_build_device with d_text carved at exactly n bytes, `skew` past a
    16-byte boundary, and d_blob at exactly blob_size bytes, in an arena that
    is 0xA5 everywhere else and in the blob area too: afterwards the guards
    and the text are untouched and the blob is the oracle's (written into a
    zeroed buffer); then fmx_load_device on it answers a small batch."""
    from _guard_cases import FILL_GUARD, Arena
    pb, planes, vb = lay
    rng = np.random.default_rng(n * 16 + skew)
    text = bytes(rng.choice(np.frombuffer(ACGT, np.uint8), size=n))
    k, sr = 2, 2
    ref = O.build(text, 4, O.layout(pb, planes, vb), k, sr, ACGT_TABLE)
    arena = Arena(mem_cls)
    arena.carve("text", n, 1, skew, data=np.frombuffer(text, np.uint8))
    arena.carve("blob", ref.size, 16, 0, fill=FILL_GUARD)
    arena.commit()
    assert arena.ptr("text") % 16 == skew and arena.ptr("blob") % 16 == 0
    assert (arena.host0[arena.bufs["blob"][0]:][:ref.size] == FILL_GUARD).all()
    table = pkg.text_encoders.EncodingTable(ACGT_TABLE)
    b = (pkg.FmIndexBuilder(n, 4, table, pos_of(pkg, pb), block_of(pkg, planes, vb))
         .set_lookup_table_config(pkg.build_config.LookupTableConfig.KmerSize(k))
         .set_suffix_array_config(pkg.build_config.SuffixArrayConfig.Compressed(sr)))
    assert b.blob_size() == ref.size
    b.build_device(arena.ptr("text"), arena.ptr("blob"), ref.size)
    arena.image()
    what = f"fmx_build_device layout={lay} n={n} skew={skew}"
    arena.check_guards_and_inputs(what)
    assert np.array_equal(arena.view("blob"), ref), f"{what}: the blob differs from the oracle's"
    ix = pkg.FmIndex.load_device(arena.ptr("blob"), ref.size, pos_of(pkg, pb), block_of(pkg, planes, vb))
    pats = [text[i:i + m] for i in range(0, n, 17) for m in (1, 2, 3) if i + m <= n] + [b"GATTACA", b"T"]
    data, offsets = pkg.pack_patterns(pats)
    ooff, olocs = O.OracleIndex(ref, O.layout(pb, planes, vb, 0)).locate_batch(data, offsets)
    goff, glocs = ix.locate_batch((data, offsets))
    assert np.array_equal(goff, ooff) and np.array_equal(glocs, olocs), f"{what}: fmx_load_device answers differ"
    ix.close()
    arena.image()
    arena.check_guards_and_inputs(what + " after the queries")
    assert np.array_equal(arena.view("blob"), ref), f"{what}: the loaded blob changed"
