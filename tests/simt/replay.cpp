// TEST INFRASTRUCTURE — a stand-alone host of the C ABI (include/fmx.h) for
// tests/test_build_simt.py::test_replay_program_sanitized: linked against the
// emulator's objects rebuilt under the host's address and undefined-behaviour
// sanitizers (make replay), run as a child process, never on a GPU.
//
//   replay IN OUT
//
// IN holds jobs (every array as a u64 byte count and its bytes): a header of
// u64s {expected build status, sigma, P bytes, planes, vector bits, encoder,
// k, sr, patterns, n options, options[4], the blob length to claim (0: the
// right one), the blob's skew past a 16-byte boundary}, the text, the
// 256-byte table (or none), the packed pattern bytes and their offsets.  Per
// job: fmx_build; then per load option, in the order check_parity
// (tests/_build_cases.py) calls them, fmx_load, fmx_locate_batch,
// fmx_count_batch, fmx_count_batch and fmx_locate_batch with reversed
// patterns, fmx_free.  OUT receives the build status, the blob, and per
// option and direction the location offsets, the locations and the counts.
// Exit status 0 when every call returned what the job expects.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fmx.h"

typedef std::vector<uint8_t> Bytes;

static bool get(FILE *f, Bytes *out) {
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1) return false;
    out->resize(n);
    return n == 0 || fread(out->data(), 1, n, f) == n;
}

static void put(FILE *f, const void *p, uint64_t n) {
    fwrite(&n, 8, 1, f);
    if (n) fwrite(p, 1, n, f);
}

#define REQUIRE(cond, ...)                \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fputc('\n', stderr);          \
            return 2;                     \
        }                                 \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 64;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 65;
    uint64_t jobs = 0;
    if (fread(&jobs, 8, 1, in) != 1) return 66;
    for (uint64_t j = 0; j < jobs; ++j) {
        Bytes head, text, table, data, offs;
        if (!get(in, &head) || !get(in, &text) || !get(in, &table) || !get(in, &data) || !get(in, &offs)) return 66;
        REQUIRE(head.size() == 16 * 8 && offs.size() % 8 == 0 && (table.empty() || table.size() == 256), "job %llu: format",
                (unsigned long long)j);
        uint64_t h[16];
        memcpy(h, head.data(), sizeof h);
        const fmx_layout L = {(uint32_t)h[2], (uint32_t)h[3], (uint32_t)h[4], (uint32_t)h[5]};
        const uint32_t sigma = (uint32_t)h[1], k = (uint32_t)h[6], sr = (uint32_t)h[7];
        const uint64_t npat = h[8], nopt = h[9], pb = L.pos_bytes;
        uint64_t size = 0;
        REQUIRE(fmx_build_blob_size(text.size(), sigma, L, k, sr, &size) == FMX_OK, "job %llu: blob size", (unsigned long long)j);
        // exactly what the caller owes: `size` bytes at the job's skew (rounded up to the allocator's 16-byte granule)
        const uint64_t claim = h[14] ? h[14] : size, skew = h[15];
        REQUIRE(skew < 16, "job %llu: skew", (unsigned long long)j);
        uint8_t *raw = static_cast<uint8_t *>(aligned_alloc(16, (size + skew + 15) / 16 * 16));
        uint8_t *blob = raw + skew;
        const fmx_status st = fmx_build(text.empty() ? nullptr : text.data(), text.size(), table.empty() ? nullptr : table.data(),
                                        sigma, L, k, sr, blob, claim, 0);
        const uint64_t st64 = (uint64_t)st;
        put(out, &st64, 8);
        put(out, blob, st == FMX_OK ? size : 0);
        REQUIRE(st64 == h[0], "job %llu: fmx_build returned %d, expected %llu", (unsigned long long)j, (int)st, (unsigned long long)h[0]);
        if (st != FMX_OK) {
            free(raw);
            continue;
        }
        std::vector<uint64_t> offsets(offs.size() / 8);
        memcpy(offsets.data(), offs.data(), offs.size());
        REQUIRE(offsets.size() == npat + 1, "job %llu: offsets", (unsigned long long)j);
        Bytes rev(data);
        for (uint64_t i = 0; i < npat; ++i)
            for (uint64_t a = offsets[i], b = offsets[i + 1]; a + 1 < b; ++a, --b) {
                const uint8_t t = rev[a];
                rev[a] = rev[b - 1];
                rev[b - 1] = t;
            }
        for (uint64_t o = 0; o < nopt; ++o) {
            fmx_index *ix = nullptr;
            uint64_t exp = 0, act = 0;
            REQUIRE(fmx_load(blob, size, L, 0, (uint32_t)h[10 + o], &ix, &exp, &act) == FMX_OK, "job %llu: fmx_load options %llu",
                    (unsigned long long)j, (unsigned long long)h[10 + o]);
            for (int dir = 0; dir < 2; ++dir) {
                const Bytes &d = dir ? rev : data;
                const uint32_t flags = dir ? FMX_PATTERN_REVERSED : 0u;
                std::vector<uint64_t> loff(npat + 1, 0);
                uint64_t cap = 1 << 16, needed = 0;
                Bytes locs(cap * pb), cnt((npat ? npat : 1) * pb);
                fmx_status q = FMX_OK;
                // forward: locate, then count; reversed: count, then locate (check_parity's order)
                for (int step = 0; step < 2; ++step) {
                    if ((step == 0) == (dir == 0)) {
                        q = fmx_locate_batch(ix, d.empty() ? nullptr : d.data(), offsets.data(), npat, flags, loff.data(),
                                             locs.data(), cap, &needed);
                        if (q == FMX_E_CAPACITY) {  // (as the Python API: once more with room for every location)
                            cap = needed;
                            locs.assign(cap * pb, 0);
                            q = fmx_locate_batch(ix, d.data(), offsets.data(), npat, flags, loff.data(), locs.data(), cap,
                                                 &needed);
                        }
                        REQUIRE(q == FMX_OK, "job %llu: fmx_locate_batch returned %d", (unsigned long long)j, (int)q);
                    } else {
                        q = fmx_count_batch(ix, d.empty() ? nullptr : d.data(), offsets.data(), npat, flags, cnt.data());
                        REQUIRE(q == FMX_OK, "job %llu: fmx_count_batch returned %d", (unsigned long long)j, (int)q);
                    }
                }
                put(out, loff.data(), loff.size() * 8);
                put(out, locs.data(), needed * pb);
                put(out, cnt.data(), npat * pb);
            }
            fmx_free(ix);
        }
        free(raw);
    }
    fclose(in);
    if (fclose(out) != 0) return 67;
    return 0;
}
