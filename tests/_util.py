"""Shared test helpers: random data in the shape of the reference's own
generators (sview-fmindex/src/tests/random_data/mod.rs:7-37, seeded here), and
a brute-force occurrence finder (the reference's accuracy contract,
src/tests/get_accurate_result/mod.rs:136-140).  Below them, what the emulator
and GPU twins of a query's tests share whatever the query: an index opened
beside its oracle, one cached text per alphabet, and the two device memories
(HostDev, TorchDev) their device-call scenarios run over."""
import numpy as np

# every (P bytes, planes, vector bits) the reference's tests sweep
# (get_accurate_result/mod.rs:179-222)
ALL_LAYOUTS = [(p, n, v) for p in (4, 8) for n in (2, 3, 4, 5, 6) for v in (32, 64, 128)]
# the few the emulator modules visit: u32 and u64 positions, every vector width, symbol-mask, paired and plain
# records among them
SIMT_LAYOUTS = [(4, 3, 64), (8, 2, 32), (4, 5, 128), (8, 4, 64)]


def table_from_symbols(symbols, with_wildcard=False):
    """EncodingTable::from_symbols[_with_wildcard] (encoding_table.rs:15-35)."""
    count = len(symbols) + (1 if with_wildcard else 0)
    t = bytearray([count - 1] * 256)
    for i, s in enumerate(symbols):
        for x in bytes(s):
            t[x] = i
    return bytes(t)


def rand_chr_list(rng, count):
    """gen_rand_chr_list: `count` distinct printable bytes (random_data/mod.rs:7-18)."""
    return bytes(rng.choice(np.arange(33, 127), size=count, replace=False).astype(np.uint8))


def rand_text(rng, chr_list, min_len, max_len):
    """gen_rand_text: every chr at least once, shuffled (random_data/mod.rs:20-30)."""
    n = int(rng.integers(min_len, max_len + 1))
    t = list(chr_list) + list(rng.choice(np.frombuffer(chr_list, np.uint8), size=max(0, n - len(chr_list))))
    rng.shuffle(t)
    return bytes(bytearray(int(x) for x in t))


def rand_pattern(rng, text, min_len, max_len):
    """gen_rand_pattern: a substring (random_data/mod.rs:31-37)."""
    m = int(rng.integers(min_len, max_len + 1))
    s = int(rng.integers(0, len(text) - m))
    return text[s:s + m]


def occurrences(text_idx: bytes, pat_idx: bytes):
    """All start positions of pat in text, over symbol indices."""
    m = len(pat_idx)
    out, i = [], text_idx.find(pat_idx)
    while i != -1:
        out.append(i)
        i = text_idx.find(pat_idx, i + 1)
    return out if m else []


def encode(table: bytes, data: bytes) -> bytes:
    return bytes(table[b] for b in data)


# Full-size blob provenance (the C2-C5 blobs' SHA-256 recorded).
# The text recipe is shared by tests/golden/make_blob_digests.py (the oracle's
# CPU builder, in this container) and tests/test_gpu_provenance.py (the GPU
# builder, on the box): numpy's PCG64 stream is the same on both.
ACGTN_SYMBOLS = [b"Aa", b"Cc", b"Gg", b"Tt", b"Nn"]
AMINO20 = b"ACDEFGHIKLMNPQRSTVWY"
PROVENANCE = {
    # name: (n, alphabet, symbols, (P bytes, planes, vector bits), seed)
    "c2": (1_000_000_000, b"ACGT", ACGTN_SYMBOLS, (4, 3, 64), 20261),
    "c4": (1_000_000_000, AMINO20, [bytes([c, c + 32]) for c in AMINO20] + [b"Xx"], (4, 5, 64), 20262),
}
PROVENANCE_K, PROVENANCE_SR = 3, 2


def provenance_text(name):
    """The seeded text of a provenance config: uniform over its alphabet."""
    n, alphabet, _, _, seed = PROVENANCE[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty(n, dtype=np.uint8)
    lut = np.frombuffer(alphabet, dtype=np.uint8)
    step = 1 << 26
    for c0 in range(0, n, step):
        c1 = min(n, c0 + step)
        out[c0:c1] = lut[rng.integers(0, len(alphabet), c1 - c0, dtype=np.uint8)]
    return out


def random_workspace_jobs(pkg, ix, orc, rng, text, sizes, length):
    """The job list of a group launch (fmx_locate_group_async) whose buffers
    start out full of random bytes: batch bi has sizes[bi] patterns of
    length(bi) bytes drawn from `text` (every third batch reversed), its
    offsets, locations, counts and workspace random, the oracle's answer in
    "want".  Returns (the batches' buffers, their jobs)."""
    bats, jobs = [], []
    for bi, n in enumerate(sizes):
        rev, m = bi % 3 == 2, length(bi)
        starts = rng.integers(0, text.size - m, size=n)
        pats = [text[s:s + m].tobytes() for s in starts]
        data, offsets = pkg.pack_patterns(pats)
        want = orc.locate_batch(data, offsets)
        q = [p[::-1] for p in pats] if rev else pats
        data, offsets = pkg.pack_patterns(q)
        cap = int(want[1].size) + 8
        ws = ix.locate_workspace_size(n)
        b = dict(n=n, want=want, data=np.concatenate([data, np.zeros(16, np.uint8)]),
                 off=offsets.view(np.int64).copy(), loff=rng.integers(0, 2**62, size=n + 1).astype(np.int64),
                 locs=rng.integers(0, 2**31, size=cap).astype(np.int32), need=np.zeros(1, np.int64),
                 cnt=rng.integers(0, 2**31, size=n).astype(np.int32),
                 ws=rng.integers(0, 256, size=ws).astype(np.uint8))
        jobs.append(ix.locate_job(b["data"].ctypes.data, b["off"].ctypes.data, n, b["loff"].ctypes.data,
                                  b["locs"].ctypes.data, cap, b["need"].ctypes.data, b["ws"].ctypes.data, ws,
                                  d_counts=b["cnt"].ctypes.data, reversed=rev, stage_kb=max(1, -(-256 * m // 1024)),
                                  fixed_len=m))
        bats.append(b)
    return bats, jobs


# ---------------------------------------------- an index and its oracle, per case

def pos_of(pkg, pb):
    return pkg.u32 if pb == 4 else pkg.u64


def block_of(pkg, planes, vb):
    return getattr(pkg.blocks, f"Block{planes}")(pkg.Vector(vb))


def open_index(pkg, O, case, pb, planes, vb, occ):
    """(the index loaded with options `occ`, the oracle over the same blob)."""
    blob = case.blob(O, pb, planes, vb)
    orc = O.OracleIndex(blob, O.layout(pb, planes, vb, 0))
    return pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=occ), orc


_CASES = {}


def case_for(planes, two_letters=False, **kw):
    """One text per alphabet size (_match_cases.Case; its expected values are
    computed once and shared by every test of the run)."""
    from _match_cases import Case  # (it imports this module)
    key = (planes, two_letters, tuple(sorted(kw.items())))
    if key not in _CASES:
        nchars = 2 if two_letters else min((1 << planes) - 1, 20)
        _CASES[key] = Case(planes * 11 + (5 if two_letters else 0), nchars, **kw)
    return _CASES[key]


# ------------------------------------------------------------ device memories

class _Dev:
    """What the device-call scenarios need of a device memory: put(array) ->
    (handle, pointer), get(handle, dtype) -> a flat host array, sync(), and
    `stream`, the hipStream_t to launch on (0: the index's own)."""
    stream = 0

    def filled(self, rnd, shape, dtype=np.uint32):
        """A buffer of random values from `rnd`: (handle, pointer, the host
        copy, kept so that what a launch must leave alone can be checked)."""
        a = rnd.integers(1, 2**31, shape).astype(dtype)
        return self.put(a) + (a,)

    def workspace(self, rnd, nbytes):
        """Random bytes (a workspace needs no initialisation), 256-byte
        aligned: (handle, pointer)."""
        h, p = self.put(rnd.integers(0, 256, nbytes + 256).astype(np.uint8))
        return h, p + (-p) % 256


class HostDev(_Dev):
    """The emulator: device memory is host memory."""

    def put(self, a):
        a = np.ascontiguousarray(a).copy()
        return a, a.ctypes.data

    def get(self, h, dtype):
        return h.view(np.uint8).reshape(-1).view(dtype)

    def sync(self):
        pass


class TorchDev(_Dev):
    """The GPU: one uint8 tensor per array.  caller_stream: launch on a
    torch.cuda.Stream of the test's own."""

    def __init__(self, caller_stream=False):
        import torch
        self.torch = torch
        if caller_stream:
            self._stream = torch.cuda.Stream()
            self.stream = self._stream.cuda_stream

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = self.torch.from_numpy(a.copy() if a.size else np.zeros(16, np.uint8)).to("cuda:0")
        return t, t.data_ptr()

    def get(self, h, dtype):
        return h.cpu().numpy().view(dtype)

    def sync(self):
        self.torch.cuda.synchronize()  # (buffers are made on torch's stream; the index launches on its own)
