"""Guard bands around the device-buffer API (fmx_locate_batch_async,
fmx_locate_jobs_async, fmx_locate_group_async, fmx_match_batch_async,
fmx_count_batch_async): the arena, the batches, the launch paths and the one
check that the emulator tests (test_guard_simt.py) and the GPU tests
(test_gpu_guard.py) share.

Every buffer of a call — inputs, outputs and workspace — is carved out of ONE
allocation filled with 0xA5, at least 4,096 guard bytes before and after it,
at exactly the size fmx.h asks for and at the weakest alignment it allows
(P-wide arrays P bytes past a 16-B boundary, uint32 arrays 4, uint64 arrays 8,
the workspace 16 B past a 256-B boundary, the pattern bytes at any skew), the
outputs prefilled with 0x5A.  After the launch and fmx_sync,
Arena.check_guards_and_inputs and Buffers.check_locate compare the whole arena
with what the contract of include/fmx.h allows it to be:
  * every guard byte still 0xA5, the input bytes and offsets unchanged;
  * d_loc_offsets (all n+1), *d_needed, counts, lens and ranges equal to the
    oracle's values;
  * d_locs[:min(cap, total)] the oracle's prefix in suffix-array-row order,
    d_locs[min(cap, total):cap] still 0x5A (nothing past the total, and — the
    buffer ends at cap — nothing past cap).
No correct or incorrect kernel of this engine strays further than a 16-B
vector, and d_locs is followed by guard bytes for every location past cap (an
emit that ignored cap would write them all), so nothing leaves the
allocation: a regression is a failed assert.
run_match also takes an explicit pattern list with its own parameters and
hints (tests/_long_cases.py: reads of mapper length, which tile is staged and
which is raw asserted from the offsets).
"""
import ctypes as C

import numpy as np

from _match_cases import ABSENT, Case
from _util import encode, rand_text

GUARD = 4096
FILL_GUARD, FILL_OUT = 0xA5, 0x5A
BATCH_SIZES = (1, 255, 256, 257, 700)
SKEWS = (0, 1, 7, 15)
# (P bytes, planes, vector bits, letters): u32 DNA (C2's shape), u64 with 128-bit vectors, and the 20
# residues + wildcard (sigma 21: multi-line walk records)
LAYOUTS = [(4, 3, 64, 4), (8, 3, 128, 4), (4, 5, 64, 20)]
LONG_M = 97  # symbols: past the 96 bits of a packed grouped record
# (P bytes, planes, vector bits, letters, load options): 0 and 1 for every layout, every derived structure
# (63, with FMX_DEEP_LUT_MB=1) for the first
INDEXES = [lay + (opt,) for lay in LAYOUTS for opt in (0, 1)] + [LAYOUTS[0] + (63,)]
CAP_NAMES = ("total", "total-1", "mid-run", "boundary", "one", "zero-null")  # caps_for()
# the batch shapes (GuardCase.batch) each launch path takes: ragged ones run in launch order, unfused, only
SHAPES = {"split": ("ragged", "single", "heavy"), "fused": ("single", "heavy"),
          "grouped": ("single", "heavy", "long"), "grouped-raw": ("single", "heavy", "long"),
          "chained": ("single", "heavy")}


def ids(p):
    return "-".join(str(x) for x in p) if isinstance(p, tuple) else str(p)


# ------------------------------------------------------------------ the arena

class HostMem:
    """The emulator: device pointers are host pointers, the arena is the array."""

    def __init__(self, nbytes):
        self._raw = np.empty(nbytes + 256, np.uint8)
        o = (-self._raw.ctypes.data) % 256
        self.mem = self._raw[o:o + nbytes]
        self.base = self.mem.ctypes.data

    def upload(self, host):
        self.mem[:] = host

    def download(self):
        return self.mem.copy()


class TorchMem:
    """The GPU: one uint8 tensor."""

    def __init__(self, nbytes):
        import torch
        self.torch = torch
        self.t = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        self.base = self.t.data_ptr()

    def upload(self, host):
        self.t.copy_(self.torch.from_numpy(host))
        self.torch.cuda.synchronize()  # (the index launches on its own stream)

    def download(self):
        self.torch.cuda.synchronize()
        return self.t.cpu().numpy()


class Arena:
    """carve() plans buffers, commit() builds the allocation; ptr() / view()
    then address a buffer in it, image() reads the whole allocation back."""

    def __init__(self, mem_cls):
        self.mem_cls = mem_cls
        self.cur = 0
        self.bufs = {}   # name -> (offset, nbytes)
        self.init = {}   # name -> initial bytes (an input) or None (an output: 0x5A, or the guard's 0xA5)
        self.fill = {}   # name -> what an output holds before the call (FILL_OUT unless carved otherwise)
        self.mem = None

    def carve(self, name, nbytes, align, skew, boundary=16, data=None, tail=0, fill=FILL_OUT):
        """A buffer of exactly nbytes at (a `boundary`-byte boundary) + skew,
        GUARD bytes or more after the previous one, and `tail` more guard
        bytes after it than the next carve's GUARD.  fill: what an output
        (data None) holds before the call — FILL_GUARD makes it look like the
        guards around it (a blob area that must not be assumed zero)."""
        assert skew % align == 0 and skew < boundary and name not in self.bufs
        off = -(-(self.cur + GUARD) // boundary) * boundary + skew
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert data.size == nbytes
        self.bufs[name] = (off, nbytes)
        self.init[name] = data
        self.fill[name] = fill
        self.cur = off + nbytes + tail
        return name

    def commit(self):
        self.size = self.cur + GUARD
        host = np.full(self.size, FILL_GUARD, np.uint8)
        self.is_guard = np.ones(self.size, bool)
        for name, (off, nb) in self.bufs.items():
            host[off:off + nb] = self.fill[name] if self.init[name] is None else self.init[name]
            self.is_guard[off:off + nb] = False
        self.mem = self.mem_cls(self.size)
        assert self.mem.base % 256 == 0
        self.mem.upload(host)
        self.host0 = host

    def ptr(self, name):
        return self.mem.base + self.bufs[name][0] if name in self.bufs else 0

    def image(self):
        self.img = self.mem.download()
        return self.img

    def view(self, name, dtype=np.uint8):
        off, nb = self.bufs[name]
        return self.img[off:off + nb].view(dtype)

    def check_guards_and_inputs(self, what):
        bad = np.flatnonzero(self.is_guard & (self.img != FILL_GUARD))
        if bad.size:
            at = int(bad[0])
            near = min(self.bufs.items(), key=lambda kv: min(abs(at - kv[1][0]), abs(at - kv[1][0] - kv[1][1])))
            rel = at - near[1][0]
            raise AssertionError(f"{what}: {bad.size} guard bytes written, first at {rel} bytes from the start of "
                                 f"{near[0]} ({near[1][1]} bytes long)")
        for name, data in self.init.items():
            if data is not None:
                assert np.array_equal(self.view(name), data), f"{what}: input {name} changed"


# ---------------------------------------------------------------- the batches

class GuardCase(Case):
    """One text of n_text symbols over `nchars` letters plus a wildcard symbol
    that does not occur in it (_match_cases.Case: its expected() gives the
    match values), and the batches of the three shapes emit_locations treats
    differently."""

    def __init__(self, seed, nchars, n_text=3000, k=3, sr=2):
        super().__init__(seed, nchars, k=k, sr=sr)
        self.text = rand_text(np.random.default_rng(seed + 7), self.chars, n_text, n_text)
        self.enc = encode(self.table, self.text)
        self.short = 1 if nchars > 8 else 2  # the fixed length whose patterns occur hundreds of times
        self._batches, self._want = {}, {}

    def _sub(self, rng, m):
        s = int(rng.integers(0, len(self.text) - m))
        return self.text[s:s + m]

    def _unique(self, rng, orc, m, count):
        """`count` substrings of m symbols that occur exactly once."""
        out = []
        while len(out) < count:
            p = self._sub(rng, m)
            if orc.count(p) == 1:
                out.append(p)
        return out

    def _absent(self, rng, orc, m):
        """m symbols of the alphabet that do not occur together (m >= 4), or a
        pattern holding the wildcard byte."""
        for _ in range(50):
            p = bytes(rng.choice(np.frombuffer(self.chars, np.uint8), size=m))
            if orc.count(p) == 0:
                return p
        p = bytearray(self._sub(rng, m))
        p[int(rng.integers(0, m))] = ABSENT
        return bytes(p)

    def batch(self, orc, shape, n):
        """shape "single": n 12-mers, exactly one occurrence each (the last few
        of a batch past a wave absent instead); "heavy": n patterns of
        self.short symbols, hundreds of occurrences each next to absent ones;
        "ragged": runs of 64+ single-occurrence 12-mers between 1- to 6-mers
        (hundreds of occurrences down to a handful) and absent patterns;
        "long": LONG_M-mers, one occurrence or none; "mid": 5-mers (a few
        occurrences each: what a derived index settles by a row scan)."""
        key = (shape, n)
        if key in self._batches:
            return self._batches[key]
        rng = np.random.default_rng(self.seed * 1000 + n + len(shape))
        if shape == "single":
            pats = self._unique(rng, orc, 12, n)
            for j in range(n - min(n, 3), n if n > 64 else 0):
                pats[j] = self._absent(rng, orc, 12)
        elif shape == "long":
            pats = self._unique(rng, orc, LONG_M, n)
            for j in range(1, n, 5):
                pats[j] = self._absent(rng, orc, LONG_M)
        elif shape == "mid":
            pats = [self._sub(rng, 5) for _ in range(n)]
            for j in range(4, n, 9):
                pats[j] = self._absent(rng, orc, 5)
        elif shape == "heavy":
            pats = [self._sub(rng, self.short) for _ in range(n)]
            for j in range(2, n, 7):  # absent ones in between
                p = bytearray(pats[j])
                p[j % self.short] = ABSENT
                pats[j] = bytes(p)
        else:
            assert shape == "ragged"
            pats = []
            while len(pats) < n:
                pats += self._unique(rng, orc, 12, 70)
                pats += [self._sub(rng, 1), self._absent(rng, orc, 2), self._sub(rng, 2)]
                for _ in range(60):
                    m = int(rng.choice([1, 2, 3, 3, 3, 4, 5, 5, 6, 6]))
                    if m <= 2 and rng.integers(0, 4):  # (few of the heaviest: the emulator walks every row)
                        m = 3
                    pats.append(self._sub(rng, m))
                    if rng.integers(0, 5) == 0:
                        pats.append(self._absent(rng, orc, int(rng.integers(1, 13))))
            if n < 64:
                pats = [self._sub(rng, 1)] if n == 1 else pats[70:70 + n]
            pats = pats[:n]
        assert len(pats) == n and all(len(p) for p in pats)
        self._batches[key] = pats
        return pats

    def want_locate(self, pkg, orc, shape, n):
        """(patterns, oracle offsets uint64[n+1], oracle locations), cached."""
        key = (shape, n)
        if key not in self._want:
            pats = self.batch(orc, shape, n)
            data, offsets = pkg.pack_patterns(pats)
            off, locs = orc.locate_batch(data, offsets)
            off, locs = off.astype(np.uint64), locs.astype(np.uint64)
            cnt = np.diff(off.astype(np.int64))
            if shape in ("single", "ragged") and n >= 255:
                run = best = 0
                for c in cnt:
                    run = run + 1 if c == 1 else 0
                    best = max(best, run)
                assert best >= 64, "no run of 64 single-occurrence patterns"
            if shape in ("heavy", "ragged"):
                assert cnt.max() >= 100 and (n == 1 or (cnt == 0).any()), "no heavy pattern next to an absent one"
            off.setflags(write=False)
            locs.setflags(write=False)
            self._want[key] = (pats, off, locs)
        return self._want[key]


_CASES = {}


def case_for(nchars):
    if nchars not in _CASES:
        _CASES[nchars] = GuardCase(400 + nchars, nchars)
    return _CASES[nchars]


def caps_for(off):
    """The caps of a batch with oracle offsets `off`, by name: total, total-1,
    one inside a heavy pattern's run and not on a multiple of 64 from its
    start (mid-wave), one exactly on a pattern boundary, 1, and 0 with d_locs
    = NULL.  Names whose cap does not exist for the batch are left out."""
    total = int(off[-1])
    cnt = np.diff(off.astype(np.int64))
    caps = {"total": total}
    if total >= 1:
        caps["total-1"] = total - 1
    j = int(np.argmax(cnt))
    if cnt[j] >= 100:
        cap = int(off[j]) + int(cnt[j]) // 2 + 1
        while (cap - int(off[j])) % 64 == 0 or cap % 64 == 0:
            cap += 1
        assert off[j] < cap < off[j + 1] and (cap - int(off[j])) % 64 and cap % 64, "cap not mid-run, mid-wave"
        caps["mid-run"] = cap
    inner = [int(x) for x in off[1:-1] if 1 < x < total - 1]
    if inner:
        caps["boundary"] = inner[len(inner) // 2]
        assert caps["boundary"] in off.tolist()
    if total > 1:
        caps["one"] = 1
    caps["zero-null"] = 0
    return caps


# ------------------------------------------------------------ paths and calls

# name -> (environment at load, fixed-length batches only, the fmx_index_info counter its launches raise)
PATHS = {
    "split":       (dict(FMX_FUSED="0", FMX_GROUPED="0", FMX_EMIT_CHAIN="0"), False, "launches_ordered"),
    "fused":       (dict(FMX_FUSED="1", FMX_GROUPED="0", FMX_EMIT_CHAIN="0"), True, "launches_fused"),
    "grouped":     (dict(FMX_FUSED="0", FMX_GROUPED="1", FMX_GROUPED_RAW="0", FMX_EMIT_CHAIN="0"), True,
                    "launches_grouped"),
    "grouped-raw": (dict(FMX_FUSED="0", FMX_GROUPED="1", FMX_GROUPED_RAW="1", FMX_EMIT_CHAIN="0"), True,
                    "launches_grouped_raw"),
    "chained":     (dict(FMX_FUSED="0", FMX_GROUPED="1", FMX_GROUPED_RAW="0", FMX_EMIT_CHAIN="1"), True,
                    "launches_chained"),
}
COUNTERS = ("launches_grouped", "launches_grouped_raw", "launches_ordered", "launches_fused", "launches_chained")
ENV_KEYS = ("FMX_FUSED", "FMX_GROUPED", "FMX_GROUPED_RAW", "FMX_EMIT_CHAIN", "FMX_GROUP_CHECK", "FMX_GROUPED_MIN",
            "FMX_FUSED_MAX_TILES", "FMX_EMIT_FOLD")


def open_index(pkg, O, monkeypatch, case, pb, planes, vb, options, path):
    """The index under the path's environment (read once, at load), and the oracle."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FMX_DEEP_LUT_MB", "1")
    blob = case.blob(O, pb, planes, vb)
    orc = O.OracleIndex(blob, O.layout(pb, planes, vb, 0))
    block = getattr(pkg.blocks, f"Block{planes}")(pkg.Vector(vb))
    ix = pkg.FmIndex.load(blob, pkg.u32 if pb == 4 else pkg.u64, block, options=options)
    return ix, orc


# (path, index): a grouped launch needs the faithful index, so with derived structures the launch-order paths only
LOCATE_PARAMS = [(path,) + ixp for path in PATHS for ixp in INDEXES if ixp[4] != 63 or path in ("split", "fused")]


def shapes_for(path, opt):
    """... plus fixed 5-mers on a derived index: what its row scan settles."""
    return SHAPES[path] + (("mid",) if opt == 63 else ())


def assert_scan_live(ix, case, orc, path):
    """Load options 63: the kHitMask branch of emit_locations is live — at
    least one pattern of the batches below is settled by a row-record scan."""
    info = ix.info()
    assert info["options"] == 63 and info["scan_rows"] >= 2 and info["deep_lut_k"] > case.k + 1
    for shape in ("mid",) + (("ragged",) if path == "split" else ()):
        assert scan_settled(case, orc, info, case.batch(orc, shape, 700)), "no interval settled by a scan"


def counters(ix):
    i = ix.info()
    return {k: i[k] for k in COUNTERS}


def expect_counters(ix, before, path, launches=1):
    """Exactly `launches` launches since `before`, all on `path`."""
    now = counters(ix)
    d = {k: now[k] - before[k] for k in COUNTERS}
    want = dict.fromkeys(COUNTERS, 0)
    if path in ("split", "fused"):
        want["launches_ordered"] = launches
        want["launches_fused"] = launches if path == "fused" else 0
    elif path == "grouped-raw":
        want["launches_grouped_raw"] = launches
    else:
        want["launches_grouped"] = launches
        want["launches_chained"] = launches if path == "chained" else 0
    assert d == want, f"{path}: launches took {d}, expected {want}"


def fixed_len_of(pats):
    m = len(pats[0])
    return m if all(len(p) == m for p in pats) else 0


def stage_kb_of(pats):
    most = max(sum(len(p) for p in pats[t:t + 256]) for t in range(0, len(pats), 256))
    return max(1, -(-most // 1024))


class Buffers:
    """One batch's buffers in an arena (names prefixed for group calls)."""

    def __init__(self, arena, pkg, ix, pats, pb, skew, reversed, cap, prefix="", counts=True, locs=True, lens=False,
                 ranges=False, workspace=True, total=0):
        q = [p[::-1] for p in pats] if reversed else pats
        self.data, self.offsets = pkg.pack_patterns(q)
        self.n, self.pb, self.cap, self.pre, self.arena = len(pats), pb, cap, prefix, arena
        n, c = self.n, arena.carve
        self.P = np.uint32 if pb == 4 else np.uint64
        if workspace:
            self.ws_bytes = ix.locate_workspace_size(n)
            c(prefix + "ws", self.ws_bytes, 16, 16, boundary=256)
        c(prefix + "offsets", 8 * (n + 1), 8, 8, data=self.offsets)
        if locs:
            c(prefix + "loc_offsets", 8 * (n + 1), 8, 8)
            c(prefix + "needed", 8, 8, 8)
            if cap:
                # guard bytes for every location past cap: an emit that ignored cap stays inside the arena
                c(prefix + "locs", pb * cap, pb, pb, tail=pb * max(total - cap, 0))
        if counts:
            c(prefix + "counts", pb * n, pb, pb)
        if lens:
            c(prefix + "lens", 4 * n, 4, 4)
        if ranges:
            c(prefix + "ranges", 2 * pb * n, pb, pb)
        # the pattern bytes last: the final byte of the arena's last batch lies flush against the end guard
        c(prefix + "bytes", self.data.size, 1, skew, data=self.data)

    def p(self, name):
        return self.arena.ptr(self.pre + name)

    def v(self, name, dtype):
        return self.arena.view(self.pre + name, dtype)

    def check_locate(self, what, off, locs, counts=True):
        """The contract of a locate-shaped output against oracle offsets / locations."""
        total = int(off[-1])
        assert np.array_equal(self.v("loc_offsets", np.uint64), off), f"{what}: d_loc_offsets"
        assert int(self.v("needed", np.uint64)[0]) == total, f"{what}: *d_needed"
        if counts:
            assert np.array_equal(self.v("counts", self.P).astype(np.uint64), np.diff(off)), f"{what}: d_counts"
        if self.cap:
            got = self.v("locs", self.P)
            k = min(self.cap, total)
            assert np.array_equal(got[:k].astype(np.uint64), locs[:k]), f"{what}: d_locs[:min(cap, total)]"
            rest = self.v("locs", np.uint8)[k * self.pb:]
            assert (rest == FILL_OUT).all(), f"{what}: d_locs written past min(cap, total)"


def flush_against_guard(arena, bufs):
    off, nb = arena.bufs[bufs.pre + "bytes"]
    assert off + nb == arena.size - GUARD, "the last pattern byte is not the byte before the end guard"


def run_locate(pkg, ix, mem_cls, case, orc, pb, path, shape, n, cap_name, skew, reversed, via_jobs=False):
    """One fmx_locate_batch_async (or, via_jobs, fmx_locate_jobs_async) call
    on `path` and the whole check.  Returns False when the batch has no cap of
    that name."""
    pats, off, locs = case.want_locate(pkg, orc, shape, n)
    caps = caps_for(off)
    if cap_name not in caps:
        return False
    cap = caps[cap_name]
    what = f"{path} {shape} n={n} cap={cap_name}({cap}) skew={skew} rev={reversed}"
    arena = Arena(mem_cls)
    b = Buffers(arena, pkg, ix, pats, pb, skew, reversed, cap, total=int(off[-1]))
    arena.commit()
    flush_against_guard(arena, b)
    assert b.p("bytes") % 16 == skew and b.p("ws") % 256 == 16 and b.p("offsets") % 16 == 8
    m = 0 if shape == "ragged" else fixed_len_of(pats)  # (every other shape is a fixed-length batch: the hint set)
    assert m or not PATHS[path][1]
    before = counters(ix)
    args = (b.p("bytes"), b.p("offsets"), n, b.p("loc_offsets"), b.p("locs"), cap, b.p("needed"), b.p("ws"), b.ws_bytes)
    kw = dict(d_counts=b.p("counts"), reversed=reversed, stage_kb=stage_kb_of(pats), fixed_len=m)
    if via_jobs:
        ix.locate_jobs_async(ix.job_queue([ix.locate_job(*args, **kw)]))
    else:
        ix.locate_batch_async(*args, **kw)
    ix.sync()
    # (patterns too long for a packed record: id-only records whatever FMX_GROUPED_RAW says)
    expect_counters(ix, before, "grouped-raw" if shape == "long" and path == "grouped" else path)
    arena.image()
    arena.check_guards_and_inputs(what)
    b.check_locate(what, off, locs)
    return True


def run_group(pkg, ix, mem_cls, case, orc, pb, path, skew, reversed):
    """fmx_locate_group_async: five fixed-length batches of 1, 255, 256, 257
    and 700 patterns in one call and one arena, each with its own cap (one a
    pattern short of its total, one 0 with d_locs = NULL, the rest exact) and
    its own workspace."""
    arena = Arena(mem_cls)
    plan = []
    for j, n in enumerate(BATCH_SIZES):
        shape = "heavy" if j % 2 else "single"
        pats, off, locs = case.want_locate(pkg, orc, shape, n)
        total = int(off[-1])
        cap = {1: total - 1, 3: 0}.get(j, total)
        b = Buffers(arena, pkg, ix, pats, pb, (skew + 5 * j) % 16 if j else skew, reversed != (j == 2), cap,
                    prefix=f"b{j}.", total=total)
        plan.append((b, pats, off, locs, reversed != (j == 2)))
    arena.commit()
    flush_against_guard(arena, plan[-1][0])
    jobs = [ix.locate_job(b.p("bytes"), b.p("offsets"), b.n, b.p("loc_offsets"), b.p("locs"), b.cap, b.p("needed"),
                          b.p("ws"), b.ws_bytes, d_counts=b.p("counts"), reversed=rev, stage_kb=stage_kb_of(pats),
                          fixed_len=fixed_len_of(pats)) for b, pats, _, _, rev in plan]
    before = counters(ix)
    ix.locate_group_async(ix.job_queue(jobs))
    ix.sync()
    expect_counters(ix, before, path)
    arena.image()
    what = f"group {path} skew={skew} rev={reversed}"
    arena.check_guards_and_inputs(what)
    for j, (b, _, off, locs, _) in enumerate(plan):
        b.check_locate(f"{what} batch {j}", off, locs)


MATCH_MIN_LEN, MATCH_MAX_OCC = 2, 200


def match_batch(case, orc, n):
    """The ragged batch plus what only a match accepts: an empty pattern, and
    12-mers with one wrong symbol (a proper suffix matches)."""
    pats = list(case.batch(orc, "ragged", n))
    rng = np.random.default_rng(n)
    for j in range(3, n, 9):
        if len(pats[j]) == 12:
            q = bytearray(pats[j])
            at = int(rng.integers(0, 9))
            q[at] = case.other(rng, q[at])
            pats[j] = bytes(q)
    if n > 10:
        pats[7] = b""
    return pats


def run_match(pkg, ix, mem_cls, case, orc, pb, n, cap_name, skew, reversed, locate=True, pats=None, params=None,
              stage_kb=None, fixed_len=0, long_patterns=False, tiles=None):
    """fmx_match_batch_async, with locations (min_len / max_occ keep the
    shortest and the heaviest matches from reporting) or lengths and intervals
    only (no location buffers, no workspace).
    pats: the patterns (n of them) in place of match_batch(case, orc, n),
    whose class check is then the caller's; params: (min_len, max_occ) in place
    of the module's; stage_kb: FMX_HINT_STAGE_KB (None: what stages every tile;
    0: no hint), fixed_len, long_patterns: the other hints; tiles: the caller's
    list of staged (True) and raw tiles, asserted against
    _strand_cases.staged_tiles()."""
    own = pats is None
    pats = match_batch(case, orc, n) if own else pats
    assert len(pats) == n
    min_len, max_occ = params or (MATCH_MIN_LEN, MATCH_MAX_OCC)
    if stage_kb is None:
        stage_kb = stage_kb_of(pats)
    if tiles is not None:
        from _strand_cases import staged_tiles  # (it imports this module)
        got = staged_tiles(pats, "forward", stage_kb, fixed_len, long_patterns)
        assert got == list(tiles), f"tiles staged by their offsets: {got}, expected {list(tiles)}"
    hints = dict(stage_kb=stage_kb, fixed_len=fixed_len, long_patterns=long_patterns)
    exp = [case.expected(orc, p) for p in pats]
    rep = [e[0] >= min_len and e[2] - e[1] <= max_occ for e in exp]
    cnt = np.array([e[2] - e[1] if r else 0 for e, r in zip(exp, rep)], np.uint64)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
    locs = np.array([x for e, r in zip(exp, rep) if r for x in e[3]], np.uint64)
    if own and n >= 255:
        assert sum(rep) >= 64 and sum(not r and e[0] > 0 for e, r in zip(exp, rep)) >= 4, "every pattern reports"
    cap = 0
    if locate:
        caps = caps_for(off)
        if cap_name not in caps:
            return False
        cap = caps[cap_name]
    what = f"match n={n} cap={cap_name}({cap}) skew={skew} rev={reversed} locate={locate}"
    arena = Arena(mem_cls)
    b = Buffers(arena, pkg, ix, pats, pb, skew, reversed, cap, counts=False, locs=locate, lens=True, ranges=True,
                workspace=locate, total=int(off[-1]))
    arena.commit()
    flush_against_guard(arena, b)
    assert b.p("lens") % 16 == 4 and b.p("ranges") % 16 == pb % 16
    if locate:
        ix.match_batch_async(b.p("bytes"), b.p("offsets"), n, b.p("lens"), b.p("ranges"), b.p("loc_offsets"),
                             b.p("locs"), cap, b.p("needed"), b.p("ws"), b.ws_bytes, min_len=min_len,
                             max_occ=max_occ, reversed=reversed, **hints)
    else:
        ix.match_batch_async(b.p("bytes"), b.p("offsets"), n, b.p("lens"), b.p("ranges"), min_len=min_len,
                             max_occ=max_occ, reversed=reversed, **hints)
    ix.sync()
    arena.image()
    arena.check_guards_and_inputs(what)
    assert b.v("lens", np.uint32).tolist() == [e[0] for e in exp], f"{what}: d_lens"
    assert b.v("ranges", b.P).reshape(n, 2).tolist() == [[e[1], e[2]] for e in exp], f"{what}: d_ranges"
    if locate:
        b.check_locate(what, off, locs, counts=False)
    return True


def run_count(pkg, ix, mem_cls, case, orc, pb, shape, n, skew, reversed, fixed):
    """fmx_count_batch_async."""
    pats, off, _ = case.want_locate(pkg, orc, shape, n)
    what = f"count {shape} n={n} skew={skew} rev={reversed}"
    arena = Arena(mem_cls)
    b = Buffers(arena, pkg, ix, pats, pb, skew, reversed, 0, locs=False, workspace=False)
    arena.commit()
    flush_against_guard(arena, b)
    assert b.p("counts") % 16 == pb % 16
    ix.count_batch_async(b.p("bytes"), b.p("offsets"), n, b.p("counts"), reversed=reversed,
                         stage_kb=stage_kb_of(pats), fixed_len=fixed_len_of(pats) if fixed else 0)
    ix.sync()
    arena.image()
    arena.check_guards_and_inputs(what)
    assert np.array_equal(b.v("counts", b.P).astype(np.uint64), np.diff(off)), f"{what}: d_counts"


def scan_settled(case, orc, info, pats):
    """Patterns whose interval a derived index settles by a row-record scan
    with two or more rows left (kHitMask in emit_locations): shorter than the
    deep table's K (seeded from the blob's k-mer table), longer than k (LF
    steps remain), the suffix one symbol shorter within scan_rows rows, and
    two or more occurrences."""
    return [p for p in pats if case.k < len(p) < info["deep_lut_k"] and orc.count(p) >= 2
            and orc.count(p[1:]) <= info["scan_rows"]]


# -------------------------------------------------------- host-buffer calls

def heavy_host_batch(case, orc, pkg, n=700):
    """n single symbols: more locations than the text has rows, and more than
    a fresh index's first scratch buffer holds (the retry pass grows it)."""
    rng = np.random.default_rng(5)
    pats = [bytes([int(rng.choice(np.frombuffer(case.chars, np.uint8)))]) for _ in range(n)]
    pats[3] = bytes([ABSENT])
    data, offsets = pkg.pack_patterns(pats)
    off, locs = orc.locate_batch(data, offsets)
    return pats, data, offsets, off.astype(np.uint64), locs


def check_host_capacity(pkg, ix, case, orc, pb, match=False):
    """fmx_locate_batch / fmx_match_batch on host buffers: cap = total - 1
    and cap = 0 return FMX_E_CAPACITY with *needed = total, the offsets (the
    match: lengths and intervals too) fully written and the caller's out_locs
    byte-identical to its prefill, canary bytes after it included; cap =
    total then succeeds on the same index through the two-pass path (the
    device output buffer regrown to the total: two launches)."""
    n_ = pkg._native
    lib = n_.lib()
    pats, data, offsets, off, locs = heavy_host_batch(case, orc, pkg)
    n, total = len(pats), int(off[-1])
    P = np.uint32 if pb == 4 else np.uint64
    assert total > n and total > len(case.text), "the batch does not overflow the first output guess"
    exp = [case.expected(orc, p) for p in pats] if match else None
    CANARY = 64
    for cap in (total - 1, 0, total):
        raw = np.full(pb * max(cap, 1) + CANARY, FILL_OUT, np.uint8)  # (cap = 0: a non-null pointer all the same)
        loff = np.full(n + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
        lens, rng = np.full(n, 0x5A5A5A5A, np.uint32), np.full((n, 2), 0x5A, P)
        needed = C.c_uint64(12345)
        before = counters(ix)
        if match:
            st = lib.fmx_match_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, (1 << 64) - 1,
                                     lens.ctypes.data, rng.ctypes.data, loff.ctypes.data, raw.ctypes.data, cap,
                                     C.byref(needed))
        else:
            st = lib.fmx_locate_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, loff.ctypes.data,
                                      raw.ctypes.data, cap, C.byref(needed))
        launches = counters(ix)["launches_ordered"] - before["launches_ordered"]
        what = f"{'match' if match else 'locate'} host cap={cap} of {total}"
        assert needed.value == total, f"{what}: *needed"
        assert np.array_equal(loff, off), f"{what}: out_loc_offsets"
        if match:
            assert lens.tolist() == [e[0] for e in exp] and rng.tolist() == [[e[1], e[2]] for e in exp], what
        if cap < total:
            assert st == n_.FMX_E_CAPACITY, f"{what}: status {st}"
            assert (raw == FILL_OUT).all(), f"{what}: out_locs written on FMX_E_CAPACITY"
        else:
            assert st == 0, f"{what}: status {st}"
            assert np.array_equal(raw[:pb * total].view(P), locs.astype(P)), f"{what}: out_locs"
            assert (raw[pb * total:] == FILL_OUT).all(), f"{what}: bytes past out_locs[cap] written"
            if not match:
                assert launches == 2, f"{what}: {launches} launches, not the two-pass path"
