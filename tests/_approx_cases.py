"""k-mismatch search (fmx_approx_batch): the cases, their bodies and the
expected values the emulator tests (test_approx_simt.py) and the GPU tests
(test_gpu_approx.py) share.  A body takes what differs between the two: the
batch size, the layouts to visit, the device memory (_util.HostDev / TorchDev).

The reference is brute force, not a search: a pattern of length m is compared
with every length-m window of the encoded text in numpy; the distinct windows
with at most max_mm differences are its variants (the text holds no wildcard
symbol, so a pattern byte that maps to it always differs), sorted by the closed
form of include/fmx.h: d ascending, then, position by position from m-1 down to
0, a substituted symbol (by symbol index) before the pattern's own.  For each
variant, lo is the bisection of the plainly sorted suffix list (as
_match_cases.Case.expected), hi - lo is OracleIndex.count and the locations are
OracleIndex.locate, asserted equal to sa[lo:hi] on the reference alone.

A batch is cut from one pool per (text, max_mm, longest pattern): substrings of
length 1, 2, k, k+1, 4, 8, 12, 20 and 24 with 0..max_mm+1 substitutions planted
at the last symbol, inside the last k, at position 0, as an adjacent pair and
at random; text[:m] with a substitution (the text start and the sentinel); an
ABSENT byte at the last, a middle and the first position (a forced
substitution); an empty pattern in mid-batch; max_mm+1 ABSENT bytes (no hit); a
pattern longer than the text; then substrings of 4..12 symbols with 0..2
substitutions up to n.
"""
import bisect
import ctypes as C
from math import comb as _comb

import numpy as np
import pytest

from _match_cases import ABSENT, Case  # noqa: F401
from _util import block_of, case_for, encode, open_index, pos_of  # noqa: F401

BATCH_SIZES = (1, 255, 256, 257, 700)
_VAR = {}
_POOLS = {}


def variants(case, orc, p, max_mm):
    """The variants of pattern p (bytes, logical order) in contract order:
    [(d, [(pos, sym), ...] by decreasing pos, lo, hi, locations, variant bytes)]."""
    key = (id(case), p, max_mm)
    got = _VAR.get(key)
    if got is not None:
        return got
    T = np.frombuffer(case.enc, np.uint8)
    m, out = len(p), []
    if 0 < m <= T.size:
        e = np.frombuffer(encode(case.table, p), np.uint8)
        win = np.lib.stride_tricks.sliding_window_view(T, m)
        keep = win[(win != e).sum(axis=1) <= max_mm]
        rows = np.unique(keep, axis=0) if keep.size else keep
        sa, suf = case.suffixes()
        keyed = []
        for v in rows:
            diff = v != e
            # the order's key: d, then from the last position down the substituted symbol, or sigma for the own one
            rank = np.where(diff, v, case.sigma)[::-1]
            keyed.append((int(diff.sum()), tuple(int(x) for x in rank), v))
        keyed.sort(key=lambda x: x[:2])
        for d, _, v in keyed:
            subs = [(int(q), int(v[q])) for q in range(m - 1, -1, -1) if v[q] != e[q]]
            vb = bytes(case.chars[int(c)] for c in v)
            cnt, locs = orc.count(vb), orc.locate(vb)
            lo = bisect.bisect_left(suf, bytes(v))
            assert cnt > 0 and len(locs) == cnt and locs == sa[lo:lo + cnt], "oracle row order != plain suffix order"
            out.append((d, subs, lo, lo + cnt, locs, vb))
    _VAR[key] = out
    return out


def pool(case, max_mm, max_len):
    key = (id(case), max_mm, max_len)
    got = _POOLS.get(key)
    if got is not None:
        return got
    rng = np.random.default_rng(case.seed + 77 * max_mm + max_len)
    t, k, n = case.text, case.k, len(case.text)

    def sub(m):
        s = int(rng.integers(0, n - m))
        return t[s:s + m]

    def plant(p, where):
        q = bytearray(p)
        for j in where:
            q[j] = case.other(rng, q[j])
        return bytes(q)
    pats = []
    for m in sorted({1, 2, k, k + 1, 4, 8, 12, 20, 24}):
        if m > max_len:
            continue
        pats += [sub(m), sub(m)]
        pats.append(plant(sub(m), [m - 1]))                             # the last symbol
        pats.append(plant(sub(m), [m - 1 - int(rng.integers(0, min(k, m)))]))  # inside the last k
        pats.append(plant(sub(m), [0]))                                 # position 0
        if m >= 2:
            j = int(rng.integers(0, m - 1))
            pats.append(plant(sub(m), [j, j + 1]))                      # an adjacent pair
        for nsub in range(1, max_mm + 2):                               # 1..max_mm+1 at random
            if nsub <= m:
                pats.append(plant(sub(m), rng.choice(m, size=nsub, replace=False).tolist()))
        pats.append(plant(t[:m], [int(rng.integers(0, m))]))            # the text start (the sentinel)
        for j in sorted({m - 1, m // 2, 0}):                            # a forced substitution
            q = bytearray(sub(m))
            q[j] = ABSENT
            pats.append(bytes(q))
    pats.insert(len(pats) // 2, b"")                                    # an empty pattern in mid-batch
    pats.append(bytes([ABSENT]) * (max_mm + 1))                         # no hit
    pats.append(t + t[:1])                                              # longer than the text
    assert len(pats) < 255, len(pats)
    # the fill, three kinds in turn (the third twice), chosen by what the text is (its length and alphabet), not by any
    # answer: 12 symbols with max_mm + 1 substitutions (mostly no hit), 12 symbols with 0..max_mm (mostly
    # the one), and a length at which a string's neighbourhood is expected in the text a few times
    s_ = len(case.chars)
    few = 3
    while few < min(12, max_len):
        nb = sum(_comb(few, d) * (s_ - 1) ** d for d in range(max_mm + 1))
        if n * nb <= 3 * s_ ** few:
            break
        few += 1
    fill = []
    for x in range(700):
        kind = (0, 1, 2, 2)[x % 4]
        m = min(12, max_len) if kind < 2 else few
        nsub = max_mm + 1 if kind == 0 else int(rng.integers(0, max_mm + 1)) if kind == 1 else int(rng.integers(0, 2))
        fill.append(plant(sub(m), rng.choice(m, size=min(m, nsub), replace=False).tolist()))
    got = _POOLS[key] = (pats, fill)
    return got


def batch(case, n, max_mm=1, max_len=24):
    core, fill = pool(case, max_mm, max_len)
    if n == 1:
        return [core[8]]
    return (core + fill)[:n]


def select(case, orc, p, max_mm, max_hits, best):
    """(the stored hits, more) of pattern p."""
    v = variants(case, orc, p, max_mm)
    if best and v:
        v = [x for x in v if x[0] == v[0][0]]
    return v[:max_hits], int(len(v) > max_hits)


def assert_classes(case, orc, pats, max_mm, max_hits, best=False):
    """What a sweep of >= 256 patterns must hold, on the expected values alone."""
    hits = [select(case, orc, p, max_mm, 1 << 30, best)[0] for p in pats]
    nh = np.array([len(h) for h in hits])
    got = {"0": int((nh == 0).sum()), "1": int((nh == 1).sum()), "2..8": int(((nh >= 2) & (nh <= 8)).sum())}
    strata = {x[0] for h in hits for x in h[:max_hits]}
    assert all(v >= 30 for v in got.values()), f"case classes missing from the batch: {got}"
    assert strata == set(range(max_mm + 1)), f"strata stored: {strata}"
    assert (nh > max_hits).any(), "no truncated pattern"


def expected_arrays(case, orc, pats, max_mm, max_hits, best, max_occ):
    """nhits, more, mm, subs, ranges, loc_offsets, locations."""
    n, mh = len(pats), max_hits
    nh, more = np.zeros(n, np.int64), np.zeros(n, np.int64)
    mm, subs, rng = np.zeros((n, mh), np.int64), np.zeros((n, mh, 3, 2), np.int64), np.zeros((n, mh, 2), np.int64)
    cnt, locs = np.zeros(n * mh, np.uint64), []
    for i, p in enumerate(pats):
        hits, more[i] = select(case, orc, p, max_mm, mh, best)
        nh[i] = len(hits)
        for j, (d, sb, lo, hi, ll, _) in enumerate(hits):
            mm[i, j] = d
            for t, ps in enumerate(sb):
                subs[i, j, t] = ps
            rng[i, j] = (lo, hi)
            if max_occ is None or hi - lo <= max_occ:
                cnt[i * mh + j] = hi - lo
                locs += ll
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
    return nh, more, mm, subs, rng, off, np.array(locs, dtype=np.uint64)


NAMES = ("nhits", "more", "mm", "subs", "ranges")


def compare(got, exp, locate=True):
    for name, g, e in zip(NAMES, got, exp):
        g = np.asarray(g)
        assert g.shape == e.shape, (name, g.shape, e.shape)
        bad = np.argwhere(g.astype(np.int64) != e)
        assert bad.size == 0, f"{name} differ at {len(bad)} places, first {bad[:4].tolist()}: " \
                              f"{[int(g[tuple(b)]) for b in bad[:4]]} expected {[int(e[tuple(b)]) for b in bad[:4]]}"
    if not locate:
        assert len(got) == 5
        return
    assert len(got) == 7
    assert np.array_equal(np.asarray(got[5]).astype(np.uint64), exp[5]), "location offsets differ"
    assert np.array_equal(np.asarray(got[6]).astype(np.uint64), exp[6]), "locations differ (SA-row order)"


def check_approx(ix, orc, case, pats, max_mm=1, max_hits=8, best=False, max_occ=None, reversed=False, locate=True):
    """approx_batch of `pats` against the expected values; returns (expected, got)."""
    exp = expected_arrays(case, orc, pats, max_mm, max_hits, best, max_occ)
    q = [p[::-1] for p in pats] if reversed else pats
    got = ix.approx_batch(q, max_mm=max_mm, max_hits=max_hits, best=best, max_occ=max_occ, reversed=reversed,
                          locate=locate)
    assert all(got[j].dtype == np.uint32 for j in range(4))
    compare(got, exp, locate)
    return exp, got


def cross_check(ix, case, pats, got):
    """Against the shipped calls on the same index: every stored variant, re-
    encoded to bytes, has match_batch's interval (a whole match) and
    locate_batch's locations."""
    nh, more, mm, subs, rng, loff, locs = got
    mh = mm.shape[1]
    vs, where = [], []
    for i, p in enumerate(pats):
        e = bytearray(encode(case.table, p))
        for j in range(int(nh[i])):
            v = bytearray(e)
            for t in range(int(mm[i, j])):
                v[int(subs[i, j, t, 0])] = int(subs[i, j, t, 1])
            vs.append(bytes(case.chars[c] for c in v))
            where.append((i, j))
    assert len(vs) >= 200
    lens, mrng = ix.match_batch(vs, locate=False)
    woff, wlocs = ix.locate_batch(vs)
    for x, (i, j) in enumerate(where):
        assert int(lens[x]) == len(pats[i]) and np.array_equal(mrng[x], rng[i, j]), (i, j)
        a, b = int(loff[i * mh + j]), int(loff[i * mh + j + 1])
        assert np.array_equal(locs[a:b], wlocs[int(woff[x]):int(woff[x + 1])]), (i, j)


def cross_check_exact(ix, pats, got):
    """max_mm = 0 is the exact search: count_batch / locate_batch."""
    nh, more, mm, subs, rng, loff, locs = got
    assert mm.shape[1] == 1
    keep = [i for i, p in enumerate(pats) if p]  # (count rejects an empty pattern)
    cnt = ix.count_batch([pats[i] for i in keep])
    woff, wlocs = ix.locate_batch([pats[i] for i in keep])
    assert not more.any() and not mm.any() and not subs.any()
    for x, i in enumerate(keep):
        assert int(nh[i]) == int(cnt[x] > 0) and int(rng[i, 0, 1] - rng[i, 0, 0]) == int(cnt[x])
        assert np.array_equal(locs[int(loff[i]):int(loff[i + 1])], wlocs[int(woff[x]):int(woff[x + 1])])


# ------------------------------------------------------------------ the cases

def three_mismatches(ix, orc, case, best):
    """max_mm = 3 (patterns of at most 12 symbols): all three frames."""
    pats = batch(case, 257, 3, 12)
    exp, _ = check_approx(ix, orc, case, pats, max_mm=3, max_hits=8, best=best, reversed=best)
    assert set(np.unique(exp[2][exp[4][:, :, 1] > 0]).tolist()) == {0, 1, 2, 3}


def two_letters(pkg, O, n, sr, layouts):
    """A two-letter text: dozens of variants per pattern (max_hits = 32 is
    exceeded), hits with hundreds of rows (the row dealing of k_emit), under
    every sampling ratio's walk."""
    case = case_for(2, two_letters=True, k=3, sr=sr)
    for pb, vb in layouts:
        ix, orc = open_index(pkg, O, case, pb, 2, vb, 1)
        pats = batch(case, n, 2)
        exp, _ = check_approx(ix, orc, case, pats, max_mm=2, max_hits=32)
        assert exp[1].sum() >= 1 and (exp[0] == 32).sum() >= 1 and int(np.diff(exp[5]).max()) >= 100
        check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, reversed=True, max_occ=40)
        ix.close()


def filters(pkg, O, n):
    """max_occ only selects which hits are located: everything else is the
    same across max_occ."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n, 1)
    first = None
    for max_occ in (0, 1, 10, None):
        exp, got = check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, max_occ=max_occ)
        first = first or got
        assert all(np.array_equal(got[j], first[j]) for j in range(5))
        if max_occ == 0:
            assert got[6].size == 0
    ix.close()


def ranges_only_and_capacity(pkg, O, n):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n, 1)
    check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, locate=False)
    for p in (pats[5], pats[40], pats[200]):
        v = variants(case, orc, p, 2)
        assert ix.approx(p, 2, 8) == [x[:4] for x in v[:8]]
        assert ix.approx(p, 2, 8, best=True) == [x[:4] for x in v if x[0] == v[0][0]][:8]
    assert ix.approx(b"") == [] and ix.approx(bytes([ABSENT]) * 2) == []
    # a cap below needed: FMX_E_CAPACITY, needed exact, everything but the locations written
    mh = 3
    exp = expected_arrays(case, orc, pats, 1, mh, False, None)
    total = int(exp[5][-1])
    data, offsets = pkg.pack_patterns(pats)
    lib, nat = pkg._native.lib(), pkg._native

    def call(cap, nh_ptr=True, max_mm=1, max_hits=mh, mode=0):
        o = [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full((n, mh), 7, np.uint32),
             np.full((n, mh, 3, 2), 7, np.uint32), np.full((n, mh, 2), 7, np.uint32), np.full(n * mh + 1, 7, np.uint64),
             np.full(max(total, 1), 7, np.uint32)]
        needed = C.c_uint64(99)
        st = lib.fmx_approx_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, max_mm, max_hits, mode,
                                  (1 << 64) - 1, o[0].ctypes.data if nh_ptr else None, o[1].ctypes.data,
                                  o[2].ctypes.data, o[3].ctypes.data, o[4].ctypes.data, o[5].ctypes.data,
                                  o[6].ctypes.data, cap, C.byref(needed))
        return st, needed.value, o
    st, needed, o = call(total - 1)
    assert st == nat.FMX_E_CAPACITY and needed == total
    compare(o[:5], exp, locate=False)
    assert np.array_equal(o[5], exp[5])
    st, needed, o = call(total)
    assert st == 0 and needed == total
    compare(o[:6] + [o[6][:total]], exp)
    # argument checks
    assert call(total, max_mm=4)[0] == nat.FMX_E_ARG
    assert call(total, max_hits=0)[0] == nat.FMX_E_ARG and call(total, max_hits=33)[0] == nat.FMX_E_ARG
    assert call(total, mode=2)[0] == nat.FMX_E_ARG and call(total, mode=3)[0] == nat.FMX_E_ARG
    assert call(total, nh_ptr=False)[0] == nat.FMX_E_ARG
    ix.close()


def pass_through(pkg, O):
    """PassThrough: a byte >= symbol_count is matched only by substituting it
    (no FMX_E_SYMBOL, nothing latched)."""
    rng = np.random.default_rng(14)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, where = [], []
    for m in (1, 2, 5, 9, 12) * 8:
        s = int(rng.integers(0, len(text) - m))
        for bad in (9, 200, 5):
            j = int(rng.integers(0, m))
            q = bytearray(text[s:s + m])
            q[j] = bad
            pats.append(bytes(q))
            where.append(j)
    two = bytearray(text[100:110])  # two such bytes: no hit at max_mm = 1, both substituted at 2
    two[3], two[8] = 77, 6
    pats.append(bytes(two))
    where.append(None)
    assert not ix.approx_batch(pats, max_mm=0, max_hits=4, locate=False)[0].any()
    nh, more, mm, subs, rg, loff, locs = ix.approx_batch(pats, max_mm=1, max_hits=4)
    for i, (p, j) in enumerate(zip(pats, where)):
        if j is None:
            assert nh[i] == 0
            continue
        want = []
        for c in range(4):  # ascending symbol order; the own symbol cannot be kept
            v = p[:j] + bytes([c]) + p[j + 1:]
            if orc.count(v):
                want.append((c, v))
        assert nh[i] == len(want) >= 1 and more[i] == 0, (i, p)
        for h, (c, v) in enumerate(want):
            assert mm[i, h] == 1 and subs[i, h].tolist() == [[j, c], [0, 0], [0, 0]]
            assert int(rg[i, h, 1] - rg[i, h, 0]) == orc.count(v)
            assert locs[int(loff[4 * i + h]):int(loff[4 * i + h + 1])].tolist() == orc.locate(v)
    nh2, _, mm2, subs2, _ = ix.approx_batch(pats[-1:], max_mm=2, max_hits=32, locate=False)
    assert nh2[0] >= 1 and (mm2[0, :nh2[0]] == 2).all()
    assert (subs2[0, :nh2[0], 0, 0] == 8).all() and (subs2[0, :nh2[0], 1, 0] == 3).all()
    ix.sync()  # nothing latched
    ix.close()


def device_call(pkg, dev, ix, pats, exp, mh, **kw):
    """One fmx_approx_batch_async on dev.stream over buffers in `dev`, the
    outputs prefilled and the workspace garbage: d_needed, every output and the
    untouched tail of the locations checked.  Returns (the inputs, the
    outputs, d_needed, the workspace) as put() gave them, and the outputs
    read back."""
    n, total = len(pats), int(exp[5][-1])
    ins = [dev.put(a) for a in pkg.pack_patterns(pats)]
    rnd = np.random.default_rng(4)
    shapes = [(n,), (n,), (n, mh), (n, mh, 3, 2), (n, mh, 2), (n * mh + 1,), (total + 4,)]
    dts = [np.uint32] * 5 + [np.uint64, np.uint32]
    o = [dev.filled(rnd, sh, dt) for sh, dt in zip(shapes, dts)]
    need = dev.filled(rnd, 1, np.uint64)
    wsb = ix.locate_workspace_size(n * mh)
    ws = dev.workspace(rnd, wsb) + (wsb,)
    dev.sync()
    ix.approx_batch_async(ins[0][1], ins[1][1], n, *[x[1] for x in o], total + 4, need[1], ws[1], wsb, max_hits=mh,
                          stream=dev.stream, **kw)
    ix.sync(dev.stream)
    assert int(dev.get(need[0], np.uint64)[0]) == total
    got = [dev.get(x[0], dt).reshape(sh) for x, sh, dt in zip(o, shapes, dts)]
    assert np.array_equal(got[6][total:], o[6][2][total:])  # (the prefill, untouched)
    compare(got[:6] + [got[6][:total]], exp)
    return ins, o, need, ws, got


def async_call(pkg, O, dev, n):
    """fmx_approx_batch_async on dev.stream: with locations, ranges only with
    no workspace, a disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the
    "approx" timer, the argument checks."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n, 2)
    mh = 3
    exp = expected_arrays(case, orc, pats, 2, mh, True, 10)
    total = int(exp[5][-1])
    ix.timing_enable(True)
    ins, o, need, ws, got = device_call(pkg, dev, ix, pats, exp, mh, max_mm=2, best=True, max_occ=10)
    t = ix.timing_read()["approx"]
    assert t["launches"] == 1 and t["units"] == n * mh
    ix.timing_enable(False)
    d_data, d_off, ptr = ins[0][1], ins[1][1], [x[1] for x in o]
    # ranges only: no workspace, no location arguments
    rnd = np.random.default_rng(5)
    o2 = [dev.filled(rnd, g.shape) for g in got[:5]]
    p2 = [x[1] for x in o2]
    dev.sync()
    ix.approx_batch_async(d_data, d_off, n, *p2, max_mm=2, max_hits=mh, best=True, stream=dev.stream)
    ix.sync(dev.stream)
    got2 = [dev.get(x[0], np.uint32).reshape(g.shape) for x, g in zip(o2, got)]
    compare(got2, exp, locate=False)
    assert all(np.array_equal(a, b) for a, b in zip(got2, got))
    # argument checks
    for kw in (dict(max_hits=0), dict(max_hits=33), dict(max_mm=4)):
        with pytest.raises(pkg.FmxError) as e:
            ix.approx_batch_async(d_data, d_off, n, *p2, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    for z in range(5):  # every required pointer
        q = list(p2)
        q[z] = 0
        with pytest.raises(pkg.FmxError) as e:
            ix.approx_batch_async(d_data, d_off, n, *q, max_hits=mh)
        assert e.value.code == pkg._native.FMX_E_ARG
    lib = pkg._native.lib()
    v = C.c_void_p
    assert lib.fmx_approx_batch_async(ix.handle, v(d_data), v(d_off), n, 0, 1, mh, 2, 0, *[v(x) for x in p2], None, None,
                                      0, None, None, 0, None) == pkg._native.FMX_E_ARG
    # locations without a workspace, or without d_needed
    with pytest.raises(pkg.FmxError) as e:
        ix.approx_batch_async(d_data, d_off, n, *ptr, total, need[1], 0, 0, max_hits=mh)
    assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        ix.approx_batch_async(d_data, d_off, n, *ptr, total, 0, ws[1], ws[2], max_hits=mh)
    assert e.value.code == pkg._native.FMX_E_ARG
    # more slots than a launch's tiles hold (checked before any pointer is used)
    assert lib.fmx_approx_batch_async(ix.handle, v(d_data), v(d_off), (1 << 40), 0, 1, 32, 0, 0, *[v(x) for x in p2], None,
                                      None, 0, None, None, 0, None) == pkg._native.FMX_E_ARG
    # a fixed-length hint the offsets disagree with
    ix.approx_batch_async(d_data, d_off, n, *p2, max_hits=mh, fixed_len=7, stream=dev.stream)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync(dev.stream)
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
