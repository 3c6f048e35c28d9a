"""Greedy seed chains (fmx_seeds_batch): the cases, their bodies and the
expected values the emulator tests (test_seeds_simt.py) and the GPU tests
(test_gpu_seeds.py) share.  A body takes what differs between the two: the
batch size, the layouts to visit, the device memory (_util.HostDev / TorchDev).

The reference is built only from _match_cases.Case.expected, which already
ties the oracle to a plainly sorted suffix list: Python runs the loop of
include/fmx.h over the prefixes p[:e] — (L, lo, hi, locations) =
expected(p[:e]); a seed when L >= max(min_len, 1); e -= min(e, max(L + skip,
1)) — until e = 0 or max_seeds are stored.  A seed's locations are the
oracle's locate of its substring (expected's fourth value).

A batch of n patterns is cut from one pool per text: Case.batch(257), 200
chimeras (2-5 substrings of the text, 1-24 symbols each, concatenated), one
pattern of 20 one-symbol seeds (bytes([ABSENT, chars[0]]) * 20) and random
substrings.  n = 1 is Case.batch(1) (one mismatching read); any other n takes
the chimeras and the 20-seed pattern whole, the first n - 201 patterns of
Case.batch(257) in front of them (at most all 257; reordered: its two seedless
patterns, then those that occur whole in the text, then the others, chosen by
what the patterns are, not by any answer) and substrings behind them up to n —
so that the batches of 255,
256 and 257 patterns, which put the tile boundaries where the kernel can go
wrong, hold every class as well (assert_classes below, on the expected values
alone).
"""
import ctypes as C

import numpy as np
import pytest

from _match_cases import ABSENT
from _util import block_of, case_for, open_index, pos_of  # noqa: F401

BATCH_SIZES = (1, 255, 256, 257, 700)
_POOLS = {}


def _pool(case):
    got = _POOLS.get(id(case))
    if got is None:
        rng = np.random.default_rng(5)
        t = case.text

        def sub(lo, hi):
            m = int(rng.integers(lo, hi + 1))
            s = int(rng.integers(0, len(t) - m))
            return t[s:s + m]
        chim = [b"".join(sub(1, 24) for _ in range(int(rng.integers(2, 6)))) for _ in range(200)]
        many = bytes([ABSENT, case.chars[0]]) * 20
        subs = [sub(1, 40) for _ in range(700)]
        # Case.batch(257) with its two seedless patterns first, then those that occur whole (one seed,
        # whatever the skip), then the rest in its own order
        b257 = case.batch(257)
        none = [b"", bytes([ABSENT])]
        assert all(p in b257 for p in none)
        whole = [p for p in b257 if p and p in t]
        base = none + whole + [p for p in b257 if p not in none and p not in t]
        base += [b""] * (len(b257) - len(base))  # (duplicates of the seedless ones collapse above)
        got = _POOLS[id(case)] = (base[:257], chim, many, subs)
    return got


def batch(case, n):
    if n == 1:
        return case.batch(1)
    base, chim, many, subs = _pool(case)
    assert n > 201
    pats = base[:min(n - 201, len(base))] + chim + [many]
    return pats + subs[:n - len(pats)]


def chain(case, orc, p, max_seeds, min_len=1, skip=0):
    """([(end, L, lo, hi, locations)], rest) of pattern p."""
    e, out, need = len(p), [], max(min_len, 1)
    while e > 0 and len(out) < max_seeds:
        L, lo, hi, locs = case.expected(orc, p[:e])
        if L >= need:
            out.append((e, L, lo, hi, locs))
        e -= min(e, max(L + skip, 1))
    return out, e


def assert_classes(case, orc, pats, skip):
    """What a sweep of >= 256 patterns must hold (min_len = 1, no slot limit)."""
    ns = np.array([len(chain(case, orc, p, 1 << 30, 1, skip)[0]) for p in pats])
    got = {j: int((ns == j).sum()) for j in range(6)}
    assert got[0] >= 2 and all(got[j] >= 30 for j in (1, 2, 3, 4, 5)) and (ns > 8).sum() >= 1, \
        f"case classes missing from the batch: {got}, max {ns.max()}"


def expected_arrays(case, orc, pats, max_seeds, min_len, skip, max_occ):
    """The call's expected outputs as arrays: nseeds, rest, spans, ranges,
    loc_offsets, locations."""
    n, ms = len(pats), max_seeds
    ns, rest = np.zeros(n, np.int64), np.zeros(n, np.int64)
    spans, rng = np.zeros((n, ms, 2), np.int64), np.zeros((n, ms, 2), np.int64)
    cnt, locs = np.zeros(n * ms, np.uint64), []
    for i, p in enumerate(pats):
        seeds, rest[i] = chain(case, orc, p, ms, min_len, skip)
        ns[i] = len(seeds)
        for j, (e, L, lo, hi, ll) in enumerate(seeds):
            spans[i, j] = (e, L)
            rng[i, j] = (lo, hi)
            if max_occ is None or hi - lo <= max_occ:
                cnt[i * ms + j] = hi - lo
                locs += ll
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
    return ns, rest, spans, rng, off, np.array(locs, dtype=np.uint64)


def compare(got, exp, locate=True):
    """(nseeds, rest, spans, ranges[, loc_offsets, locations]) against
    expected_arrays: every slot, every offset, the locations element-wise."""
    names = ("nseeds", "rest", "spans", "ranges")
    for name, g, e in zip(names, got, exp):
        g = np.asarray(g)
        assert g.shape == e.shape, (name, g.shape, e.shape)
        bad = np.argwhere(g.astype(np.int64) != e)
        assert bad.size == 0, f"{name} differ at {len(bad)} places, first {bad[:4].tolist()}: " \
                              f"{[int(g[tuple(b)]) for b in bad[:4]]} expected {[int(e[tuple(b)]) for b in bad[:4]]}"
    if not locate:
        assert len(got) == 4
        return
    assert len(got) == 6
    assert np.array_equal(np.asarray(got[4]).astype(np.uint64), exp[4]), "location offsets differ"
    assert np.array_equal(np.asarray(got[5]).astype(np.uint64), exp[5]), "locations differ (SA-row order)"


def check_seeds(ix, orc, case, pats, max_seeds=8, min_len=1, skip=0, max_occ=None, reversed=False, locate=True):
    """seeds_batch of `pats` against the expected values; returns (expected, got)."""
    exp = expected_arrays(case, orc, pats, max_seeds, min_len, skip, max_occ)
    q = [p[::-1] for p in pats] if reversed else pats
    got = ix.seeds_batch(q, max_seeds=max_seeds, min_len=min_len, skip=skip, max_occ=max_occ, reversed=reversed,
                         locate=locate)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    compare(got, exp, locate)
    return exp, got


def cross_check(ix, pats, got):
    """Against the shipped calls on the same index (min_len = 1): slot 0 is
    match_batch's answer wherever it matched anything; a pattern that occurs
    whole has the one seed (m, m, ., .) and locate_batch's locations."""
    ns, rest, spans, rng, loff, locs = got
    lens, mrng = ix.match_batch(pats, locate=False)
    m = np.array([len(p) for p in pats])
    hit = lens >= 1
    assert hit.sum() >= 200 and (ns[hit] >= 1).all()
    assert np.array_equal(spans[hit, 0, 0], m[hit]) and np.array_equal(spans[hit, 0, 1], lens[hit])
    assert np.array_equal(rng[hit, 0], mrng[hit])
    whole = np.flatnonzero((lens == m) & (m > 0))
    assert whole.size >= 20
    assert (ns[whole] == 1).all() and (rest[whole] == 0).all()
    woff, wlocs = ix.locate_batch([pats[i] for i in whole])
    ms = spans.shape[1]
    for j, i in enumerate(whole):
        a, b = int(loff[i * ms]), int(loff[i * ms + 1])
        assert np.array_equal(locs[a:b], wlocs[int(woff[j]):int(woff[j + 1])])
        assert int(loff[i * ms + ms]) == b  # (its other slots hold nothing)


# ------------------------------------------------------------------ the cases

def two_letters(pkg, O, n, sr, layouts):
    """A two-letter text: seeds with hundreds of rows (the row dealing of
    k_emit), under every sampling ratio's walk."""
    case = case_for(2, two_letters=True, k=3, sr=sr)
    for pb, vb in layouts:
        ix, orc = open_index(pkg, O, case, pb, 2, vb, 1)
        pats = batch(case, n)
        exp, _ = check_seeds(ix, orc, case, pats, max_seeds=3, skip=1)
        assert int(np.diff(exp[4]).max()) >= 300
        check_seeds(ix, orc, case, pats, max_seeds=3, reversed=True, max_occ=400)
        ix.close()


def filters(pkg, O, n, min_len):
    """min_len decides what is a seed; max_occ only which seeds are located:
    spans and ranges are the same across max_occ."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n)
    first = None
    for max_occ in (0, 1, 10, None):
        exp, got = check_seeds(ix, orc, case, pats, max_seeds=3, min_len=min_len, skip=1, max_occ=max_occ)
        first = first or got
        assert np.array_equal(got[2], first[2]) and np.array_equal(got[3], first[3])
        if max_occ == 0:
            assert got[5].size == 0
    if min_len == 5:
        assert (exp[0] == 0).sum() >= 30 and (exp[2][:, :, 1][exp[2][:, :, 1] > 0] >= 5).all()
    ix.close()


def ranges_only_and_capacity(pkg, O, n):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n)
    check_seeds(ix, orc, case, pats, max_seeds=3, skip=1, locate=False)
    s, rest = chain(case, orc, pats[5], 8, 1, 0)
    assert ix.seeds(pats[5]) == [x[:4] for x in s] and rest == 0
    assert ix.seeds(b"") == [] and ix.seeds(bytes([ABSENT])) == []
    many = bytes([ABSENT, case.chars[0]]) * 20
    assert many in pats and len(ix.seeds(many, max_seeds=32)) == 20
    # a cap below needed: FMX_E_CAPACITY, needed exact, everything but the locations written
    ms = 3
    exp = expected_arrays(case, orc, pats, ms, 1, 0, None)
    total = int(exp[4][-1])
    data, offsets = pkg.pack_patterns(pats)
    lib, nat = pkg._native.lib(), pkg._native

    def call(cap, ns_ptr=True, max_seeds=ms):
        o = [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full((n, ms, 2), 7, np.uint32),
             np.full((n, ms, 2), 7, np.uint32), np.full(n * ms + 1, 7, np.uint64), np.full(max(total, 1), 7, np.uint32)]
        needed = C.c_uint64(99)
        st = lib.fmx_seeds_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, max_seeds, 1, 0, (1 << 64) - 1,
                                 o[0].ctypes.data if ns_ptr else None, o[1].ctypes.data, o[2].ctypes.data,
                                 o[3].ctypes.data, o[4].ctypes.data, o[5].ctypes.data, cap, C.byref(needed))
        return st, needed.value, o
    st, needed, o = call(total - 1)
    assert st == nat.FMX_E_CAPACITY and needed == total
    compare(o[:4], exp, locate=False)
    assert np.array_equal(o[4], exp[4])
    st, needed, o = call(total)
    assert st == 0 and needed == total
    compare(o[:5] + [o[5][:total]], exp)
    # argument checks
    assert call(total, max_seeds=0)[0] == nat.FMX_E_ARG and call(total, max_seeds=33)[0] == nat.FMX_E_ARG
    assert call(total, ns_ptr=False)[0] == nat.FMX_E_ARG
    ix.close()


def pass_through(pkg, O):
    """PassThrough: bytes >= symbol_count in mid-pattern split it into seeds
    on both sides (no FMX_E_SYMBOL, nothing latched)."""
    rng = np.random.default_rng(13)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, parts = [], []
    for la, lb in [(1, 1), (2, 3), (3, 2), (9, 4), (4, 9), (12, 12)] * 6:
        a0, b0 = int(rng.integers(0, len(text) - la)), int(rng.integers(0, len(text) - lb))
        a, b = text[a0:a0 + la], text[b0:b0 + lb]
        for bad in (bytes([9]), bytes([200]), bytes([4, 77])):
            pats.append(a + bad + b)
            parts.append((a, bad, b))
    for skip in (0, 1):
        ns, rest, spans, rg, loff, locs = ix.seeds_batch(pats, max_seeds=4, skip=skip)
        for i, (a, bad, b) in enumerate(parts):
            m = len(pats[i])
            assert ns[i] == 2 and rest[i] == 0, (i, pats[i])
            assert spans[i, :2].tolist() == [[m, len(b)], [len(a), len(a)]] and spans[i, 2:].tolist() == [[0, 0]] * 2
            for j, sub in enumerate((b, a)):
                assert int(rg[i, j, 1] - rg[i, j, 0]) == orc.count(sub)
                assert locs[int(loff[4 * i + j]):int(loff[4 * i + j + 1])].tolist() == orc.locate(sub)
    ix.sync()  # nothing latched
    ix.close()


def device_call(pkg, O, dev, n):
    """fmx_seeds_batch_async over buffers in `dev`: with locations over a
    garbage workspace and prefilled outputs, ranges only with no workspace, a
    disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the "seeds" timer, the
    argument checks."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n)
    ms = 3
    exp = expected_arrays(case, orc, pats, ms, 5, 1, 10)
    total = int(exp[4][-1])
    ins = [dev.put(a) for a in pkg.pack_patterns(pats)]
    d_data, d_off = ins[0][1], ins[1][1]
    rnd = np.random.default_rng(4)
    shapes = [(n,), (n,), (n, ms, 2), (n, ms, 2), (n * ms + 1,), (total + 4,)]
    dts = [np.uint32] * 4 + [np.uint64, np.uint32]
    o = [dev.filled(rnd, sh, dt) for sh, dt in zip(shapes, dts)]
    need = dev.filled(rnd, 1, np.uint64)
    wsb = ix.locate_workspace_size(n * ms)
    ws = dev.workspace(rnd, wsb)
    dev.sync()
    ix.timing_enable(True)
    ix.seeds_batch_async(d_data, d_off, n, *[x[1] for x in o], total + 4, need[1], ws[1], wsb, max_seeds=ms, min_len=5,
                         skip=1, max_occ=10)
    ix.sync()
    assert ix.timing_read()["seeds"]["launches"] == 1
    ix.timing_enable(False)
    assert int(dev.get(need[0], np.uint64)[0]) == total
    got = [dev.get(x[0], dt).reshape(sh) for x, sh, dt in zip(o, shapes, dts)]
    compare(got[:5] + [got[5][:total]], exp)
    assert np.array_equal(got[5][total:], o[5][2][total:])  # (the prefill, untouched)
    # ranges only: no workspace, no location arguments
    o2 = [dev.filled(rnd, sh) for sh in shapes[:4]]
    p2 = [x[1] for x in o2]
    dev.sync()
    ix.seeds_batch_async(d_data, d_off, n, *p2, max_seeds=ms, min_len=5, skip=1)
    ix.sync()
    got2 = [dev.get(x[0], np.uint32).reshape(sh) for x, sh in zip(o2, shapes)]
    compare(got2, exp, locate=False)
    assert all(np.array_equal(a, b) for a, b in zip(got2, got))
    # argument checks
    for kw in (dict(max_seeds=0), dict(max_seeds=33)):
        with pytest.raises(pkg.FmxError) as e:
            ix.seeds_batch_async(d_data, d_off, n, *p2, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        ix.seeds_batch_async(d_data, d_off, n, 0, *p2[1:], max_seeds=ms)
    assert e.value.code == pkg._native.FMX_E_ARG
    # a fixed-length hint the offsets disagree with
    ix.seeds_batch_async(d_data, d_off, n, *p2, max_seeds=ms, fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
