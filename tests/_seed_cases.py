"""Greedy seed chains (fmx_seeds_batch): the cases and expected values the
emulator tests (test_seeds_simt.py) and the GPU tests (test_gpu_seeds.py)
share.

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
import numpy as np

from _match_cases import ABSENT, Case

BATCH_SIZES = (1, 255, 256, 257, 700)
_CASES = {}
_POOLS = {}


def case_for(planes, two_letters=False, **kw):
    """One text per alphabet size (its expected values are computed once and
    shared by every test of the run)."""
    key = (planes, two_letters, tuple(sorted(kw.items())))
    if key not in _CASES:
        nchars = 2 if two_letters else min((1 << planes) - 1, 20)
        _CASES[key] = Case(planes * 11 + (5 if two_letters else 0), nchars, **kw)
    return _CASES[key]


def pos_of(pkg, pb):
    return pkg.u32 if pb == 4 else pkg.u64


def block_of(pkg, planes, vb):
    return getattr(pkg.blocks, f"Block{planes}")(pkg.Vector(vb))


def open_index(pkg, O, case, pb, planes, vb, occ):
    blob = case.blob(O, pb, planes, vb)
    orc = O.OracleIndex(blob, O.layout(pb, planes, vb, 0))
    return pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=occ), orc


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
