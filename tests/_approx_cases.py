"""k-mismatch search (fmx_approx_batch): the cases and expected values the
emulator tests (test_approx_simt.py) and the GPU tests (test_gpu_approx.py)
share.

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
from math import comb as _comb

import numpy as np

from _match_cases import ABSENT, Case  # noqa: F401
from _seed_cases import block_of, case_for, open_index, pos_of  # noqa: F401
from _util import encode

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
