"""Longest-suffix match (fmx_match_batch): the cases, their bodies and the
expected values the emulator tests (test_match_simt.py) and the GPU tests
(test_gpu_match.py) share.  A body takes what differs between the two: the
batch size, the layouts to visit, the device memory (_util.HostDev / TorchDev).

Expected values, per pattern p of length m (computed once per text and
cached):
  * L = the largest t with OracleIndex.count(p[m-t:]) > 0 (monotone in t: a
    suffix of an occurring string occurs), 0 if none;
  * S = p[m-L:]; hi - lo = OracleIndex.count(S); the locations are
    OracleIndex.locate(S), element-wise;
  * lo = the number of non-empty suffixes of the encoded text that sort before
    S by plain byte order (a proper prefix first), from a suffix list sorted
    in Python — and OracleIndex.locate(S) must equal sa[lo:hi] of that list,
    which ties the oracle's row order to the plain order (asserted here, on
    the reference alone, before anything is compared with it).
"""
import bisect
import ctypes as C

import numpy as np
import pytest

from _util import (block_of, case_for, encode, open_index, pos_of, rand_chr_list, rand_text,  # noqa: F401
                   table_from_symbols)

ABSENT = 0  # byte 0x00: maps to the wildcard symbol, which no text here holds
BATCH_SIZES = (1, 255, 256, 257, 700)


class Case:
    """One text: `nchars` distinct printable bytes plus a wildcard symbol that
    does not occur in it (symbol_count = nchars + 1), k and sr in 1..4.
    n_text: a text of exactly that many symbols from a stream of its own (the
    alphabet, k and sr stay what they are without it) in place of the 300 to
    4,000 of the default."""

    def __init__(self, seed, nchars, k=None, sr=None, n_text=None):
        rng = np.random.default_rng(seed)
        self.chars = rand_chr_list(rng, nchars)
        self.table = table_from_symbols([bytes([c]) for c in self.chars], with_wildcard=True)
        self.sigma = nchars + 1
        self.text = rand_text(rng, self.chars, 300, 4000)
        if n_text is not None:
            self.text = rand_text(np.random.default_rng(seed + 7), self.chars, n_text, n_text)
        self.k = int(rng.integers(1, 5)) if k is None else k
        self.sr = int(rng.integers(1, 5)) if sr is None else sr
        while (self.sigma + 1) ** self.k > 1 << 20:
            self.k -= 1
        self.seed = seed
        self.enc = encode(self.table, self.text)
        self._sa = None
        self._exp = {}

    def blob(self, O, pb, planes, vb):
        return O.build(self.text, self.sigma, O.layout(pb, planes, vb), self.k, self.sr, self.table)

    # -- the reference ---------------------------------------------------
    def suffixes(self):
        if self._sa is None:
            e = self.enc
            sa = sorted(range(len(e)), key=lambda i: e[i:])
            self._sa = (sa, [e[i:] for i in sa])
        return self._sa

    def expected(self, orc, p):
        """(L, lo, hi, locations) of pattern p (bytes, logical order)."""
        got = self._exp.get(p)
        if got is not None:
            return got
        m = len(p)
        lo_t, hi_t = 0, m  # count(p[m-t:]) > 0 for t <= lo_t; binary search on the monotone predicate
        while lo_t < hi_t:
            mid = (lo_t + hi_t + 1) // 2
            if orc.count(p[m - mid:]) > 0:
                lo_t = mid
            else:
                hi_t = mid - 1
        L = lo_t
        if L == 0:
            got = (0, 0, 0, [])
        else:
            S = p[m - L:]
            cnt = orc.count(S)
            locs = orc.locate(S)
            sa, suf = self.suffixes()
            lo = bisect.bisect_left(suf, encode(self.table, S))
            assert len(locs) == cnt and locs == sa[lo:lo + cnt], "oracle row order != plain suffix order"
            assert L == m or orc.count(p[m - L - 1:]) == 0
            got = (L, lo, lo + cnt, locs)
        self._exp[p] = got
        return got

    # -- the patterns ------------------------------------------------------
    def other(self, rng, c):
        """A byte of the alphabet other than c (one symbol only: the absent byte)."""
        rest = [x for x in self.chars if x != c]
        return int(rng.choice(rest)) if rest else ABSENT

    def core(self):
        """Every case class once or more (fewer than 255 patterns)."""
        rng = np.random.default_rng(self.seed + 1000)
        t, k, n = self.text, self.k, len(self.text)
        pats = []

        def sub(m):
            s = int(rng.integers(0, n - m))
            return t[s:s + m]

        def subst(p, j):
            q = bytearray(p)
            q[j] = self.other(rng, q[j])
            return bytes(q)
        # substrings: full matches
        for m in sorted({1, 2, k - 1, k, k + 1, 7, 40} - {0}):
            pats += [sub(m) for _ in range(4)]
        # one symbol substituted: inside the last k (the seed falls back: L < k), at m - k - 1 (the first
        # LF step fails: L = k), further left
        for m in (k + 2, 12, 40):
            for j in range(k):
                pats.append(subst(sub(m), m - 1 - j))
            pats += [subst(sub(m), m - k - 1) for _ in range(3)]
            if m - k - 1 > 0:
                pats += [subst(sub(m), int(rng.integers(0, m - k - 1))) for _ in range(3)]
        # a last byte that the text does not hold: L = 0
        pats += [sub(m) + bytes([ABSENT]) for m in (0, 1, k, 9)]
        pats.insert(len(pats) // 2, b"")  # an empty pattern in mid-batch
        # c + text[:j]: the match reaches the text start (the sentinel adjustment, the walk's text-start exit)
        for c in list(self.chars) + [ABSENT]:
            for j in (1, k, 9, 30):
                pats.append(bytes([c]) + t[:j])
        # substrings long enough to be unique, a wrong symbol before them: the match ends in the
        # single-row phase with one step rolled back (the sampled-row bookkeeping)
        for _ in range(12):
            s = int(rng.integers(1, n - 30))
            pats.append(bytes([self.other(rng, t[s - 1])]) + t[s:s + 30])
        # an absent symbol in the middle and right before the seed
        pats += [sub(6) + bytes([ABSENT]) + sub(k + 3), sub(3) + bytes([ABSENT]) + sub(k)]
        assert len(pats) < 255
        return pats

    def batch(self, n):
        """n patterns: one mismatching read for n = 1, else the core classes
        followed by substrings, substituted or not."""
        core = self.core()
        if n == 1:
            return [core[40]]
        rng = np.random.default_rng(self.seed + n)
        t, pats = self.text, list(core)
        while len(pats) < n:
            m = int(rng.integers(1, 41))
            s = int(rng.integers(0, len(t) - m))
            q = bytearray(t[s:s + m])
            if rng.integers(0, 2):
                j = int(rng.integers(0, m))
                q[j] = self.other(rng, q[j])
            pats.append(bytes(q))
        return pats[:n]


def check_match(pkg, ix, orc, case, pats, reversed=False, min_len=1, max_occ=None, locate=True):
    """match_batch of `pats` against the expected values; returns them."""
    exp = [case.expected(orc, p) for p in pats]
    q = [p[::-1] for p in pats] if reversed else pats
    out = ix.match_batch(q, reversed=reversed, locate=locate, min_len=min_len, max_occ=max_occ)
    lens, rng = out[0], out[1]
    n = len(pats)
    assert lens.dtype == np.uint32 and lens.shape == (n,) and rng.shape == (n, 2)
    eL = np.array([e[0] for e in exp], dtype=np.int64)
    elo = np.array([e[1] for e in exp], dtype=np.int64)
    ehi = np.array([e[2] for e in exp], dtype=np.int64)
    bad = np.flatnonzero(lens.astype(np.int64) != eL)
    assert bad.size == 0, (f"lengths differ for {bad.size} patterns, first {bad[:5].tolist()}: "
                           f"{lens[bad[:5]].tolist()} expected {eL[bad[:5]].tolist()} ({[pats[i] for i in bad[:3]]})")
    bad = np.flatnonzero((rng[:, 0].astype(np.int64) != elo) | (rng[:, 1].astype(np.int64) != ehi))
    assert bad.size == 0, (f"ranges differ for {bad.size} patterns, first {bad[:5].tolist()}: "
                           f"{rng[bad[:5]].tolist()} expected {list(zip(elo[bad[:5]].tolist(), ehi[bad[:5]].tolist()))}")
    if not locate:
        assert len(out) == 2
        return exp
    loff, locs = out[2], out[3]
    need = max(min_len, 1)
    rep = [e[0] >= need and (max_occ is None or e[2] - e[1] <= max_occ) for e in exp]
    ecnt = np.array([e[2] - e[1] if r else 0 for e, r in zip(exp, rep)], dtype=np.uint64)
    eoff = np.concatenate([np.zeros(1, np.uint64), np.cumsum(ecnt, dtype=np.uint64)])
    assert np.array_equal(loff, eoff), "location offsets differ"
    elocs = [x for e, r in zip(exp, rep) if r for x in e[3]]
    assert np.array_equal(locs.astype(np.uint64), np.array(elocs, dtype=np.uint64)), "locations differ (SA-row order)"
    return exp


# ------------------------------------------------------------------ the cases

def classes_and_full_match_check(ix, case, pats, exp):
    """What a sweep's batch of >= 256 patterns must hold (on the expected
    values alone), and a fully matching pattern's locations against the
    shipped locate_batch on the same index."""
    L = np.array([e[0] for e in exp])
    m = np.array([len(p) for p in pats])
    assert (L == 0).sum() >= 4 and (L == m).sum() >= 20 and (L == case.k).sum() >= 1 \
        and (L > case.k).sum() >= 20 and (case.k == 1 or ((L > 0) & (L < case.k)).sum() >= 1), \
        "case classes missing from the batch"
    # a fully matching pattern: exactly what locate_batch returns for it
    full = [p for p, e in zip(pats, exp) if e[0] == len(p) and len(p)]
    _, rng, loff, locs = ix.match_batch(full)
    woff, wlocs = ix.locate_batch(full)
    assert np.array_equal(loff, woff) and np.array_equal(locs, wlocs)
    assert np.array_equal((rng[:, 1] - rng[:, 0]).astype(np.uint64), np.diff(woff))


def two_letters(pkg, O, n, sr, layouts):
    """A two-letter text: short matched suffixes have hundreds of rows (the
    row dealing of k_emit), under every sampling ratio's walk."""
    case = case_for(2, two_letters=True, k=3, sr=sr)
    for pb, vb in layouts:
        ix, orc = open_index(pkg, O, case, pb, 2, vb, 1)
        pats = case.batch(n)
        exp = check_match(pkg, ix, orc, case, pats)
        assert max(e[2] - e[1] for e in exp) >= 300
        check_match(pkg, ix, orc, case, pats, reversed=True, max_occ=400)
        ix.close()


def filters(pkg, O, n, min_len, max_occ):
    """min_len / max_occ: lengths and ranges unchanged, locations only for the
    reporting patterns."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    check_match(pkg, ix, orc, case, case.batch(n), min_len=min_len, max_occ=max_occ)
    ix.close()


def ranges_only_and_capacity(pkg, O, n):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = case.batch(n)
    exp = check_match(pkg, ix, orc, case, pats, locate=False)
    assert ix.match(pats[5]) == exp[5][:3]
    assert ix.match(b"") == (0, 0, 0) and ix.match(bytes([ABSENT])) == (0, 0, 0)
    # a cap below needed: FMX_E_CAPACITY, needed exact, lengths / ranges / offsets written all the same
    total = sum(e[2] - e[1] for e in exp if e[0] >= 1)
    data, offsets = pkg.pack_patterns(pats)
    lens, rng = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32)
    loff, locs, needed = np.zeros(n + 1, np.uint64), np.zeros(total, np.uint32), C.c_uint64()
    lib = pkg._native.lib()
    args = lambda cap: (ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, (1 << 64) - 1, lens.ctypes.data,  # noqa
                        rng.ctypes.data, loff.ctypes.data, locs.ctypes.data, cap, C.byref(needed))
    assert lib.fmx_match_batch(*args(total - 1)) == pkg._native.FMX_E_CAPACITY
    assert needed.value == total and int(loff[-1]) == total
    assert lens.tolist() == [e[0] for e in exp] and rng[:, 0].tolist() == [e[1] for e in exp]
    assert lib.fmx_match_batch(*args(total)) == 0 and needed.value == total
    assert locs.tolist() == [x for e in exp for x in e[3]]
    # argument checks: no outputs, locations without a buffer
    assert lib.fmx_match_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, 0, None, rng.ctypes.data,
                               None, None, 0, None) == pkg._native.FMX_E_ARG
    assert lib.fmx_match_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, 0, lens.ctypes.data,
                               rng.ctypes.data, loff.ctypes.data, None, 5, None) == pkg._native.FMX_E_ARG
    ix.close()


def pass_through(pkg, O):
    """PassThrough: a byte >= symbol_count ends the match before it (no
    FMX_E_SYMBOL), among the seed's symbols and beyond them."""
    rng = np.random.default_rng(12)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, want = [], []
    for m in [1, 2, 3, 4, 9, 30] * 8:
        s = int(rng.integers(0, len(text) - m))
        p = text[s:s + m]
        for bad in (9, 200):
            for cut in sorted({0, 1, min(2, m), min(k, m), m}):  # valid symbols after the bad byte
                q = p[:m - cut] + bytes([bad]) + p[m - cut:]
                pats.append(q)
                want.append(q[len(q) - cut:])
    lens, rg, loff, locs = ix.match_batch(pats)
    for i, (p, w) in enumerate(zip(pats, want)):
        L = len(w)
        while L and orc.count(w[len(w) - L:]) == 0:  # (the valid tail itself may not occur whole)
            L -= 1
        assert lens[i] == L, (i, p, w)
        S = w[len(w) - L:]
        assert int(rg[i, 1] - rg[i, 0]) == (orc.count(S) if L else 0)
        assert locs[int(loff[i]):int(loff[i + 1])].tolist() == (orc.locate(S) if L else [])
    ix.sync()  # nothing latched
    ix.close()


def device_call(pkg, O, dev, n):
    """fmx_match_batch_async over buffers in `dev`: with locations over a
    garbage workspace and prefilled outputs, ranges only with no workspace, a
    disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the "match" timer."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = case.batch(n)
    exp = [case.expected(orc, p) for p in pats]
    data, offsets = pkg.pack_patterns(pats)
    rnd = np.random.default_rng(3)
    rep = [e[0] >= 5 and e[2] - e[1] <= 10 for e in exp]
    total = sum(e[2] - e[1] for e, r in zip(exp, rep) if r)
    ins = [dev.put(np.concatenate([data, np.zeros(16, np.uint8)])), dev.put(offsets)]
    o = [dev.filled(rnd, n), dev.filled(rnd, (n, 2)), dev.filled(rnd, n + 1, np.uint64),
         dev.put(np.zeros(total + 4, np.uint32)), dev.put(np.zeros(1, np.uint64))]
    wsb = ix.locate_workspace_size(n)
    ws = dev.workspace(rnd, wsb)
    dev.sync()
    ix.timing_enable(True)
    ix.match_batch_async(ins[0][1], ins[1][1], n, *[x[1] for x in o[:4]], total + 4, o[4][1], ws[1], wsb,
                         min_len=5, max_occ=10)
    ix.sync()
    assert ix.timing_read()["match"]["launches"] == 1
    ix.timing_enable(False)
    lens, rng = dev.get(o[0][0], np.uint32), dev.get(o[1][0], np.uint32).reshape(n, 2)
    assert lens.tolist() == [e[0] for e in exp]
    assert rng.tolist() == [[e[1], e[2]] for e in exp]
    assert int(dev.get(o[4][0], np.uint64)[0]) == total
    assert np.diff(dev.get(o[2][0], np.uint64)).tolist() == [e[2] - e[1] if r else 0 for e, r in zip(exp, rep)]
    assert dev.get(o[3][0], np.uint32)[:total].tolist() == [x for e, r in zip(exp, rep) if r for x in e[3]]
    # ranges only: no workspace, no location arguments
    o2 = [dev.put(np.zeros(n, np.uint32)), dev.put(np.zeros((n, 2), np.uint32))]
    dev.sync()
    ix.match_batch_async(ins[0][1], ins[1][1], n, o2[0][1], o2[1][1])
    ix.sync()
    assert np.array_equal(dev.get(o2[0][0], np.uint32), lens)
    assert np.array_equal(dev.get(o2[1][0], np.uint32).reshape(n, 2), rng)
    # a fixed-length hint the offsets disagree with
    ix.match_batch_async(ins[0][1], ins[1][1], n, o2[0][1], o2[1][1], fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
