"""Verifying placements (fmx_verify_async, fmx_map_batch, FMX_OPT_VERIFY_TEXT):
the model, the synthetic batches, the runs and the cases' bodies that the
emulator tests (test_verify_simt.py, test_verify_guard_simt.py) and the GPU
tests (test_gpu_verify.py, test_gpu_verify_guard.py) share.

model() is the contract of include/fmx.h in NumPy over case.enc and the encoded
virtual patterns: the forward recurrence F and the anchored backward recurrence
G, both written in the contract's own (i, j) — the backward one as such, not as
a forward pass over reversed strings —, a row per step, vectorised over the
candidates and the band's diagonals, the in-row term by np.minimum.accumulate.
It asserts on its own values that min G[0][.] == D, and plain() — the two
recurrences cell by cell over a dict — checks it on small cases.

make_batch() cuts reads from the text and plants 0..4 edits; its candidates
are the cut's start shifted by -band-1 .. band+1 and the edge positions of the
contract (P < 0 inside and outside the band, P + m > n, P - band > n, P = n -
m), a read with no similarity, reads whose first and last symbol are
substituted (two cheapest ends, two cheapest starts), ncands of 0, 1, max_cands
and max_cands + 1 with junk in the unused positions.  assert_classes checks on
the model's values alone that a batch of 255 reads or more holds every class.
"""
import numpy as np
import pytest

import _guard_cases as G
import _vote_cases as V
from _guard_cases import SKEWS, Arena
from _match_cases import ABSENT
from _seed_cases import BATCH_SIZES, batch, case_for, open_index  # noqa: F401
from _strand_cases import cycle_map, expand, involution, unrc
from _util import HostDev, TorchDev, block_of, encode, pos_of  # noqa: F401

NONE, ANY, MAX_LEN, MAX_BAND = 0xFFFFFFFF, 0xFFFFFFFE, 65535, 31
INF = 1 << 40
VERIFY_TEXT = 64  # FMX_OPT_VERIFY_TEXT
READ_COUNTS = (1, 3, 4, 5, 255, 256, 257)
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129)  # the edges of the 64-symbol read chunk
SHORT = (0, 1, 2, 63, 64, 65, 70)  # the large batches: m <= 70
# (band, max_cands): every band and every max_cands of the contract's edges
CONFIGS = ((8, 4), (0, 1), (1, 16), (31, 4))
LAYOUTS = V.LAYOUTS
JUNK = 0x5A5A5A5A5A5A  # an unused candidate position: never read


# ------------------------------------------------------------------ the model

def model(case, pats, ncands, pos, K, band, max_dist):
    """(dist, tstart, tend) as int64[nv * K] and, for assert_classes, the
    slots' D before max_dist (INF: none), used flag, read length and the
    numbers of cheapest ends and starts."""
    t = np.frombuffer(case.enc, np.uint8).astype(np.int64)
    n, sigma, nv = len(t), case.sigma, len(pats)
    W = 2 * band + 1
    kk = np.arange(W, dtype=np.int64)
    nc = np.minimum(np.asarray(ncands, np.int64), K)
    used = (np.arange(K)[None, :] < nc[:, None]).reshape(-1)
    mlen = np.repeat(np.array([len(p) for p in pats], np.int64), K)
    P = np.asarray(pos, np.int64).reshape(-1)
    dist = np.where(used, NONE, 0).astype(np.int64)
    ts, te = np.zeros(nv * K, np.int64), np.zeros(nv * K, np.int64)
    info = dict(D=np.full(nv * K, INF, np.int64), used=used, m=mlen, ends=np.zeros(nv * K, np.int64),
                starts=np.zeros(nv * K, np.int64))
    idx = np.flatnonzero(used & (mlen <= MAX_LEN))
    if idx.size == 0:
        return dist, ts, te, info
    mm, Pc, C = mlen[idx], P[idx], idx.size
    maxm = int(mm.max())
    Q = np.full((nv, maxm + 1), -1, np.int64)
    for v, p in enumerate(pats):
        if len(p) <= MAX_LEN:
            Q[v, :len(p)] = np.frombuffer(encode(case.table, p), np.uint8)
    Qc = Q[idx // K]
    d = Pc[:, None] - band + kk[None, :]  # the diagonals: j = i + d
    rows = np.arange(C)
    inf_col = np.full((C, 1), INF, np.int64)

    def allowed(i):
        j = i[:, None] + d
        return (j >= 0) & (j <= n)

    def sub(qs, j):  # [q != t[j]]; a symbol >= symbol_count never matches
        tj = np.where((j >= 0) & (j < n), t[np.clip(j, 0, n - 1)], -2)
        return ((qs[:, None] != tj) | (qs[:, None] >= sigma)).astype(np.int64)

    # forward: F[0][j] = 0 on A(0)
    F = np.where(allowed(np.zeros(C, np.int64)), 0, INF)
    for i in range(1, maxm + 1):
        ii = np.full(C, i, np.int64)
        j, ok = ii[:, None] + d, allowed(ii)
        h = np.minimum(F + sub(Qc[:, i - 1], j - 1), np.concatenate([F[:, 1:], inf_col], 1) + 1)
        h = np.where(ok, h, INF)
        Fn = np.minimum.accumulate(h - kk, axis=1) + kk  # F[i][j-1] + 1, along the row
        Fn = np.where(ok, np.minimum(Fn, INF), INF)
        F = np.where((mm >= i)[:, None], Fn, F)
    D = F.min(1)
    kb = (F == D[:, None]).argmax(1)  # the smallest j attaining D
    tend = mm + Pc - band + kb
    fin = D < INF

    # backward: G[m][tend] = 0, the same cells and costs
    def in_row(h):  # G[i][j+1] + 1, along the row from its end
        return np.minimum.accumulate((h + kk)[:, ::-1], axis=1)[:, ::-1] - kk

    Gm = np.full((C, W), INF, np.int64)
    Gm[rows[fin], kb[fin]] = 0
    Gm = np.where(allowed(mm), np.minimum(in_row(Gm), INF), INF)
    for s in range(1, maxm + 1):
        i = np.maximum(mm - s, 0)
        j, ok = i[:, None] + d, allowed(i)
        h = np.minimum(Gm + sub(Qc[rows, i], j), np.concatenate([inf_col, Gm[:, :-1]], 1) + 1)
        h = np.where(ok, h, INF)
        Gn = np.where(ok, np.minimum(in_row(h), INF), INF)
        Gm = np.where((mm >= s)[:, None], Gn, Gm)
    assert (Gm.min(1)[fin] == D[fin]).all(), "the model's two passes disagree on D"
    ks = W - 1 - (Gm[:, ::-1] == D[:, None]).argmax(1)  # the largest j in A(0) with G[0][j] = D
    tstart = Pc - band + ks
    good = fin & (D <= max_dist)
    assert ((tstart <= tend) & (tstart >= 0) & (tend <= n))[good].all()
    dist[idx] = np.where(good, D, NONE)
    ts[idx], te[idx] = np.where(good, tstart, 0), np.where(good, tend, 0)
    info["D"][idx] = D
    info["ends"][idx] = np.where(fin, (F == D[:, None]).sum(1), 0)
    info["starts"][idx] = np.where(fin, (Gm == D[:, None]).sum(1), 0)
    return dist, ts, te, info


def plain(t, sigma, q, P, band):
    """The contract cell by cell for one candidate: (D, tstart, tend), or None."""
    n, m = len(t), len(q)

    def A(i):
        return range(max(0, i + P - band), min(n, i + P + band) + 1)
    F = {}
    for i in range(m + 1):
        for j in A(i):
            if i == 0:
                F[i, j] = 0
                continue
            c = []
            if (i - 1, j - 1) in F:
                c.append(F[i - 1, j - 1] + int(q[i - 1] != t[j - 1] or q[i - 1] >= sigma))
            if (i - 1, j) in F:
                c.append(F[i - 1, j] + 1)
            if (i, j - 1) in F:
                c.append(F[i, j - 1] + 1)
            if c:
                F[i, j] = min(c)
    last = [(F[m, j], j) for j in A(m) if (m, j) in F]
    if not last:
        return None
    D, tend = min(last)
    Gd = {(m, tend): 0}
    for i in range(m, -1, -1):
        for j in reversed(A(i)):
            c = [Gd[i, j]] if (i, j) in Gd else []
            if (i + 1, j + 1) in Gd:
                c.append(Gd[i + 1, j + 1] + int(q[i] != t[j] or q[i] >= sigma))
            if (i + 1, j) in Gd:
                c.append(Gd[i + 1, j] + 1)
            if (i, j + 1) in Gd:
                c.append(Gd[i, j + 1] + 1)
            if c:
                Gd[i, j] = min(c)
    first = [j for j in A(0) if Gd.get((0, j)) == D]
    assert first and min(Gd[0, j] for j in A(0) if (0, j) in Gd) == D
    return D, max(first), tend


def check_model(case, seed=0):
    """model() against plain() on reads of up to 20 symbols."""
    t = list(case.enc)
    for band, K in CONFIGS:
        reads, nc, pos = make_batch(case, 40, K, band, lens=(0, 1, 2, 5, 9, 20), mmax=20, seed=seed)
        dist, ts, te, info = model(case, reads, nc, pos, K, band, ANY)
        for c in np.flatnonzero(info["used"]):
            want = plain(t, case.sigma, list(encode(case.table, reads[c // K])), int(pos.reshape(-1)[c]), band)
            got = None if dist[c] == NONE else (int(dist[c]), int(ts[c]), int(te[c]))
            assert got == want, (band, K, int(c), got, want)


def compare(what, got, exp):
    """Every slot of (dist, tstart, tend) against the model."""
    for name, g, e in zip(("dist", "tstart", "tend"), got, exp):
        g = np.asarray(g).astype(np.int64).reshape(-1)
        e = np.asarray(e).reshape(-1)
        assert g.shape == e.shape, f"{what}: {name} has {g.shape} slots, expected {e.shape}"
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (f"{what}: {name} differ at {bad.size} slots, first {bad[:4].tolist()}: "
                               f"{g[bad[:4]].tolist()} expected {e[bad[:4]].tolist()}")


# ------------------------------------------------------- the synthetic batches

def _read(case, rng, s, m, edits):
    """m symbols cut from the text at s (fewer at its end) with `edits` planted
    substitutions, insertions and deletions, brought back to m symbols."""
    t = case.text
    q = bytearray(t[s:s + m])
    for _ in range(edits):
        if not q:
            break
        at, kind = int(rng.integers(len(q))), int(rng.integers(3))
        if kind == 0:
            q[at] = case.other(rng, q[at])
        elif kind == 1:
            q.insert(at, int(rng.choice(np.frombuffer(case.chars, np.uint8))))
        else:
            del q[at]
    q = q[:m]
    q += t[s + m:s + m + (m - len(q))]
    return bytes(q)


def make_batch(case, n, K, band, lens=SHORT, mmax=70, seed=0):
    """(reads, ncands uint32[n], pos int64[n, K]): n reads with candidates.
    Read i has length lens[i] for the first reads, then 20..mmax; i % 16 picks
    its class: the edge positions, the read without similarity, the tie read,
    else a cut with i % 5 edits at a shift cycling through -band-1 .. band+1."""
    rng = np.random.default_rng(seed * 7919 + n * 131 + K * 17 + band)
    nT = len(case.text)
    shifts = list(range(-band - 1, band + 2))
    reads, nc, pos = [], np.zeros(n, np.uint32), np.full((n, K), JUNK, np.int64)
    for i in range(n):
        m = lens[i] if n > 1 and i < len(lens) else int(rng.integers(min(20, mmax), mmax + 1))
        kind = i % 16 if n > 1 else 6
        s = int(rng.integers(0, nT - m + 1))
        edits = i % 5
        if kind in (0, 1):
            s = 0
        elif kind in (2, 4):
            s = nT - m
        first = s + shifts[i % len(shifts)]
        if kind == 0:
            first = -band  # P < 0, P + band >= 0 (band 0: P = 0)
        elif kind == 1:
            first = -band - 3  # P + band < 0: the early rows have no allowed cell
        elif kind == 2:
            first = s + min(band, 2)  # P + m > n
        elif kind == 3:
            first = nT + band + 1  # P - band > n
        elif kind == 4:
            first, edits = s, 1  # P = n - m exactly
        q = _read(case, rng, s, m, edits)
        if kind == 5:
            q = bytes([ABSENT]) * m  # no similarity to the text
        elif kind == 6 and m >= 2:  # first and last symbol substituted: ends and starts tie
            q = bytearray(case.text[s:s + m])
            q[0], q[-1] = case.other(rng, q[0]), case.other(rng, q[-1])
            q, first = bytes(q), s
        reads.append(q)
        nc[i] = (1, K, 1, 0, 1, K + 1, 1, 1)[i % 8] if kind > 6 else max(1, (1, K, K + 1)[i % 3])
        p = [first] + [s + shifts[(i + 3 * k) % len(shifts)] for k in range(1, K)]
        pos[i, :min(int(nc[i]), K)] = p[:min(int(nc[i]), K)]
    return reads, nc, pos


def length_batch(case, band, K=4):
    """Reads of every length of LENGTHS, one of 300 symbols, and one of 65,536
    (a text substring repeated), which gives NONE; two candidates each."""
    rng = np.random.default_rng(band + 99)
    nT = len(case.text)
    reads, nc, pos = [], [], []
    for i, m in enumerate(LENGTHS + (300,)):
        s = int(rng.integers(0, nT - m + 1))
        reads.append(_read(case, rng, s, m, i % 4))
        nc.append(2)
        pos.append([s, s + (band if i % 2 else -band), JUNK, JUNK][:K])
    reads.append((case.text[:256] * 256)[:MAX_LEN + 1])
    nc.append(2)
    pos.append([0, 7, JUNK, JUNK][:K])
    return reads, np.array(nc, np.uint32), np.array(pos, np.int64)


def assert_classes(case, band, K, max_dist, nc, pos, exp):
    """On the inputs and the model's values alone: a batch of 255 reads or more
    holds every class its band can (one diagonal has no indels and no ties)."""
    dist, ts, te, info = exp
    n, used, D, m = len(case.enc), info["used"], info["D"], info["m"]
    good = used & (dist != NONE)
    P = np.asarray(pos, np.int64).reshape(-1)
    got = dict(zero=(good & (dist == 0)).any(), by_max_dist=(used & (D < INF) & (D > max_dist)).any(),
               by_infinity=(used & (D >= INF) & (m <= MAX_LEN)).any(), negative=(used & (P < 0)).any(),
               negative_good=(good & (P < 0)).any() or band == 0, unused=(~used).any(),
               above=(np.asarray(nc) > K).any())
    if band:
        got.update(indel=(good & (dist > 0) & (te - ts != m)).any(), late_end=(good & (te > n - band)).any(),
                   ties=(good & (info["ends"] >= 2) & (info["starts"] >= 2)).any())
    assert all(got.values()), f"case classes missing from the batch: {got}"


def d_star(info):
    """A max_dist equal to one candidate's D, above another's and below a
    third's (the second smallest positive D: 2 wherever the tie reads are)."""
    Ds = np.unique(info["D"][info["used"] & (info["D"] < INF) & (info["D"] > 0)])
    assert Ds.size >= 3
    return int(Ds[1])


# -------------------------------------------------------------------- the runs

def run_verify(pkg, dev, ix, reads, nc, pos, K, band, max_dist, reversed=False, strands="forward"):
    """fmx_verify_async over device buffers, outputs prefilled with -1:
    (dist, tstart, tend)."""
    q = [p[::-1] for p in reads] if reversed else reads
    data, offsets = pkg.pack_patterns(q)
    nv = len(nc)
    ins = [dev.put(a) for a in (np.concatenate([data, np.zeros(1, np.uint8)]), offsets, np.asarray(nc, np.uint32),
                                np.asarray(pos, np.int64).reshape(-1))]
    outs = [dev.put(np.full(max(nv * K, 1), -1, dt)) for dt in (np.int32, np.int64, np.int64)]
    dev.sync()
    ix.verify_async(ins[0][1], ins[1][1], len(reads), ins[2][1], ins[3][1], *[p for _, p in outs], max_cands=K,
                    band=band, max_dist=max_dist, reversed=reversed, strands=strands)
    ix.sync()
    return [dev.get(h, dt)[:nv * K] for (h, _), dt in zip(outs, (np.uint32, np.int64, np.int64))]


def text_index(pkg, O, case, pb, planes, vb, options=1 | VERIFY_TEXT):
    return open_index(pkg, O, case, pb, planes, vb, options)


# ------------------------------------------------------------------ the cases

def synthetic(pkg, dev, ix, case, n):
    """Every CONFIGS class over a batch of n reads: max_dist = 0, 2, a
    candidate's D, one less and no limit for the small batches, the D for the
    large ones (their classes asserted)."""
    for band, K in CONFIGS:
        reads, nc, pos = make_batch(case, n, K, band)
        free = model(case, reads, nc, pos, K, band, ANY)
        if n >= 255:
            mds = (d_star(free[3]),)
            assert_classes(case, band, K, mds[0], nc, pos, model(case, reads, nc, pos, K, band, mds[0]))
        else:
            fin = free[3]["D"][free[3]["used"] & (free[3]["D"] < INF)]
            ds = int(fin.max()) if fin.size else 1
            mds = (0, 2, ds, max(ds, 1) - 1, ANY)
        for md in mds:
            exp = model(case, reads, nc, pos, K, band, md)
            got = run_verify(pkg, dev, ix, reads, nc, pos, K, band, md, reversed=(n + band) % 2 == 1)
            compare(f"verify n={n} band={band} max_cands={K} max_dist={md}", got, exp[:3])


def lengths(pkg, dev, ix, case):
    """Read lengths around the 64-symbol chunk, 300 and 65,536, every band."""
    for band in (0, 1, 8, 31):
        reads, nc, pos = length_batch(case, band)
        exp = model(case, reads, nc, pos, 4, band, ANY)
        assert exp[0][-4] == NONE and exp[0][-3] == NONE and (exp[0][:-4].reshape(-1, 4)[:, 0] != NONE).all()
        for rev in (False, True):
            got = run_verify(pkg, dev, ix, reads, nc, pos, 4, band, ANY, reversed=rev)
            compare(f"verify lengths band={band} rev={rev}", got, exp[:3])


def strand_flags(pkg, dev, ix, case, n=65):
    """FMX_PATTERN_REVCOMP and FMX_BOTH_STRANDS, an involution and a 3-cycle:
    the strand call equals the flag-less call on the expanded batch, and the
    model over it.  Odd reads are the rc of a cut: strand 1 truly aligns."""
    band, K = 8, 4
    cuts, nc, pos = make_batch(case, n, K, band, seed=5)
    for cmap in (involution(case), cycle_map(case)):
        ix.set_complement(cmap)
        reads = [c if i % 2 == 0 else unrc(c, cmap) for i, c in enumerate(cuts)]
        for strands, per in (("both", 2), ("reverse", 1)):
            flat = expand(reads, cmap, strands)
            nc2, pos2 = np.repeat(nc, per), np.repeat(pos, per, axis=0)
            exp = model(case, flat, nc2, pos2, K, band, 3)
            good = (exp[0] != NONE) & exp[3]["used"]
            # (strand 1 of the odd reads: rows 3, 7, ... of 2n, rows 1, 3, ... of n)
            assert good.reshape(-1, K)[2 * per - 1::2 * per].any() and good.sum() >= n // 4, "no strand-1 alignment"
            for rev in (False, True):
                got = run_verify(pkg, dev, ix, reads, nc2, pos2, K, band, 3, reversed=rev, strands=strands)
                compare(f"verify strands={strands} rev={rev}", got, exp[:3])
                alone = run_verify(pkg, dev, ix, flat, nc2, pos2, K, band, 3, reversed=rev)
                assert all(np.array_equal(a, b) for a, b in zip(got, alone))
    ix.set_complement(None)


MAP = dict(align_band=8, max_dist=6)


def map_expected(case, orc, pats, skip, band, align_band, max_dist, **over):
    """The model applied to place_expected's candidates: (place's five, then
    dist, tstart, tend)."""
    exp = V.place_expected(case, orc, pats, skip, band, **over)
    K = exp[2].shape[1]
    return exp, model(case, pats, exp[0], exp[2], K, align_band, max_dist)


def check_map(ix, orc, case, pats, skip, band, reversed=False, align_band=8, max_dist=6, **over):
    """map_batch of `pats` against the model, its first five arrays against
    place_batch; returns (expected place, expected verify, got)."""
    exp, ver = map_expected(case, orc, pats, skip, band, align_band, max_dist, **over)
    q = [p[::-1] for p in pats] if reversed else pats
    kw = dict(V.PLACE, **over)
    got = ix.map_batch(q, skip=skip, band=band, reversed=reversed, align_band=align_band, max_dist=max_dist, **kw)
    what = f"map n={len(pats)} skip={skip} band={band} rev={reversed}"
    assert got[5].dtype == np.uint32 and got[6].dtype == np.int64 and got[7].shape == exp[2].shape
    V.compare(what, got[:5], exp)
    compare(what, got[5:], ver[:3])
    place = ix.place_batch(q, skip=skip, band=band, reversed=reversed, **kw)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got[:5], place))
    return exp, ver, got


def map_runs(pkg, O, pb, planes, vb, sizes, runs=V.PLACE_RUNS, options=1 | VERIFY_TEXT):
    case = case_for(3, k=3, sr=2)
    ix, orc = text_index(pkg, O, case, pb, planes, vb, options)
    for n in sizes:
        pats = batch(case, n)
        for skip, band, rev in runs:
            exp, ver, _ = check_map(ix, orc, case, pats, skip, band, rev)
            if n >= 255:
                good = ver[3]["used"] & (ver[0] != NONE)
                assert (good & (ver[0] == 0)).sum() >= 20 and (good & (ver[0] > 0)).any()
    ix.close()


def map_both_strands(pkg, O, sizes):
    case = case_for(3, k=3, sr=2)
    ix, orc = text_index(pkg, O, case, 4, 3, 64)
    cmap = involution(case)
    ix.set_complement(cmap)
    for n in sizes:
        reads = batch(case, n)
        flat = expand(reads, cmap, "both")
        exp, ver = map_expected(case, orc, flat, 1, 8, **MAP)
        both = ix.map_batch(reads, skip=1, band=8, strands="both", **MAP, **V.PLACE)
        assert both[0].shape == (2 * n,)
        V.compare("map both strands", both[:5], exp)
        compare("map both strands", both[5:], ver[:3])
        alone = ix.map_batch(flat, skip=1, band=8, **MAP, **V.PLACE)
        assert all(np.array_equal(a, b) for a, b in zip(both, alone))
    one = ix.map(reads[3], strands="both")
    assert one == (ix.map(reads[3]), ix.map(expand(reads[3:4], cmap, "reverse")[0]))
    ix.close()


def map_chunks(pkg, O, monkeypatch, n):
    """FMX_PLACE_CHUNK=100 (read at load): the results those of one chunk."""
    case = case_for(3, k=3, sr=2)
    pats = batch(case, n)
    ix, orc = text_index(pkg, O, case, 4, 3, 64)
    whole = ix.map_batch(pats, skip=1, band=8, **MAP, **V.PLACE)
    ix.close()
    monkeypatch.setenv("FMX_PLACE_CHUNK", "100")
    ix, orc = text_index(pkg, O, case, 4, 3, 64)
    check_map(ix, orc, case, pats, 1, 8)
    parts = ix.map_batch(pats, skip=1, band=8, **MAP, **V.PLACE)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    assert [a.shape for a in ix.map_batch([])] == [(0,), (0,)] + [(0, 4)] * 6
    ix.close()


def planted_reads(case, n=256, m=60, seed=12):
    """n reads of m symbols cut from the text, 2 substitutions and one
    insertion or deletion each."""
    rng = np.random.default_rng(seed)
    reads = []
    for s in rng.integers(0, len(case.text) - m - 1, size=n):
        q = bytearray(case.text[int(s):int(s) + m + 1])
        at = sorted(int(x) for x in rng.choice(np.arange(1, m - 1), size=3, replace=False))
        q[at[0]], q[at[2]] = case.other(rng, q[at[0]]), case.other(rng, q[at[2]])
        if rng.integers(2):
            q.insert(at[1], int(rng.choice(np.frombuffer(case.chars, np.uint8))))
            q = q[:m]
        else:
            del q[at[1]]
        assert len(q) == m
        reads.append(bytes(q))
    return reads


def planted(pkg, O, layouts):
    """On the model alone: every planted read has a candidate with D <= 3; the
    device equals the model."""
    case = case_for(3, k=3, sr=2)
    reads = planted_reads(case)
    for pb, planes, vb in layouts:
        ix, orc = text_index(pkg, O, case, pb, planes, vb)
        exp, ver, got = check_map(ix, orc, case, reads, 1, 8, align_band=8, max_dist=ANY, **V.PLANTED)
        d = np.where(ver[3]["used"], ver[3]["D"], INF).reshape(len(reads), -1).min(1)
        assert (d <= 3).all() and (d > 0).any(), "the model does not verify every planted read"
        first = ix.map(reads[0], skip=1, band=8, **V.PLANTED)
        assert first[0][3:] == (None if ver[0][0] == NONE else int(ver[0][0]), int(ver[1][0]), int(ver[2][0]))
        ix.close()


def load_option(pkg, O, dev, case, pb, planes, vb):
    """options 1 | 64 against options 1: the bit, the bytes, the same answers
    from every search; 63 | 64 and 8 verify the same values; 1: FMX_E_ARG."""
    blob = case.blob(O, pb, planes, vb)
    orc = O.OracleIndex(blob, O.layout(pb, planes, vb, 0))
    load = lambda o: pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=o)  # noqa: E731
    plain_ix, text_ix = load(1), load(1 | VERIFY_TEXT)
    a, b = plain_ix.info(), text_ix.info()
    assert a["options"] == 1 and b["options"] == 1 | VERIFY_TEXT
    assert b["device_bytes"] == a["device_bytes"] + len(case.text) + 16
    skip = ("options", "device_bytes")
    assert {k: v for k, v in a.items() if k not in skip} == {k: v for k, v in b.items() if k not in skip}
    pats = batch(case, 257)
    full = [p for p in pats if p]
    same = lambda x, y: all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(x, y))  # noqa: E731
    assert np.array_equal(plain_ix.count_batch(full), text_ix.count_batch(full))
    assert same(plain_ix.locate_batch(full), text_ix.locate_batch(full))
    assert same(plain_ix.match_batch(pats), text_ix.match_batch(pats))
    assert same(plain_ix.seeds_batch(pats, max_occ=16), text_ix.seeds_batch(pats, max_occ=16))
    assert same(plain_ix.place_batch(pats, skip=1, band=8, **V.PLACE), text_ix.place_batch(pats, skip=1, band=8, **V.PLACE))
    reads, nc, pos = make_batch(case, 65, 4, 8, seed=9)
    exp = model(case, reads, nc, pos, 4, 8, 3)
    ref = run_verify(pkg, dev, text_ix, reads, nc, pos, 4, 8, 3)
    compare("verify options 65", ref, exp[:3])
    mapped = text_ix.map_batch(pats, skip=1, band=8, **MAP, **V.PLACE)
    for o, bit in ((63 | VERIFY_TEXT, VERIFY_TEXT), (8, 0)):
        ix = load(o)
        assert ix.info()["options"] & VERIFY_TEXT == bit
        assert same(run_verify(pkg, dev, ix, reads, nc, pos, 4, 8, 3), ref)
        assert same(ix.map_batch(pats, skip=1, band=8, **MAP, **V.PLACE), mapped)
        ix.close()
    with pytest.raises(pkg.FmxError) as e:
        run_verify(pkg, dev, plain_ix, reads, nc, pos, 4, 8, 3)
    assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        plain_ix.map_batch(pats)
    assert e.value.code == pkg._native.FMX_E_ARG
    plain_ix.close()
    text_ix.close()
    return orc


def still_grouped(pkg, O, monkeypatch, mem_cls):
    """Under FMX_GROUPED=1 a locate on an index loaded with 1 | 64 is a grouped
    launch (run_locate checks launches_grouped, guards and locations): the
    index still counts as the faithful one."""
    pb, planes, vb, letters = G.LAYOUTS[0]
    case = G.case_for(letters)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, 1 | VERIFY_TEXT, "grouped")
    info = ix.info()
    assert info["options"] == 1 | VERIFY_TEXT and info["group_key_len"] > 0
    assert G.run_locate(pkg, ix, mem_cls, case, orc, pb, "grouped", "single", 257, "total", 0, False)
    ix.close()


def check_arguments(pkg, dev, ix, case):
    """One small launch under the timer, n = 0, and every FMX_E_ARG of
    fmx_verify_async."""
    n, K, band = 5, 4, 8
    reads, nc, pos = make_batch(case, n, K, band)
    exp = model(case, reads, nc, pos, K, band, ANY)
    data, offsets = pkg.pack_patterns(reads)
    ins = [dev.put(a) for a in (np.concatenate([data, np.zeros(1, np.uint8)]), offsets, nc, pos.reshape(-1))]
    outs = [dev.put(np.full(n * K, -1, dt)) for dt in (np.int32, np.int64, np.int64)]
    names = ("d_bytes", "d_offsets", "d_ncands", "d_pos", "d_dist", "d_tstart", "d_tend")
    base = dict(zip(names, [p for _, p in ins + outs]), n=n, max_cands=K, band=band)
    dev.sync()
    ix.timing_enable(True)
    ix.verify_async(**base)
    ix.verify_async(**dict(base, n=0))
    ix.verify_async(**dict(dict.fromkeys(names, 0), n=0, max_cands=K, band=band))
    ix.sync()
    t = ix.timing_read()["verify"]
    assert t["launches"] == 1 and t["units"] == n * K
    ix.timing_enable(False)
    got = [dev.get(h, dt) for (h, _), dt in zip(outs, (np.uint32, np.int64, np.int64))]
    compare("verify under the timer", got, exp[:3])
    # the hints are accepted and ignored: a wrong fixed length among them
    ix.verify_async(**dict(base, long_patterns=True, stage_kb=3, fixed_len=7))
    ix.sync()
    compare("verify with hints", [dev.get(h, dt) for (h, _), dt in zip(outs, (np.uint32, np.int64, np.int64))], exp[:3])
    bad = [dict(band=32), dict(max_cands=0), dict(max_cands=17), dict(strands="reverse"), dict(strands="both")]
    bad += [{k: 0} for k in names]
    bad += [{k: base[k] + (2 if k in ("d_ncands", "d_dist") else 4)} for k in names if k != "d_bytes"]
    bad += [dict(n=4 * 0x7FFFFFFF // K + 1), dict(n=1 << 63, strands="both")]
    for over in bad:
        with pytest.raises(pkg.FmxError) as e:
            ix.verify_async(**dict(base, **over))
        assert e.value.code == pkg._native.FMX_E_ARG, over
    ix.set_complement(involution(case))
    flags = pkg._native.FMX_PATTERN_REVCOMP | pkg._native.FMX_BOTH_STRANDS  # both strand flags at once
    st = pkg._native.lib().fmx_verify_async(ix.handle, base["d_bytes"], base["d_offsets"], n, flags, K, base["d_ncands"],
                                           base["d_pos"], band, ANY, base["d_dist"], base["d_tstart"], base["d_tend"],
                                           None)
    assert st == pkg._native.FMX_E_ARG
    for kw in (dict(align_band=32), dict(max_cands=0), dict(max_cands=17), dict(max_seeds=33)):
        with pytest.raises(pkg.FmxError) as e:
            ix.map_batch(reads, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()


# ---------------------------------------------------------------- guard bands

def run_verify_guard(pkg, ix, mem_cls, case, n, K, band, skew):
    """Every buffer of one fmx_verify_async call carved at its exact size and
    weakest alignment (d_bytes at `skew` past a 16-B boundary, uint32 arrays 4,
    the offsets and the int64 arrays 8) out of one 0xA5-filled allocation:
    guards and inputs untouched, every output the model's."""
    reads, nc, pos = make_batch(case, n, K, band, seed=3)
    free = model(case, reads, nc, pos, K, band, ANY)
    md = d_star(free[3]) if n >= 255 else 2
    exp = model(case, reads, nc, pos, K, band, md)
    if n >= 255:
        assert_classes(case, band, K, md, nc, pos, exp)
    data, offsets = pkg.pack_patterns(reads)
    arena = Arena(mem_cls)
    c = arena.carve
    c("bytes", data.size, 1, skew, data=data)
    c("offsets", 8 * (n + 1), 8, 8, data=offsets)
    c("ncands", 4 * n, 4, 4, data=nc)
    c("pos", 8 * n * K, 8, 8, data=pos)
    c("dist", 4 * n * K, 4, 4)
    c("tstart", 8 * n * K, 8, 8)
    c("tend", 8 * n * K, 8, 8)
    arena.commit()
    p = arena.ptr
    assert p("bytes") % 16 == skew and p("offsets") % 16 == 8 and p("dist") % 16 == 4 and p("tend") % 16 == 8
    ix.verify_async(p("bytes"), p("offsets"), n, p("ncands"), p("pos"), p("dist"), p("tstart"), p("tend"), max_cands=K,
                    band=band, max_dist=md)
    ix.sync()
    arena.image()
    what = f"verify n={n} max_cands={K} band={band} skew={skew}"
    arena.check_guards_and_inputs(what)
    v = arena.view
    compare(what, [v("dist", np.uint32), v("tstart", np.int64), v("tend", np.int64)], exp[:3])


def guard(pkg, O, mem_cls, pb, planes, vb):
    case = case_for(planes)
    ix, _ = text_index(pkg, O, case, pb, planes, vb)
    for skew in SKEWS:
        band, K = CONFIGS[SKEWS.index(skew) % len(CONFIGS)]
        run_verify_guard(pkg, ix, mem_cls, case, 3, K, band, skew)
        run_verify_guard(pkg, ix, mem_cls, case, 257, 4, 8, skew)
    ix.close()
