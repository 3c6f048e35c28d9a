"""Placing reads (fmx_vote_async, fmx_place_batch): the model, the synthetic
batches, the runs and the cases' bodies that the emulator tests (test_vote_simt.py,
test_vote_guard_simt.py) and the GPU tests (test_gpu_vote.py,
test_gpu_vote_guard.py) share.

model() is the contract of include/fmx.h in plain Python over (nseeds, spans,
loc_offsets, locs): a chain's hits (d, j) sorted, a new cluster wherever the
diagonal jumps by more than band, pos / mask / cover per cluster, those with
cover >= min_cover by (cover descending, pos ascending), the first max_cands
of them.  For real reads those four arrays are _seed_cases.expected_arrays'
output, which is tied to the oracle; for the synthetic batches they are made
here, so that every edge of the kernel is hit exactly: chains of 0, 1, 2, 63,
64, 65, 127, 128, 129, 1,023, 1,024 and 1,025 hits (the last overflows), a last
chain whose offsets reach past cap, diagonals that are negative, equal, a band
and a band + 1 apart and, for u64 positions, around 2^32, chains with exactly
max_cands and max_cands + 1 clusters.  assert_classes checks on the model's
values alone that a batch holds them.
"""
import numpy as np
import pytest

from _guard_cases import Arena
from _seed_cases import BATCH_SIZES, batch, case_for, expected_arrays, open_index  # noqa: F401
from _strand_cases import expand, involution
from _util import HostDev, TorchDev  # noqa: F401

MAX_HITS, OVERFLOW, MORE = 1024, 1, 2
CHAIN_COUNTS = (1, 3, 4, 5, 255, 256, 257)
HS = (64, 1025, 65, 63, 0, 1024, 1, 2, 127, 128, 129, 1023)  # the first chains' hit counts
LENS = (3, 5, 5, 8, 12, 20)  # seed lengths: few values, so that covers tie
# (max_seeds, band, min_cover, max_cands): every max_seeds, band and max_cands of the issue; min_cover 1 keeps
# every cluster, 12 drops the clusters of one short seed, 10^6 drops all
CONFIGS = ((8, 0, 1, 4), (1, 1, 1, 1), (32, 50, 1, 16), (8, 1, 12, 16), (8, 0, 10 ** 6, 4), (32, 0, 12, 1))
# (P bytes, planes, vector bits)
LAYOUTS = [(4, 3, 64), (8, 5, 128)]


# ------------------------------------------------------------------ the model

def chain_clusters(nseeds, spans, off, locs, ms, i, band):
    """Chain i's sorted hits [(d, j)] and clusters [[pos, mask, hits]]."""
    sp = spans.reshape(-1, 2).astype(np.int64)
    hits = sorted((int(locs[x]) - int(sp[i * ms + j, 0] - sp[i * ms + j, 1]), j) for j in range(int(nseeds[i]))
                  for x in range(int(off[i * ms + j]), int(off[i * ms + j + 1])))
    cl, last = [], None
    for d, j in hits:
        if last is None or d - last > band:
            cl.append([d, 0, 0])
        cl[-1][1] |= 1 << j
        cl[-1][2] += 1
        last = d
    return hits, cl


def model(nseeds, spans, off, locs, ms, cap, band, min_cover, K):
    """(ncands, flags, pos[n, K], cover[n, K], mask[n, K], Q[n]) as int64."""
    n = len(nseeds)
    spans = np.asarray(spans)
    sp = spans.reshape(-1, 2).astype(np.int64)
    nc, fl, Q = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    pos, cov, mask = (np.zeros((n, K), np.int64) for _ in range(3))
    for i in range(n):
        a, b = int(off[i * ms]), int(off[(i + 1) * ms])
        if b - a > MAX_HITS or b > cap:
            fl[i] = OVERFLOW
            continue
        _, cl = chain_clusters(nseeds, spans, off, locs, ms, i, band)
        cands = sorted((-sum(int(sp[i * ms + j, 1]) for j in range(ms) if m >> j & 1), p, m) for p, m, _ in cl)
        cands = [c for c in cands if -c[0] >= min_cover]
        Q[i], nc[i], fl[i] = len(cands), min(len(cands), K), MORE if len(cands) > K else 0
        for k, (c, p, m) in enumerate(cands[:K]):
            pos[i, k], cov[i, k], mask[i, k] = p, -c, m
    return nc, fl, pos, cov, mask, Q


def compare(what, got, exp):
    """Every slot of (ncands, flags, pos, cover, mask) against the model."""
    for name, g, e in zip(("ncands", "flags", "pos", "cover", "mask"), got, exp):
        g = np.asarray(g).astype(np.int64).reshape(e.shape)
        bad = np.argwhere(g != e)
        assert bad.size == 0, (f"{what}: {name} differ at {len(bad)} places, first {bad[:4].tolist()}: "
                               f"{[int(g[tuple(b)]) for b in bad[:4]]} expected {[int(e[tuple(b)]) for b in bad[:4]]}")


# ------------------------------------------------------- the synthetic batches

def _seeds(rng, ns):
    """ns seeds of a read, right to left, not overlapping: [(end, length)]."""
    Ls = [int(rng.choice(LENS)) for _ in range(ns)]
    gaps = [int(rng.integers(0, 3)) for _ in range(ns)]
    e = sum(Ls) + sum(gaps) + int(rng.integers(0, 4))
    out = []
    for L, g in zip(Ls, gaps):
        out.append((e, L))
        e -= L + g
    assert e >= 0
    return out


def _chain(rng, ms, H, band, lim, base=None, clusters=None):
    """One chain of H hits: (seeds, per-seed location lists).  Its diagonals
    walk from `base` in steps of 0, 1, band, band + 1, band + 2 and 1,000;
    `clusters`: that many diagonals 1,000 + band apart instead, the first H of
    the hits one per diagonal, so that the chain has exactly that many
    clusters."""
    ns = int(rng.integers(1, ms + 1)) if H else int(rng.integers(0, ms + 1))
    seeds = _seeds(rng, ns)
    qs = [e - L for e, L in seeds]
    d0 = int(rng.integers(-3, 3000)) if base is None else base
    if clusters:
        ds = [d0 + i * (1000 + band) for i in range(clusters)]
    else:
        nd = max(1, min(H, int(rng.integers(1, 12))))
        steps = rng.choice([0, 1, band, band + 1, band + 2, 1000], size=nd)
        ds = [d0 + int(s) for s in np.concatenate([[0], np.cumsum(steps[:-1])])]
    locs = [[] for _ in range(ns)]
    for k in range(H):
        d = ds[k] if k < len(ds) else ds[int(rng.integers(len(ds)))]
        if clusters and k >= len(ds) and band and rng.integers(0, 2):
            d += band  # (exactly a band from its cluster's first diagonal: the same cluster)
        js = [j for j in range(ns) if 0 <= d + qs[j] < lim]
        if not js:  # (a negative diagonal no seed of the chain reaches, or one past the position type)
            d = max(0, min(d, lim - 1 - max(qs)))
            js = list(range(ns))
        j = js[int(rng.integers(len(js)))]
        locs[j].append(d + qs[j])
    for ll in locs:
        rng.shuffle(ll)
    return seeds, locs


def make_batch(n, ms, pb, band, K, seed=0):
    """(nseeds uint32[n], spans uint32[n, ms, 2], loc_offsets uint64[n ms + 1],
    locs P[total], cap): n chains — the hit counts of HS first, then chains of
    exactly K and K + 1 clusters, chains around 2^32, random ones, and (n >= 3)
    a last chain of 30 hits of which cap leaves room for 10."""
    rng = np.random.default_rng(seed * 7919 + n * 131 + ms * 17 + pb + band + K)
    P = np.uint32 if pb == 4 else np.uint64
    lim = 1 << 32 if pb == 4 else 1 << 40
    chains = []
    for i in range(n):
        if n >= 3 and i == n - 1:
            chains.append(_chain(rng, ms, 30, band, lim))
        elif i < len(HS):
            chains.append(_chain(rng, ms, HS[i], band, lim, base=-2 if i % 2 else None))
        elif i < len(HS) + 4:
            c = K + (i - len(HS)) % 2
            chains.append(_chain(rng, ms, c + (i - len(HS)) // 2 * 5, band, lim, base=-1, clusters=c))
        elif i < len(HS) + 8:
            # (the first hit of the third lies within 1,000 below 2^32 whatever its seed, of the fourth above it)
            chains.append(_chain(rng, ms, int(rng.integers(2, 40)), band, lim,
                                 base=(1 << 32) + (-2, -30, -802, 5)[i - len(HS) - 4]))
        else:
            chains.append(_chain(rng, ms, int(rng.choice([0, 1, 3, 8, 20, 40, 70, 200], p=[.1, .1, .2, .2, .2, .1, .05, .05])),
                                 band, lim))
    ns = np.array([len(s) for s, _ in chains], np.uint32)
    spans = np.zeros((n, ms, 2), np.uint32)
    cnt = np.zeros(n * ms, np.uint64)
    flat = []
    for i, (s, ll) in enumerate(chains):
        for j, ((e, L), x) in enumerate(zip(s, ll)):
            spans[i, j] = (e, L)
            cnt[i * ms + j] = len(x)
            flat += x
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
    locs = np.array(flat, dtype=np.uint64).astype(P)
    cap = int(off[-1])
    if n >= 3:
        cap = int(off[(n - 1) * ms]) + 10
        locs[cap:] = P(0xA5A5A5A5)  # (never written by the seeds launch this stands for, never to be read)
    return ns, spans, off, locs, cap


def assert_classes(arrays, ms, pb, band, min_cover, K, exp):
    """On the inputs and the model's outputs alone: the batch holds every class
    its size and parameters can (everything, from 255 chains on)."""
    ns, spans, off, locs, cap = arrays
    nc, fl, pos, cov, mask, Q = exp
    n = len(ns)
    H = np.diff(off[::ms].astype(np.int64))
    assert set(H.tolist()) >= set(HS[:min(n - (n >= 3), len(HS))]), "hit counts missing"
    if n >= 3:
        assert off[-1] > cap and fl[-1] == OVERFLOW and H[-1] <= MAX_HITS, "no chain past cap"
        assert (locs[cap:] == 0xA5A5A5A5).all()
    if n < 255:
        return
    over = np.flatnonzero(fl == OVERFLOW)
    assert 1 in over and H[1] == 1025 and len(over) == 2
    info = dict(neg=0, same_d_seeds=0, same_d_seed=0, twice=0, gap_band=0, gap_band1=0, dropped=0, ties=0)
    for i in range(n):
        if fl[i] == OVERFLOW:
            continue
        hits, cl = chain_clusters(ns, spans, off, locs, ms, i, band)
        d = np.array([h[0] for h in hits], np.int64)
        j = np.array([h[1] for h in hits], np.int64)
        if len(d) > 1:
            same = np.diff(d) == 0
            info["same_d_seeds"] += int((same & (np.diff(j) != 0)).any())
            info["same_d_seed"] += int((same & (np.diff(j) == 0)).any())
            info["gap_band"] += int((np.diff(d) == band).any())
            info["gap_band1"] += int((np.diff(d) == band + 1).any())
        info["twice"] += int(any(h > bin(m).count("1") for _, m, h in cl))
        info["neg"] += int((pos[i, :nc[i]] < 0).any())
        info["dropped"] += int(0 < Q[i] < len(cl))
        info["ties"] += int((np.diff(cov[i, :nc[i]]) == 0).any())
    must = ["same_d_seed", "twice", "gap_band", "gap_band1"] + (["same_d_seeds"] if ms > 1 else [])
    if min_cover == 1:
        must += ["neg"] + (["ties"] if K > 1 else [])
        exact = (Q == K) & (fl == 0)
        assert exact.sum() >= 2 and ((fl == MORE) & (Q == K + 1)).sum() >= 2, "no chain with exactly K / K + 1 clusters"
        # an overflowing chain's neighbours in its workgroup have candidates of their own
        assert nc[0] > 0 and nc[2] > 0 and nc[3] > 0
    elif min_cover <= 20:
        must += ["dropped"]
    else:
        assert (nc == 0).all() and (H[fl == 0] > 0).any()
    assert all(info[k] for k in must), f"case classes missing from the batch: {info}"
    if pb == 8:
        assert (locs[:cap] >= 1 << 32).any() and ((locs[:cap] < 1 << 32) & (locs[:cap] >= (1 << 32) - 1000)).any()


def vote_device(dev, ix, n, ms, d_ns, d_spans, d_off, d_locs, cap, band, min_cover, K):
    """fmx_vote_async over device pointers into outputs prefilled with -1;
    returns (ncands, flags, pos, cover, mask)."""
    outs = [dev.put(np.full(max(n, 1) * w, -1, dt)) for w, dt in ((1, np.int32), (1, np.int32), (K, np.int64),
                                                                  (K, np.int32), (K, np.int32))]
    dev.sync()
    ix.vote_async(n, ms, d_ns, d_spans, d_off, d_locs, cap, *[p for _, p in outs], band=band, min_cover=min_cover,
                  max_cands=K)
    ix.sync()
    got = [dev.get(h, dt) for (h, _), dt in zip(outs, (np.uint32, np.uint32, np.int64, np.uint32, np.uint32))]
    return [g[:n * w] for g, w in zip(got, (1, 1, K, K, K))]


def run_vote(dev, ix, arrays, ms, band, min_cover, K):
    ns, spans, off, locs, cap = arrays
    ins = [dev.put(a) for a in (ns, spans, off, locs)]
    return vote_device(dev, ix, len(ns), ms, *[p for _, p in ins], cap, band, min_cover, K)


# --------------------------------------------------------------- the pipeline

PLACE = dict(max_seeds=8, min_len=1, max_occ=16, min_cover=3, max_cands=4)
# (skip, band, reversed)
PLACE_RUNS = ((0, 0, False), (1, 8, True), (1, 0, False), (0, 8, True))


def place_expected(case, orc, pats, skip, band, **over):
    """The model over _seed_cases.expected_arrays of the same batch."""
    kw = dict(PLACE, **over)
    ns, _, spans, _, off, locs = expected_arrays(case, orc, pats, kw["max_seeds"], kw["min_len"], skip, kw["max_occ"])
    assert np.diff(off[::kw["max_seeds"]].astype(np.int64)).max() <= kw["max_seeds"] * kw["max_occ"]
    return model(ns, spans, off, locs, kw["max_seeds"], int(off[-1]), band, kw["min_cover"], kw["max_cands"])


def check_place(ix, orc, case, pats, skip, band, reversed=False, **over):
    """place_batch of `pats` against the model; returns (expected, got)."""
    exp = place_expected(case, orc, pats, skip, band, **over)
    q = [p[::-1] for p in pats] if reversed else pats
    got = ix.place_batch(q, skip=skip, band=band, reversed=reversed, **dict(PLACE, **over))
    assert got[0].dtype == np.uint32 and got[2].dtype == np.int64 and got[2].shape == (len(pats), exp[2].shape[1])
    compare(f"place n={len(pats)} skip={skip} band={band} rev={reversed}", got, exp)
    return exp, got


def place_device(dev, pkg, ix, pb, pats, skip, band, **over):
    """What place_batch composes, run by the caller on buffers of its own:
    seeds_batch_async with locations, then vote_async over the very buffers it
    wrote, on the same stream with nothing in between."""
    kw = dict(PLACE, **over)
    ms, n = kw["max_seeds"], len(pats)
    P = np.uint32 if pb == 4 else np.uint64
    S, cap = n * ms, n * ms * kw["max_occ"]
    data, offsets = pkg.pack_patterns(pats)
    wsb = ix.locate_workspace_size(S)
    bufs = [dev.put(a) for a in (np.concatenate([data, np.zeros(1, np.uint8)]), offsets, np.zeros(n, np.uint32),
                                 np.zeros(n, np.uint32), np.zeros(2 * S, np.uint32), np.zeros(2 * S, P),
                                 np.zeros(S + 1, np.uint64), np.zeros(max(cap, 1), P), np.zeros(1, np.uint64),
                                 np.zeros(wsb + 256, np.uint8))]
    p = [q for _, q in bufs]
    ws = p[9] + (-p[9]) % 256
    dev.sync()
    ix.seeds_batch_async(p[0], p[1], n, p[2], p[3], p[4], p[5], p[6], p[7], cap, p[8], ws, wsb, max_seeds=ms,
                         min_len=kw["min_len"], skip=skip, max_occ=kw["max_occ"])
    return vote_device(dev, ix, n, ms, p[2], p[4], p[6], p[7], cap, band, kw["min_cover"], kw["max_cands"])


def planted_reads(case, n=256, m=60, subs=2, seed=11):
    """n reads of m symbols cut from the text, `subs` substitutions each, and
    where each was cut."""
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, len(case.text) - m, size=n)
    reads = []
    for s in starts:
        q = bytearray(case.text[int(s):int(s) + m])
        for at in rng.choice(m, size=subs, replace=False):
            q[at] = case.other(rng, q[at])
        reads.append(bytes(q))
    return reads, starts.astype(np.int64)


PLANTED = dict(max_seeds=8, min_len=6, max_occ=16, min_cover=1, max_cands=4)


def check_planted(ix, orc, case):
    """256 reads of 60 symbols cut from the text with 2 substitutions each:
    the model's best candidate is where the read was cut, for every read
    (asserted on the model alone), and the device equals the model."""
    reads, starts = planted_reads(case)
    exp = place_expected(case, orc, reads, 1, 0, **PLANTED)
    assert (exp[0] >= 1).all() and np.array_equal(exp[2][:, 0], starts), "the model does not place every planted read"
    assert (exp[3][:, 0] >= 40).all()  # (58 symbols survive, the seeds leave out those next to a substitution)
    got = ix.place_batch(reads, skip=1, band=0, **PLANTED)
    compare("planted reads", got, exp)
    assert ix.place(reads[0], skip=1, **PLANTED)[0][0] == int(starts[0])


def check_limits(pkg, ix, pats):
    """max_seeds * max_occ up to FMX_VOTE_MAX_HITS, and no further."""
    for ms, occ, ok in ((8, 128, True), (8, 129, False), (1, 1024, True), (1, 1025, False), (32, 32, True),
                        (32, 33, False)):
        if ok:
            ix.place_batch(pats, max_seeds=ms, max_occ=occ)
        else:
            with pytest.raises(pkg.FmxError) as e:
                ix.place_batch(pats, max_seeds=ms, max_occ=occ)
            assert e.value.code == pkg._native.FMX_E_ARG
    for kw in (dict(max_seeds=0), dict(max_seeds=33), dict(max_cands=0), dict(max_cands=17)):
        with pytest.raises(pkg.FmxError) as e:
            ix.place_batch(pats, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    assert [a.shape for a in ix.place_batch([])] == [(0,), (0,), (0, 4), (0, 4), (0, 4)]


def check_arguments(pkg, dev, ix, pb):
    """One small launch under the timer, n_chains = 0, and every FMX_E_ARG of
    fmx_vote_async."""
    n, ms, K = 5, 8, 4
    arrays = make_batch(n, ms, pb, 0, K)
    ns, spans, off, locs, cap = arrays
    exp = model(ns, spans, off, locs, ms, cap, 0, 1, K)
    ins = [dev.put(a) for a in (ns, spans, off, locs)]
    outs = [dev.put(np.full(n * w, -1, dt)) for w, dt in ((1, np.int32), (1, np.int32), (K, np.int64), (K, np.int32),
                                                          (K, np.int32))]
    names = ("d_nseeds", "d_spans", "d_loc_offsets", "d_locs", "d_ncands", "d_flags", "d_pos", "d_cover", "d_mask")
    base = dict(zip(names, [p for _, p in ins + outs]), n_chains=n, max_seeds=ms, cap=cap, max_cands=K)
    dev.sync()
    ix.timing_enable(True)
    ix.vote_async(**base)
    ix.vote_async(**dict(base, n_chains=0))
    ix.vote_async(**dict(dict.fromkeys(names, 0), n_chains=0, max_seeds=ms, cap=0, max_cands=K))
    ix.sync()
    t = ix.timing_read()["vote"]
    assert t["launches"] == 1 and t["units"] == n
    ix.timing_enable(False)
    got = [dev.get(h, dt) for (h, _), dt in zip(outs, (np.uint32, np.uint32, np.int64, np.uint32, np.uint32))]
    compare("vote under the timer", got, exp)
    bad = [dict(max_seeds=0), dict(max_seeds=33), dict(max_cands=0), dict(max_cands=17)]
    bad += [{k: 0} for k in names]
    bad += [{k: base[k] + (4 if k in ("d_loc_offsets", "d_pos") else 2)} for k in names if k != "d_locs"]
    bad += [dict(d_locs=base["d_locs"] + pb // 2)]
    for over in bad:
        with pytest.raises(pkg.FmxError) as e:
            ix.vote_async(**dict(base, **over))
        assert e.value.code == pkg._native.FMX_E_ARG, over
    ix.vote_async(**dict(base, d_locs=0, cap=0))  # (d_locs may be null when cap = 0: every chain with a hit overflows)
    ix.sync()
    got = [dev.get(h, dt) for (h, _), dt in zip(outs[:2], (np.uint32, np.uint32))]
    assert (got[0] == 0).all() and np.array_equal(got[1], np.where(off[ms::ms] > 0, OVERFLOW, 0))
    ix.close()


# ------------------------------------------------------------------ the cases

def synthetic(dev, ix, n, pb):
    """Every CONFIGS class over a batch of n synthetic chains."""
    for ms, band, mc, K in CONFIGS:
        arrays = make_batch(n, ms, pb, band, K)
        exp = model(*arrays[:4], ms, arrays[4], band, mc, K)
        assert_classes(arrays, ms, pb, band, mc, K, exp)
        got = run_vote(dev, ix, arrays, ms, band, mc, K)
        compare(f"vote n={n} max_seeds={ms} band={band} min_cover={mc} max_cands={K}", got, exp)


def place_runs(dev, pkg, ix, orc, case, pb, n, runs):
    """place_batch against the model, and against seeds_batch_async +
    vote_async run here on buffers of the test's own."""
    pats = batch(case, n)
    for skip, band, rev in runs:
        exp, got = check_place(ix, orc, case, pats, skip, band, rev)
        if n >= 255:
            assert (exp[0] > 1).sum() >= 20 and (exp[0] == 0).sum() >= 2 and (exp[5] > exp[0]).sum() >= 1
        if not rev:
            dgot = place_device(dev, pkg, ix, pb, pats, skip, band)
            compare("seeds_batch_async + vote_async", dgot, exp)


def two_letters(pkg, O, sizes):
    """A two-letter text: most seeds have more than max_occ occurrences and
    bring none, the others bring up to 16 each."""
    case = case_for(2, two_letters=True, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    for n in sizes:
        exp, _ = check_place(ix, orc, case, batch(case, n), 1, 8)
        assert (exp[0] > 0).sum() >= 50
        check_place(ix, orc, case, batch(case, n), 0, 0, True, max_cands=16, min_cover=1)
    ix.close()


def both_strands(pkg, O, sizes):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    cmap = involution(case)
    ix.set_complement(cmap)
    for n in sizes:
        reads = batch(case, n)
        both = ix.place_batch(reads, skip=1, band=8, strands="both", **PLACE)
        flat = ix.place_batch(expand(reads, cmap, "both"), skip=1, band=8, **PLACE)
        assert both[0].shape == (2 * n,) and all(np.array_equal(a, b) for a, b in zip(both, flat))
    assert ix.place(reads[3], strands="both") == (ix.place(reads[3]), ix.place(expand(reads[3:4], cmap, "reverse")[0]))
    ix.close()


def chunks_and_limits(pkg, O, monkeypatch):
    """FMX_PLACE_CHUNK=100 (read at load): 700 reads in seven chunks, the
    results those of one; max_seeds * max_occ = 1,024 is accepted, 1,025 is
    FMX_E_ARG."""
    case = case_for(3, k=3, sr=2)
    pats = batch(case, 700)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    whole = ix.place_batch(pats, skip=1, band=8, **PLACE)
    ix.close()
    monkeypatch.setenv("FMX_PLACE_CHUNK", "100")
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    check_place(ix, orc, case, pats, 1, 8)
    parts = ix.place_batch(pats, skip=1, band=8, **PLACE)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    check_limits(pkg, ix, pats[:40])
    ix.close()


def planted(pkg, O, layouts):
    case = case_for(3, k=3, sr=2)
    for pb, planes, vb in layouts:
        ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
        check_planted(ix, orc, case)
        ix.close()


# ---------------------------------------------------------------- guard bands

def run_vote_guard(pkg, ix, mem_cls, pb, n, ms, band, min_cover, K):
    """Every buffer of one fmx_vote_async call carved at its exact size and
    weakest alignment (uint32 arrays 4 B past a 16-B boundary, the offsets and
    d_pos 8, d_locs — exactly cap entries — P) out of one 0xA5-filled
    allocation: guards and inputs untouched, every output the model's."""
    arrays = make_batch(n, ms, pb, band, K, seed=3)
    ns, spans, off, locs, cap = arrays
    exp = model(ns, spans, off, locs, ms, cap, band, min_cover, K)
    assert_classes(arrays, ms, pb, band, min_cover, K, exp)
    arena = Arena(mem_cls)
    c = arena.carve
    c("nseeds", 4 * n, 4, 4, data=ns)
    c("spans", 8 * n * ms, 4, 4, data=spans)
    c("loc_offsets", 8 * (n * ms + 1), 8, 8, data=off)
    c("locs", pb * cap, pb, pb, data=locs[:cap])
    c("ncands", 4 * n, 4, 4)
    c("flags", 4 * n, 4, 4)
    c("cover", 4 * n * K, 4, 4)
    c("mask", 4 * n * K, 4, 4)
    c("pos", 8 * n * K, 8, 8)
    arena.commit()
    p = arena.ptr
    assert p("nseeds") % 16 == 4 and p("loc_offsets") % 16 == 8 and p("locs") % 16 == pb and p("pos") % 16 == 8
    ix.vote_async(n, ms, p("nseeds"), p("spans"), p("loc_offsets"), p("locs"), cap, p("ncands"), p("flags"), p("pos"),
                  p("cover"), p("mask"), band=band, min_cover=min_cover, max_cands=K)
    ix.sync()
    arena.image()
    what = f"vote n={n} max_seeds={ms} band={band} min_cover={min_cover} max_cands={K}"
    arena.check_guards_and_inputs(what)
    v = arena.view
    compare(what, [v("ncands", np.uint32), v("flags", np.uint32), v("pos", np.int64), v("cover", np.uint32),
                   v("mask", np.uint32)], exp)
