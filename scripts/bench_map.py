#!/usr/bin/env python3
"""Time read mapping with verification (fmx_map_batch, fmx_verify_async)
against what the parent of that change already had (DESIGN.md §5,
profiles/r14/README.md).

One index (bench.py's C2 by default: 1 Gbp ACGT, u32 / Block3<u64>, k 3, sr 2,
built on the GPU from bench.py's seeded text, loaded with FMX_OPT_DEFAULT |
FMX_OPT_VERIFY_TEXT), 100,000 reads of 150 bp per call — legs s0, s1, s3: 0, 1
and 3 random substitutions; leg indel: one deletion and one insertion —, the
seeds and the vote as scripts/bench_place.py has them, max_cands = 4,
align_band = 8, max_dist = 12; the legs alternate, --runs times each:

  host buffers (wall clock around synchronous calls, --calls per run)
    map_<leg>      fmx_map_batch: reads up, candidates and alignments down;
    hostdp_<leg>   what it replaces: fmx_place_batch, then the banded alignment
                   of every candidate against a host copy of the text in NumPy,
                   vectorised over candidates and band, a loop over rows — its
                   results must equal map_batch's (asserted before anything is
                   timed);
  device buffers (device events around --launches back-to-back calls)
    seedsvote_<leg>        fmx_seeds_batch_async + fmx_vote_async: the baseline;
    seedsvoteverify_<leg>  the same followed by fmx_verify_async on their
                           buffers: what the verification adds.

The last line is one JSON object with every run, the medians and each leg's
own run-to-run spread.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, cut_patterns)

MAX_SEEDS, SKIP, MIN_LEN, BAND, MIN_COVER, MAX_CANDS = 8, 1, 12, 8, 20, 4
ALIGN_BAND, MAX_DIST = 8, 12
NONE = 0xFFFFFFFF
LEGS = ("s0", "s1", "s3", "indel")


def numpy_verify(t, reads, m, nc, pos, K, band, max_dist):
    """The contract of fmx_verify_async for reads of one length m over the
    text's symbol indices t: (dist uint32[n, K], tstart, tend int64[n, K]).
    Both recurrences a row at a time over every used candidate and the band."""
    n = t.size
    used = np.arange(K)[None, :] < np.minimum(nc, K)[:, None]
    idx = np.flatnonzero(used.reshape(-1))
    dist = np.where(used, NONE, 0).astype(np.uint32).reshape(-1)
    ts, te = np.zeros(dist.size, np.int64), np.zeros(dist.size, np.int64)
    if idx.size == 0:
        return dist.reshape(-1, K), ts.reshape(-1, K), te.reshape(-1, K)
    INF, W = np.int16(16000), 2 * band + 1
    kk = np.arange(W, dtype=np.int16)
    P = pos.reshape(-1)[idx]
    Q = reads.reshape(-1, m)[idx // K]
    d = P[:, None] - band + np.arange(W)[None, :]
    C = idx.size
    inf_col = np.full((C, 1), INF, np.int16)

    def row(i):  # (allowed cells of row i, t[j - 1] and t[j] over them)
        j = i + d
        return (j >= 0) & (j <= n), t[np.clip(j - 1, 0, n - 1)], t[np.clip(j, 0, n - 1)]

    ok, _, _ = row(0)
    F = np.where(ok, np.int16(0), INF)
    for i in range(1, m + 1):
        ok, tl, _ = row(i)
        h = np.minimum(F + (Q[:, i - 1, None] != tl), np.concatenate([F[:, 1:], inf_col], 1) + np.int16(1))
        h = np.where(ok, h, INF)
        F = np.where(ok, np.minimum(np.minimum.accumulate(h - kk, axis=1) + kk, INF), INF)
    D = F.min(1)
    kb = (F == D[:, None]).argmax(1)
    live = (D < INF) & (D <= max_dist)
    G = np.full((C, W), INF, np.int16)
    G[np.arange(C), kb] = 0

    def in_row(h):
        return np.minimum.accumulate((h + kk)[:, ::-1], axis=1)[:, ::-1] - kk

    ok, _, _ = row(m)
    G = np.where(ok, np.minimum(in_row(G), INF), INF)
    for i in range(m - 1, -1, -1):
        ok, _, tr = row(i)
        h = np.minimum(G + (Q[:, i, None] != tr), np.concatenate([inf_col, G[:, :-1]], 1) + np.int16(1))
        h = np.where(ok, h, INF)
        G = np.where(ok, np.minimum(in_row(h), INF), INF)
    ks = W - 1 - (G[:, ::-1] == D[:, None]).argmax(1)
    dist[idx] = np.where(live, D.astype(np.uint32), NONE)
    ts[idx] = np.where(live, P - band + ks, 0)
    te[idx] = np.where(live, m + P - band + kb, 0)
    return dist.reshape(-1, K), ts.reshape(-1, K), te.reshape(-1, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--text-len", type=int, default=0, help="override the config's text length")
    ap.add_argument("--patterns", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of each leg (at least 3)")
    ap.add_argument("--launches", type=int, default=50, help="timed calls per run, device-buffer legs")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per run, map_batch")
    ap.add_argument("--host-calls", type=int, default=1, help="timed calls per run, the NumPy baseline")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map.py needs a GPU (unmeasured without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = bench.CONFIGS[args.config]
    n, B, P, m, occ = args.text_len or cfg["text_len"], args.patterns, cfg["pos"], args.read_len, args.max_occ
    position = pkg.u32 if P == 4 else pkg.u64
    block = getattr(pkg.blocks, f"Block{cfg['planes']}")(pkg.Vector(cfg["vec"]))
    pdt = torch.int32 if P == 4 else torch.int64

    # bench.py's text and blob
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    A = len(cfg["alphabet"])
    alpha = torch.tensor(list(cfg["alphabet"]), dtype=torch.uint8, device=dev)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    for c0 in range(0, n, 1 << 28):
        c1 = min(n, c0 + (1 << 28))
        d_text[c0:c1] = alpha[torch.randint(0, A, (c1 - c0,), device=dev, dtype=torch.int64, generator=gen)]
    table = pkg.text_encoders.EncodingTable.from_symbols(cfg["symbols"])
    builder = (pkg.FmIndexBuilder(n, table.symbol_count(), table, position, block)
               .set_lookup_table_config(pkg.build_config.LookupTableConfig.KmerSize(cfg["k"]))
               .set_suffix_array_config(pkg.build_config.SuffixArrayConfig.Compressed(cfg["sr"])))
    blob_len = builder.blob_size()
    d_blob = torch.empty(blob_len, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    builder.build_device(d_text.data_ptr(), d_blob.data_ptr(), blob_len, device=0)
    t0 = time.perf_counter()
    ix = pkg.FmIndex.load_device(d_blob.data_ptr(), blob_len, position, block, pkg.text_encoders.EncodingTable,
                                 device=0, options=pkg._native.FMX_OPT_DEFAULT | pkg.OPT_VERIFY_TEXT)
    load_s = time.perf_counter() - t0
    info = ix.info()
    print(f"index: {cfg['desc']}; text {n:,}, options {info['options']}, record {info['occ_record']}, "
          f"device bytes {info['device_bytes']:,}, load {load_s:.2f} s", flush=True)
    # the baseline's host copy of the text, as symbol indices (the configs' symbols come in the alphabet's order)
    lut = np.zeros(256, np.uint8)
    for code, c in enumerate(cfg["alphabet"]):
        lut[c] = code
    h_text = lut[d_text.cpu().numpy()]

    pg = torch.Generator(device=dev)
    pg.manual_seed(args.seed * 1000 + 17)
    rng = np.random.default_rng(args.seed + 5)
    pad = np.zeros(64, np.uint8)
    letters = np.frombuffer(bytes(cfg["alphabet"]), np.uint8)

    def reads_of(leg):
        starts = torch.randint(0, n - m - 1, (B,), device=dev, dtype=torch.int64, generator=pg)
        r = bench.cut_patterns(torch, d_text, starts, m + 1).view(B, m + 1).cpu().numpy()
        rows = np.arange(B)
        if leg == "indel":  # symbol a deleted, a random one inserted before symbol b of what is left
            a, b = rng.integers(10, m - 10, B), rng.integers(10, m - 10, B)
            col = np.arange(m)[None, :]
            r = np.take_along_axis(r, col + (col >= a[:, None]), axis=1)
            shifted = np.take_along_axis(r, np.maximum(col - (col > b[:, None]), 0), axis=1)
            r = np.where(col == b[:, None], letters[rng.integers(0, A, B)][:, None], shifted)
        else:
            r = r[:, :m].copy()
            for _ in range(int(leg[1:])):  # another letter at a random position
                at = rng.integers(0, m, B)
                r[rows, at] = letters[(lut[r[rows, at]] + rng.integers(1, A, B)) % A]
        return np.ascontiguousarray(r).reshape(-1), starts.cpu().numpy()

    h_reads, d_reads, starts = {}, {}, {}
    for leg in LEGS:
        h_reads[leg], starts[leg] = reads_of(leg)
        d_reads[leg] = torch.from_numpy(np.concatenate([h_reads[leg], pad])).to(dev)
    h_off = (np.arange(B + 1, dtype=np.uint64) * m)
    d_off = (torch.arange(B + 1, device=dev, dtype=torch.int64) * m).contiguous()
    S, K = B * MAX_SEEDS, MAX_CANDS
    wsb = ix.locate_workspace_size(S)
    d_ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=dev)
    ws_ptr = d_ws.data_ptr() + (-d_ws.data_ptr()) % 256
    cap = S * occ
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    s_ns, s_rest, s_spans, s_rng = z(B), z(B), z((S, 2)), z((S, 2), pdt)
    s_loff, s_locs, s_need = z(S + 1, torch.int64), z(cap, pdt), z(1, torch.int64)
    v_nc, v_fl, v_pos, v_cov, v_mask = z(B), z(B), z((B, K), torch.int64), z((B, K)), z((B, K))
    a_dist, a_ts, a_te = z((B, K)), z((B, K), torch.int64), z((B, K), torch.int64)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    kb = min(56, -(-256 * m // 1024))
    torch.cuda.synchronize()
    skw = dict(max_seeds=MAX_SEEDS, min_len=MIN_LEN, skip=SKIP, max_occ=occ)
    vkw = dict(band=BAND, min_cover=MIN_COVER, max_cands=K)
    akw = dict(align_band=ALIGN_BAND, max_dist=MAX_DIST)

    def seeds_vote(leg):
        ix.seeds_batch_async(d_reads[leg].data_ptr(), d_off.data_ptr(), B, s_ns.data_ptr(), s_rest.data_ptr(),
                             s_spans.data_ptr(), s_rng.data_ptr(), s_loff.data_ptr(), s_locs.data_ptr(), cap,
                             s_need.data_ptr(), ws_ptr, wsb, stream=sh, stage_kb=kb, fixed_len=m, **skw)
        ix.vote_async(B, MAX_SEEDS, s_ns.data_ptr(), s_spans.data_ptr(), s_loff.data_ptr(), s_locs.data_ptr(), cap,
                      v_nc.data_ptr(), v_fl.data_ptr(), v_pos.data_ptr(), v_cov.data_ptr(), v_mask.data_ptr(),
                      stream=sh, **vkw)

    def seeds_vote_verify(leg):
        seeds_vote(leg)
        ix.verify_async(d_reads[leg].data_ptr(), d_off.data_ptr(), B, v_nc.data_ptr(), v_pos.data_ptr(),
                        a_dist.data_ptr(), a_ts.data_ptr(), a_te.data_ptr(), max_cands=K, band=ALIGN_BAND,
                        max_dist=MAX_DIST, stream=sh)

    def map_(leg):
        return ix.map_batch((h_reads[leg], h_off), **skw, **vkw, **akw)

    def host_dp(leg):
        nc, fl, pos, cov, mask = ix.place_batch((h_reads[leg], h_off), **skw, **vkw)
        return (nc, fl, pos, cov, mask) + numpy_verify(h_text, lut[h_reads[leg]], m, nc, pos, K, ALIGN_BAND, MAX_DIST)

    # results first: the three routes agree, and the best candidate starts where the read was cut
    facts = {}
    for leg in LEGS:
        a, b = map_(leg), host_dp(leg)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"map_batch != place_batch + NumPy alignment ({leg})"
        seeds_vote_verify(leg)
        ix.sync(sh)
        dv = [t.cpu().numpy() for t in (v_nc, v_fl, v_pos, v_cov, v_mask, a_dist, a_ts, a_te)]
        dv = [x.view(np.uint32) if x.dtype == np.int32 else x for x in dv]  # (FMX_VERIFY_NONE in an int32 tensor)
        assert all(np.array_equal(x.astype(np.int64), y.astype(np.int64)) for x, y in zip(a, dv)), \
            f"map_batch != seeds + vote + verify on device buffers ({leg})"
        nc, dist, ts = a[0], a[5].astype(np.int64), a[6]
        used = np.arange(K)[None, :] < nc[:, None]
        ok = used & (dist != NONE)
        best = np.where(ok, dist, 1 << 40).argmin(1)
        rows = np.arange(B)
        at_cut = ok[rows, best] & (ts[rows, best] == starts[leg])
        facts[leg] = dict(candidates=int(used.sum()), verified=int(ok.sum()), reads_verified=int(ok.any(1).sum()),
                          best_at_cut=int(at_cut.sum()), mean_best_dist=float(dist[rows, best][ok[rows, best]].mean()),
                          dp_rows=int(used.sum() + ok.sum()) * m)
        print(f"{leg}: {facts[leg]}", flush=True)
    facts["bytes"] = dict(reads_up=B * m + (B + 1) * 8, map_down=B * (8 + K * 36), text_host_copy=int(h_text.size))

    def timed_dev(fn, reps, warm):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        ix.sync(sh)
        return a.elapsed_time(b) * 1000.0 / reps  # us per call

    def timed_host(fn, reps, warm):
        for _ in range(warm):
            fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()  # (synchronous: returns with the results in host memory)
        return (time.perf_counter() - t0) * 1e6 / reps

    legs = {}
    for leg in LEGS:
        legs[f"seedsvote_{leg}"] = (timed_dev, lambda leg=leg: seeds_vote(leg), args.launches, args.warmup)
        legs[f"seedsvoteverify_{leg}"] = (timed_dev, lambda leg=leg: seeds_vote_verify(leg), args.launches, args.warmup)
        legs[f"hostdp_{leg}"] = (timed_host, lambda leg=leg: host_dp(leg), args.host_calls, 0)
        legs[f"map_{leg}"] = (timed_host, lambda leg=leg: map_(leg), args.calls, 1)
    runs = {k: [] for k in legs}
    for r in range(args.runs):
        for kind, (timer, fn, reps, warm) in legs.items():
            us = timer(fn, reps, warm)
            runs[kind].append(us)
            print(f"run {r} {kind:22s} {us:14.2f} us/call", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    adds = {leg: med[f"seedsvoteverify_{leg}"] - med[f"seedsvote_{leg}"] for leg in LEGS}
    # per run, the difference of the two legs measured next to each other: its own spread
    adds_runs = {leg: [a - b for a, b in zip(runs[f"seedsvoteverify_{leg}"], runs[f"seedsvote_{leg}"])] for leg in LEGS}
    res = {"config": args.config, "text_len": n, "patterns": B, "read_len": m, "max_seeds": MAX_SEEDS, "skip": SKIP,
           "min_len": MIN_LEN, "max_occ": occ, "band": BAND, "min_cover": MIN_COVER, "max_cands": K,
           "align_band": ALIGN_BAND, "max_dist": MAX_DIST, "launches": args.launches, "calls": args.calls,
           "host_calls": args.host_calls, "load_s": load_s, "device_bytes": info["device_bytes"],
           "runs_us": runs, "median_us": med, "spread_us": spread,
           "hostdp_over_map": {leg: med[f"hostdp_{leg}"] / med[f"map_{leg}"] for leg in LEGS},
           "verify_adds_us": adds, "verify_adds_runs_us": adds_runs,
           "verify_adds_spread_us": {leg: max(v) - min(v) for leg, v in adds_runs.items()},
           "verify_ns_per_dp_row": {leg: adds[leg] * 1000.0 / max(facts[leg]["dp_rows"], 1) for leg in LEGS},
           "verify_ns_per_dp_row_runs": {leg: [x * 1000.0 / max(facts[leg]["dp_rows"], 1) for x in adds_runs[leg]]
                                         for leg in LEGS},
           "facts": facts}
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
