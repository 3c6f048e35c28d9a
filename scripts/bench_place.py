#!/usr/bin/env python3
"""Time read placement (fmx_place_batch, fmx_vote_async) against what the
parent of that change already had (profiles/r13/README.md).

One index (bench.py's C2 by default: 1 Gbp ACGT, u32 / Block3<u64>, k 3, sr 2,
built on the GPU from bench.py's seeded text), 100,000 reads of 150 bp per
call with 0, 1 and 3 random substitutions, max_seeds = 8, skip = 1, min_len =
12, max_occ = 16, band = 8, min_cover = 20, max_cands = 4; the legs alternate,
--runs times each:

  host buffers (wall clock around synchronous calls, --calls per run)
    place_s{0,1,3}     fmx_place_batch: reads up, candidates down;
    hostvote_s{0,1,3}  the loop it replaces: fmx_seeds_batch with locations
                       (spans, ranges, offsets and locations down), then the
                       vote in vectorised NumPy on the host — its candidates
                       must equal place_batch's (asserted before anything is
                       timed);
  device buffers (device events around --launches back-to-back calls)
    seeds_s{0,1,3}     fmx_seeds_batch_async alone: the baseline;
    seedsvote_s{0,1,3} the same launch followed by fmx_vote_async on its
                       buffers: what the vote adds.

The last line is one JSON object with every run, the medians and each
baseline's own run-to-run spread.  Needs a GPU.
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


def numpy_vote(ns, spans, loff, locs, ms, band, min_cover, K):
    """The contract of fmx_vote_async for chains that do not overflow, whole
    batch at a time: (ncands, flags, pos, cover, mask)."""
    n = ns.size
    cnt = np.diff(loff.astype(np.int64))
    slot = np.repeat(np.arange(n * ms), cnt)
    chain, j = slot // ms, slot % ms
    sp = spans.reshape(-1, 2).astype(np.int64)
    d = locs.astype(np.int64) - (sp[slot, 0] - sp[slot, 1])
    order = np.lexsort((j, d, chain))
    chain, j, d = chain[order], j[order], d[order]
    head = np.ones(d.size, bool)
    head[1:] = (chain[1:] != chain[:-1]) | (d[1:] - d[:-1] > band)
    at = np.flatnonzero(head)
    out = (np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, K), np.int64), np.zeros((n, K), np.uint32),
           np.zeros((n, K), np.uint32))
    if at.size == 0:
        return out
    mask = np.bitwise_or.reduceat(np.left_shift(1, j).astype(np.uint32), at)
    c_chain, c_pos = chain[at], d[at]
    L = sp[:, 1].reshape(n, ms)
    cover = (((mask[:, None] >> np.arange(ms, dtype=np.uint32)) & 1) * L[c_chain]).sum(axis=1)
    keep = cover >= min_cover
    c_chain, c_pos, mask, cover = c_chain[keep], c_pos[keep], mask[keep], cover[keep]
    order = np.lexsort((c_pos, -cover, c_chain))
    c_chain, c_pos, mask, cover = c_chain[order], c_pos[order], mask[order], cover[order]
    Q = np.bincount(c_chain, minlength=n)
    first = np.concatenate([[0], np.cumsum(Q)[:-1]])
    rank = np.arange(c_chain.size) - first[c_chain]
    top = rank < K
    out[0][:] = np.minimum(Q, K)
    out[1][:] = np.where(Q > K, 2, 0)
    out[2][c_chain[top], rank[top]] = c_pos[top]
    out[3][c_chain[top], rank[top]] = cover[top]
    out[4][c_chain[top], rank[top]] = mask[top]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--text-len", type=int, default=0, help="override the config's text length")
    ap.add_argument("--patterns", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of each leg (at least 3)")
    ap.add_argument("--launches", type=int, default=100, help="timed calls per run, device-buffer legs")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per run, host-buffer legs")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_place.py needs a GPU (unmeasured without one)")
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
    alpha = torch.tensor(list(cfg["alphabet"]), dtype=torch.uint8, device=dev)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    for c0 in range(0, n, 1 << 28):
        c1 = min(n, c0 + (1 << 28))
        d_text[c0:c1] = alpha[torch.randint(0, len(cfg["alphabet"]), (c1 - c0,), device=dev, dtype=torch.int64,
                                            generator=gen)]
    table = pkg.text_encoders.EncodingTable.from_symbols(cfg["symbols"])
    builder = (pkg.FmIndexBuilder(n, table.symbol_count(), table, position, block)
               .set_lookup_table_config(pkg.build_config.LookupTableConfig.KmerSize(cfg["k"]))
               .set_suffix_array_config(pkg.build_config.SuffixArrayConfig.Compressed(cfg["sr"])))
    blob_len = builder.blob_size()
    d_blob = torch.empty(blob_len, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    builder.build_device(d_text.data_ptr(), d_blob.data_ptr(), blob_len, device=0)
    ix = pkg.FmIndex.load_device(d_blob.data_ptr(), blob_len, position, block, pkg.text_encoders.EncodingTable,
                                 device=0, options=pkg._native.FMX_OPT_DEFAULT)
    print(f"index: {cfg['desc']}; text {n:,}, options {ix.info()['options']}, record {ix.info()['occ_record']}",
          flush=True)

    pg = torch.Generator(device=dev)
    pg.manual_seed(args.seed * 1000 + 13)
    pad = torch.zeros(64, dtype=torch.uint8, device=dev)
    row = torch.arange(B, device=dev)

    def reads_of(subs):
        starts = torch.randint(0, n - m + 1, (B,), device=dev, dtype=torch.int64, generator=pg)
        r = bench.cut_patterns(torch, d_text, starts, m).clone().view(B, m)
        for _ in range(subs):  # another letter at a random position
            pos = torch.randint(0, m, (B,), device=dev, generator=pg)
            rot = torch.randint(1, len(cfg["alphabet"]), (B,), device=dev, generator=pg)
            code = (r[row, pos][:, None] == alpha[None, :]).to(torch.int64).argmax(dim=1)
            r[row, pos] = alpha[(code + rot) % len(cfg["alphabet"])]
        return torch.cat([r.reshape(-1), pad]), starts

    d_reads, starts, h_reads = {}, {}, {}
    for s in (0, 1, 3):
        d_reads[s], starts[s] = reads_of(s)
        h_reads[s] = d_reads[s][:B * m].cpu().numpy()
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
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    kb = min(56, -(-256 * m // 1024))
    torch.cuda.synchronize()
    skw = dict(max_seeds=MAX_SEEDS, min_len=MIN_LEN, skip=SKIP, max_occ=occ)
    vkw = dict(band=BAND, min_cover=MIN_COVER, max_cands=K)

    def seeds(s):
        ix.seeds_batch_async(d_reads[s].data_ptr(), d_off.data_ptr(), B, s_ns.data_ptr(), s_rest.data_ptr(),
                             s_spans.data_ptr(), s_rng.data_ptr(), s_loff.data_ptr(), s_locs.data_ptr(), cap,
                             s_need.data_ptr(), ws_ptr, wsb, stream=sh, stage_kb=kb, fixed_len=m, **skw)

    def seeds_vote(s):
        seeds(s)
        ix.vote_async(B, MAX_SEEDS, s_ns.data_ptr(), s_spans.data_ptr(), s_loff.data_ptr(), s_locs.data_ptr(), cap,
                      v_nc.data_ptr(), v_fl.data_ptr(), v_pos.data_ptr(), v_cov.data_ptr(), v_mask.data_ptr(),
                      stream=sh, **vkw)

    def place(s):
        return ix.place_batch((h_reads[s], h_off), **skw, **vkw)

    # the baseline's host outputs, allocated once, and room for every location: one pass, no retry
    npdt = np.uint32 if P == 4 else np.uint64
    b_ns, b_rest, b_spans, b_rng = (np.zeros(B, np.uint32), np.zeros(B, np.uint32), np.zeros((S, 2), np.uint32),
                                    np.zeros((S, 2), npdt))
    b_loff, b_locs = np.zeros(S + 1, np.uint64), np.zeros(cap, npdt)
    lib = pkg._native.lib()

    def host_vote(s):
        import ctypes as C
        needed = C.c_uint64()
        st = lib.fmx_seeds_batch(ix.handle, h_reads[s].ctypes.data, h_off.ctypes.data, B, 0, MAX_SEEDS, MIN_LEN, SKIP,
                                 occ, b_ns.ctypes.data, b_rest.ctypes.data, b_spans.ctypes.data, b_rng.ctypes.data,
                                 b_loff.ctypes.data, b_locs.ctypes.data, cap, C.byref(needed))
        assert st == 0, st
        return numpy_vote(b_ns, b_spans, b_loff, b_locs[:needed.value], MAX_SEEDS, BAND, MIN_COVER, K)

    # results first: the three routes agree, and the best candidate is where the read was cut
    facts = {}
    for s in (0, 1, 3):
        a, b = place(s), host_vote(s)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"place_batch != seeds_batch + NumPy vote ({s} subs)"
        seeds_vote(s)
        ix.sync(sh)
        dv = [t.cpu().numpy() for t in (v_nc, v_fl, v_pos, v_cov, v_mask)]
        assert all(np.array_equal(x.astype(np.int64), y.astype(np.int64)) for x, y in zip(a, dv))
        placed = int(((a[0] >= 1) & (a[2][:, 0] == starts[s].cpu().numpy())).sum())
        facts[s] = dict(placed_at_cut=placed, no_candidate=int((a[0] == 0).sum()), more=int((a[1] == 2).sum()),
                        locations=int(s_need.item()), overflow=int((a[1] == 1).sum()))
        print(f"{s} substitutions: {facts[s]}", flush=True)
    up = B * m + (B + 1) * 8
    facts["bytes"] = dict(reads_up=up, place_down=B * (8 + K * 16),
                          hostvote_down={s: B * 8 + S * (8 + 2 * P + 8) + 8 + facts[s]["locations"] * P for s in (0, 1, 3)})

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
    for s in (0, 1, 3):
        legs[f"seeds_s{s}"] = (timed_dev, lambda s=s: seeds(s), args.launches, args.warmup)
        legs[f"seedsvote_s{s}"] = (timed_dev, lambda s=s: seeds_vote(s), args.launches, args.warmup)
        legs[f"hostvote_s{s}"] = (timed_host, lambda s=s: host_vote(s), args.calls, 1)
        legs[f"place_s{s}"] = (timed_host, lambda s=s: place(s), args.calls, 1)
    runs = {k: [] for k in legs}
    for r in range(args.runs):
        for kind, (timer, fn, reps, warm) in legs.items():
            us = timer(fn, reps, warm)
            runs[kind].append(us)
            print(f"run {r} {kind:14s} {us:12.2f} us/call", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    res = {"config": args.config, "text_len": n, "patterns": B, "read_len": m, "max_seeds": MAX_SEEDS, "skip": SKIP,
           "min_len": MIN_LEN, "max_occ": occ, "band": BAND, "min_cover": MIN_COVER, "max_cands": K,
           "launches": args.launches, "calls": args.calls, "runs_us": runs, "median_us": med, "spread_us": spread,
           "hostvote_over_place": {s: med[f"hostvote_s{s}"] / med[f"place_s{s}"] for s in (0, 1, 3)},
           "vote_adds_us": {s: med[f"seedsvote_s{s}"] - med[f"seeds_s{s}"] for s in (0, 1, 3)},
           "seedsvote_over_seeds": {s: med[f"seedsvote_s{s}"] / med[f"seeds_s{s}"] for s in (0, 1, 3)}, "facts": facts}
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
