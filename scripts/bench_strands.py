#!/usr/bin/env python3
"""Time FMX_BOTH_STRANDS against what callers did before it: the flag-less call
on the expanded batch p_0, rc(p_0), p_1, rc(p_1), ... (include/fmx.h, "Both
strands").

One index (bench.py's C2 by default: 1 Gbp ACGT, u32 / Block3<u64>, k 3, sr 2,
built on the GPU from bench.py's seeded text), 100,000 reads of 20 bp and of
150 bp cut from the text, every second one reverse-complemented (so both
strands match), complement A<->T, C<->G.  Per read length and per query —
match, seeds (max_seeds = 8, min_len = 12) and approx (max_mm = 1, max_hits =
8), all with locations, max_occ = --max-occ — four legs, alternating, --runs
times each:

  both      (a) the device call of n reads with FMX_BOTH_STRANDS;
  expanded  (b) the flag-less device call of the 2n-pattern batch, built on
            the device before anything is timed — the yardstick;
  h_both    (c) the host-buffer call of n reads with the flag (uploads n reads);
  h_expanded    the host-buffer call of the expanded batch (uploads 2n).

(a)'s outputs must equal (b)'s, element for element (asserted before anything
is timed).  (a), (b): --launches back-to-back calls between two device events
after --warmup calls; (c): --host-calls calls by the wall clock after one.
The last line is one JSON object with every run, the medians, (a) over (b) per
leg and (b)'s own run-to-run spread.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, cut_patterns)

PER, MIN_LEN, MAX_MM = 8, 12, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--text-len", type=int, default=0, help="override the config's text length")
    ap.add_argument("--patterns", type=int, default=100_000)
    ap.add_argument("--lens", type=int, nargs="+", default=[20, 150])
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of each leg (at least 3)")
    ap.add_argument("--launches", type=int, default=100, help="timed calls per run, device legs")
    ap.add_argument("--host-calls", type=int, default=3, help="timed calls per run, host legs")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    import numpy as np
    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_strands.py needs a GPU (unmeasured without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = bench.CONFIGS[args.config]
    if bytes(cfg["alphabet"]) != b"ACGT":
        raise SystemExit("bench_strands.py complements ACGT: pick a DNA config")
    n, B, P, occ = args.text_len or cfg["text_len"], args.patterns, cfg["pos"], args.max_occ
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
    cmap = pkg.complement_map([(b"A", b"T"), (b"C", b"G")])
    ix.set_complement(cmap)
    d_cmap = torch.tensor(list(cmap), dtype=torch.uint8, device=dev)
    print(f"index: {cfg['desc']}; text {n:,}, options {ix.info()['options']}, record {ix.info()['occ_record']}",
          flush=True)

    pg = torch.Generator(device=dev)
    pg.manual_seed(args.seed * 1000 + 17)
    pad = torch.zeros(64, dtype=torch.uint8, device=dev)
    S = 2 * B * PER
    wsb = ix.locate_workspace_size(S)
    d_ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=dev)
    ws_ptr = d_ws.data_ptr() + (-d_ws.data_ptr()) % 256
    cap = S * occ + 4096
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731

    def rc(r):
        return d_cmap[r.flip(1).to(torch.int64)]

    class Outs:
        """One set of 2n-shaped outputs per query (the widest: approx's)."""
        def __init__(self):
            self.c0, self.c1 = z(2 * B), z(2 * B)
            self.mm, self.subs, self.spans, self.rng = z(S), z((S, 6)), z((S, 2)), z((S, 2), pdt)
            self.loff, self.locs, self.need = z(S + 1, torch.int64), z(cap, pdt), z(1, torch.int64)

        def used(self, query, need):
            own = {"match": (self.c0[:2 * B], self.rng[:2 * B]),
                   "seeds": (self.c0, self.c1, self.spans, self.rng),
                   "approx": (self.c0, self.c1, self.mm, self.subs, self.rng)}[query]
            slots = 2 * B * (1 if query == "match" else PER)
            return own + (self.loff[:slots + 1], self.locs[:need])

    oa, ob = Outs(), Outs()

    def device_call(query, o, src, offs, cnt, m, strands):
        loc = (o.loff.data_ptr(), o.locs.data_ptr(), cap, o.need.data_ptr(), ws_ptr, wsb)
        # (each tile's bytes; both strands' copies of a 128-read tile are as many as a 256-pattern tile's)
        kw = dict(stream=sh, stage_kb=min(56, -(-256 * m // 1024)), fixed_len=m, strands=strands, max_occ=occ)
        a = (src.data_ptr(), offs.data_ptr(), cnt)
        if query == "match":
            ix.match_batch_async(*a, o.c0.data_ptr(), o.rng.data_ptr(), *loc, min_len=MIN_LEN, **kw)
        elif query == "seeds":
            ix.seeds_batch_async(*a, o.c0.data_ptr(), o.c1.data_ptr(), o.spans.data_ptr(), o.rng.data_ptr(), *loc,
                                 max_seeds=PER, min_len=MIN_LEN, **kw)
        else:
            ix.approx_batch_async(*a, o.c0.data_ptr(), o.c1.data_ptr(), o.mm.data_ptr(), o.subs.data_ptr(),
                                  o.rng.data_ptr(), *loc, max_mm=MAX_MM, max_hits=PER, **kw)

    def host_call(query, pats, strands):
        kw = dict(strands=strands, max_occ=occ)
        if query == "match":
            return ix.match_batch(pats, min_len=MIN_LEN, **kw)
        if query == "seeds":
            return ix.seeds_batch(pats, max_seeds=PER, min_len=MIN_LEN, **kw)
        return ix.approx_batch(pats, max_mm=MAX_MM, max_hits=PER, **kw)

    def timed(fn, reps, warm):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        ix.sync(sh)
        return a.elapsed_time(b) * 1000.0 / reps  # us per call

    def walled(fn, reps):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e6 / reps

    legs, facts = {}, {}
    for m in args.lens:
        starts = torch.randint(0, n - m + 1, (B,), device=dev, dtype=torch.int64, generator=pg)
        r = bench.cut_patterns(torch, d_text, starts, m).clone().view(B, m)
        r[1::2] = rc(r[1::2])  # every second read from the other strand
        x = torch.stack([r, rc(r)], dim=1).reshape(2 * B, m)  # the expanded batch
        d_reads, d_exp = torch.cat([r.reshape(-1), pad]), torch.cat([x.reshape(-1), pad])
        off_r = (torch.arange(B + 1, device=dev, dtype=torch.int64) * m).contiguous()
        off_x = (torch.arange(2 * B + 1, device=dev, dtype=torch.int64) * m).contiguous()
        h_reads = (r.reshape(-1).cpu().numpy(), off_r.cpu().numpy().astype(np.uint64))
        h_exp = (x.reshape(-1).cpu().numpy(), off_x.cpu().numpy().astype(np.uint64))
        for query in ("match", "seeds", "approx"):
            # results first: (a) == (b), and the host forms agree with them
            device_call(query, oa, d_reads, off_r, B, m, "both")
            device_call(query, ob, d_exp, off_x, 2 * B, m, "forward")
            ix.sync(sh)
            need = int(oa.need.item())
            assert need <= cap and int(ob.need.item()) == need
            for u, v in zip(oa.used(query, need), ob.used(query, need)):
                assert torch.equal(u, v), (query, m)
            hb, hx = host_call(query, h_reads, "both"), host_call(query, h_exp, "forward")
            assert all(np.array_equal(u, v) for u, v in zip(hb, hx)) and hb[-1].size == need
            loff = oa.used(query, need)[-2]
            facts[f"{query}{m}"] = dict(locations=need, reporting_slots=int((loff[1:] > loff[:-1]).sum().item()))
            print(f"parity ok: {query} {B:,} x {m} bp, both == expanded, {need:,} locations", flush=True)
            legs[f"{query}{m}_both"] = (lambda q=query, d=d_reads, o=off_r, m=m:
                                        device_call(q, oa, d, o, B, m, "both"), None)
            legs[f"{query}{m}_expanded"] = (lambda q=query, d=d_exp, o=off_x, m=m:
                                            device_call(q, ob, d, o, 2 * B, m, "forward"), None)
            legs[f"{query}{m}_h_both"] = (None, lambda q=query, h=h_reads: host_call(q, h, "both"))
            legs[f"{query}{m}_h_expanded"] = (None, lambda q=query, h=h_exp: host_call(q, h, "forward"))

    runs = {k: [] for k in legs}
    for rr in range(args.runs):
        for kind, (dfn, hfn) in legs.items():
            us = timed(dfn, args.launches, args.warmup) if dfn else walled(hfn, args.host_calls)
            runs[kind].append(us)
            print(f"run {rr} {kind:22s} {us:10.2f} us/call", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    ratio, spread = {}, {}
    for k in legs:
        if k.endswith("_both"):
            base = k[:-len("both")] + "expanded"
            ratio[k[:-len("_both")]] = med[k] / med[base]
            spread[k[:-len("_both")]] = (max(runs[base]) - min(runs[base])) / med[base]
    res = {"config": args.config, "text_len": n, "reads": B, "lens": args.lens, "per": PER, "min_len": MIN_LEN,
           "max_mm": MAX_MM, "max_occ": occ, "launches": args.launches, "host_calls": args.host_calls,
           "runs_us": runs, "median_us": med, "both_over_expanded": ratio, "expanded_spread": spread, "facts": facts}
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
