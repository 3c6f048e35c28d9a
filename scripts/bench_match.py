#!/usr/bin/env python3
"""Time fmx_match_batch_async against fmx_locate_batch_async.

One index (bench.py's C2 by default: 1 Gbp ACGT, u32 / Block3<u64>, k 3, sr 2,
built on the GPU from bench.py's seeded text), one batch of 100,000 x 20 bp
reads cut from the text, three calls timed on one stream, alternating, --runs
times each:

  locate        fmx_locate_batch_async in launch order, split (FMX_FUSED=0:
                k_search + k_emit) — the yardstick: the same loads as the
                match, without its length and range stores;
  match         fmx_match_batch_async with locations, the same reads (every
                one matches whole, so its offsets and locations must equal the
                locate's: asserted before anything is timed);
  match_subst   the same reads with one random substitution each: greedy
                matching stops early there (informational).

Each figure is --launches back-to-back calls between two device events, after
--warmup calls of the same kind; the last line is one JSON object with every
run, the medians and the locate's own run-to-run spread.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the locate leg is the split launch (k_search + k_emit); read when an index is loaded
os.environ["FMX_FUSED"] = "0"

import bench  # noqa: E402  (CONFIGS, cut_patterns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--text-len", type=int, default=0, help="override the config's text length")
    ap.add_argument("--patterns", type=int, default=100_000)
    ap.add_argument("--pattern-len", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of each call (at least 3)")
    ap.add_argument("--launches", type=int, default=300, help="timed calls per run")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = bench.CONFIGS[args.config]
    n, m, B, P = args.text_len or cfg["text_len"], args.pattern_len, args.patterns, cfg["pos"]
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

    # the reads, and the same reads with one substitution each (another letter at a random position)
    pg = torch.Generator(device=dev)
    pg.manual_seed(args.seed * 1000 + 7)
    starts = torch.randint(0, n - m + 1, (B,), device=dev, dtype=torch.int64, generator=pg)
    pad = torch.zeros(64, dtype=torch.uint8, device=dev)
    reads = bench.cut_patterns(torch, d_text, starts, m)
    subst = reads.clone().view(B, m)
    pos = torch.randint(0, m, (B,), device=dev, generator=pg)
    rot = torch.randint(1, len(cfg["alphabet"]), (B,), device=dev, generator=pg)
    row = torch.arange(B, device=dev)
    old = subst[row, pos]
    code = (old[:, None] == alpha[None, :]).to(torch.int64).argmax(dim=1)
    subst[row, pos] = alpha[(code + rot) % len(cfg["alphabet"])]
    d_reads, d_subst = torch.cat([reads, pad]), torch.cat([subst.reshape(-1), pad])
    d_off = (torch.arange(B + 1, device=dev, dtype=torch.int64) * m).contiguous()
    cap = B + B // 8 + 4096
    wsb = ix.locate_workspace_size(B)
    d_ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=dev)
    ws_ptr = d_ws.data_ptr() + (-d_ws.data_ptr()) % 256
    out = {k: dict(loff=torch.zeros(B + 1, dtype=torch.int64, device=dev), locs=torch.zeros(cap, dtype=pdt, device=dev),
                   need=torch.zeros(1, dtype=torch.int64, device=dev)) for k in ("locate", "match", "match_subst")}
    d_lens = torch.zeros(B, dtype=torch.int32, device=dev)
    d_rng = torch.zeros((B, 2), dtype=pdt, device=dev)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    stage_kb = min(56, -(-256 * m // 1024))
    torch.cuda.synchronize()

    def call(kind):
        o = out[kind]
        if kind == "locate":
            ix.locate_batch_async(d_reads.data_ptr(), d_off.data_ptr(), B, o["loff"].data_ptr(), o["locs"].data_ptr(),
                                  cap, o["need"].data_ptr(), ws_ptr, wsb, stream=sh, stage_kb=stage_kb, fixed_len=m)
        else:
            src = d_reads if kind == "match" else d_subst
            ix.match_batch_async(src.data_ptr(), d_off.data_ptr(), B, d_lens.data_ptr(), d_rng.data_ptr(),
                                 o["loff"].data_ptr(), o["locs"].data_ptr(), cap, o["need"].data_ptr(), ws_ptr, wsb,
                                 stream=sh, stage_kb=stage_kb, fixed_len=m)

    # results first: on whole-matching reads the match is the locate
    for kind in out:
        call(kind)
        ix.sync(sh)
        out[kind]["lens"] = d_lens.clone()
    info = ix.info()
    assert info["launches_fused"] == 0 and info["launches_grouped"] == 0, "the locate leg must be k_search + k_emit"
    need = int(out["locate"]["need"].item())
    assert need <= cap and int(out["match"]["need"].item()) == need
    assert torch.equal(out["match"]["loff"], out["locate"]["loff"])
    assert torch.equal(out["match"]["locs"][:need], out["locate"]["locs"][:need])
    assert bool((out["match"]["lens"] == m).all())
    sl = out["match_subst"]["lens"].to(torch.float64)
    print(f"parity ok: {need:,} locations; substituted reads: mean matched length {sl.mean().item():.2f} of {m}, "
          f"{int(out['match_subst']['need'].item()):,} locations", flush=True)

    def timed(kind):
        for _ in range(args.warmup):
            call(kind)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.launches):
            call(kind)
        b.record(stream)
        ix.sync(sh)
        return a.elapsed_time(b) * 1000.0 / args.launches  # us per call

    runs = {k: [] for k in out}
    for r in range(args.runs):
        for kind in out:
            us = timed(kind)
            runs[kind].append(us)
            print(f"run {r} {kind:12s} {us:8.2f} us/call  {B / us * 1e6 / 1e9:6.3f} x 10^9 patterns/s", flush=True)
    res = {"config": args.config, "text_len": n, "patterns": B, "pattern_len": m, "launches": args.launches,
           "runs_us": runs, "median_us": {k: statistics.median(v) for k, v in runs.items()}}
    loc = runs["locate"]
    res["locate_spread_us"] = max(loc) - min(loc)
    res["locate_spread_pct"] = 100.0 * (max(loc) - min(loc)) / statistics.median(loc)
    res["match_over_locate"] = res["median_us"]["match"] / res["median_us"]["locate"]
    res["substituted_mean_len"] = float(sl.mean().item())
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
