#!/usr/bin/env python3
"""Time fmx_approx_batch_async against fmx_locate_batch_async and against the
host loop it replaces.

One index (bench.py's C2 by default: 1 Gbp ACGT, u32 / Block3<u64>, k 3, sr 2,
built on the GPU from bench.py's seeded text), 100,000 reads per call, every
call on one stream, the legs alternating, --runs times each:

  locate        (a) fmx_locate_batch_async on 20 bp reads cut from the text —
                the yardstick, timed in the same run;
  approx0       (b) fmx_approx_batch_async, max_mm = 0, max_hits = 1, the same
                reads: its intervals, offsets and locations must equal (a)'s
                (asserted before anything is timed) — the overhead of the new
                path, to be read against (a)'s own run-to-run spread;
  m{20,32}_s{0,1,2}_k{1,2}[_best]
                (c) fmx_approx_batch_async, max_hits = 8, max_occ = --max-occ,
                on 20 and 32 bp reads with 0, 1 and 2 planted substitutions, at
                max_mm = 1 and 2, with and without FMX_APPROX_BEST;
  loop_m{20,32}_s{0,1,2}
                (d) the host loop (c) replaces at max_mm = 1: the read and its
                m (sigma - 1) one-substitution variants, made with torch on the
                device (counted in the time), one fmx_locate_batch_async each.

(a), (b): --launches back-to-back calls between two device events after
--warmup calls; (c), (d): --heavy calls (whole loops) after one warm-up.  The
last line is one JSON object with every run, the medians and the yardstick's
own run-to-run spread.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, cut_patterns)

MAX_HITS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--text-len", type=int, default=0, help="override the config's text length")
    ap.add_argument("--patterns", type=int, default=100_000)
    ap.add_argument("--lens", type=int, nargs="+", default=[20, 32])
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs of each leg (at least 3)")
    ap.add_argument("--launches", type=int, default=100, help="timed calls per run, legs (a), (b)")
    ap.add_argument("--heavy", type=int, default=3, help="timed calls (loops) per run, legs (c), (d)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_approx.py needs a GPU (unmeasured without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = bench.CONFIGS[args.config]
    n, B, P = args.text_len or cfg["text_len"], args.patterns, cfg["pos"]
    occ, m0 = args.max_occ, args.lens[0]
    position = pkg.u32 if P == 4 else pkg.u64
    block = getattr(pkg.blocks, f"Block{cfg['planes']}")(pkg.Vector(cfg["vec"]))
    pdt = torch.int32 if P == 4 else torch.int64
    na = len(cfg["alphabet"])

    # bench.py's text and blob
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    alpha = torch.tensor(list(cfg["alphabet"]), dtype=torch.uint8, device=dev)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    for c0 in range(0, n, 1 << 28):
        c1 = min(n, c0 + (1 << 28))
        d_text[c0:c1] = alpha[torch.randint(0, na, (c1 - c0,), device=dev, dtype=torch.int64, generator=gen)]
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

    def code_of(x):
        return (x[..., None] == alpha).to(torch.int64).argmax(dim=-1)

    def reads_of(m, subs):
        starts = torch.randint(0, n - m + 1, (B,), device=dev, dtype=torch.int64, generator=pg)
        r = bench.cut_patterns(torch, d_text, starts, m).clone().view(B, m)
        for _ in range(subs):  # another letter at a random position
            pos = torch.randint(0, m, (B,), device=dev, generator=pg)
            rot = torch.randint(1, na, (B,), device=dev, generator=pg)
            r[row, pos] = alpha[(code_of(r[row, pos]) + rot) % na]
        return torch.cat([r.reshape(-1), pad])

    reads = {(m, s): reads_of(m, s) for m in args.lens for s in (0, 1, 2)}
    offs = {m: (torch.arange(B + 1, device=dev, dtype=torch.int64) * m).contiguous() for m in args.lens}
    S = B * MAX_HITS
    wsb = ix.locate_workspace_size(S)
    d_ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=dev)
    ws_ptr = d_ws.data_ptr() + (-d_ws.data_ptr()) % 256
    cap = S * occ + 4096
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    l_cnt, l_loff, l_locs, l_need = z(B, pdt), z(B + 1, torch.int64), z(cap, pdt), z(1, torch.int64)
    a_nh, a_more, a_mm, a_subs, a_rng = z(B), z(B), z(S), z((S, 6)), z((S, 2), pdt)
    a_loff, a_locs, a_need = z(S + 1, torch.int64), z(cap, pdt), z(1, torch.int64)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    kb = lambda m: min(56, -(-256 * m // 1024))  # noqa: E731
    torch.cuda.synchronize()

    def locate(src, m):
        ix.locate_batch_async(src.data_ptr(), offs[m].data_ptr(), B, l_loff.data_ptr(), l_locs.data_ptr(), cap,
                              l_need.data_ptr(), ws_ptr, wsb, d_counts=l_cnt.data_ptr(), stream=sh, stage_kb=kb(m),
                              fixed_len=m)

    def approx(src, m, mm, mh, best=False, max_occ=None):
        ix.approx_batch_async(src.data_ptr(), offs[m].data_ptr(), B, a_nh.data_ptr(), a_more.data_ptr(),
                              a_mm.data_ptr(), a_subs.data_ptr(), a_rng.data_ptr(), a_loff.data_ptr(),
                              a_locs.data_ptr(), cap, a_need.data_ptr(), ws_ptr, wsb, max_mm=mm, max_hits=mh, best=best,
                              max_occ=max_occ, stream=sh, stage_kb=kb(m), fixed_len=m)

    def host_loop(src, m):
        """The read, then every one-substitution variant, each through a locate; returns the hits."""
        hits = 0
        with torch.cuda.stream(stream):
            base = src[:B * m].view(B, m)
            codes = code_of(base)
            locate(src, m)
            hits += int((l_cnt != 0).sum().item())
            for q in range(m - 1, -1, -1):
                for rot in range(1, na):
                    v = base.clone()
                    v[:, q] = alpha[(codes[:, q] + rot) % na]
                    vv = torch.cat([v.reshape(-1), pad])
                    locate(vv, m)
                    hits += int((l_cnt != 0).sum().item())  # (the call's host read-back)
        return hits

    # results first
    locate(reads[(m0, 0)], m0)
    approx(reads[(m0, 0)], m0, 0, 1)
    ix.sync(sh)
    need = int(l_need.item())
    assert need <= cap and int(a_need.item()) == need and bool((a_nh == 1).all()) and not bool(a_more.any())
    assert torch.equal((a_rng[:B, 1] - a_rng[:B, 0]), l_cnt) and torch.equal(a_loff[:B + 1], l_loff)
    assert torch.equal(a_locs[:need], l_locs[:need])
    print(f"parity ok: approx(max_mm=0) == locate on {B:,} x {m0} bp, {need:,} locations", flush=True)
    facts = {}
    for (m, s), src in reads.items():
        for mm in (1, 2):
            approx(src, m, mm, MAX_HITS, max_occ=occ)
            ix.sync(sh)
            assert int(a_need.item()) <= cap
            facts[f"m{m}_s{s}_k{mm}"] = dict(hits=int(a_nh.sum().item()), truncated=int(a_more.sum().item()),
                                             reads_hit=int((a_nh > 0).sum().item()), locations=int(a_need.item()))
    for m in args.lens:  # the host loop finds what approx(max_mm = 1) finds
        src = reads[(m, 1)]
        approx(src, m, 1, MAX_HITS)
        ix.sync(sh)
        full = not bool(a_more.any())
        got = int(a_nh.sum().item())
        found = host_loop(src, m)
        ix.sync(sh)
        assert not full or found == got, (found, got)
        facts[f"loop_m{m}_s1"] = dict(loop_hits=found, approx_hits=got, approx_truncated=not full)
        print(f"{m} bp, 1 substitution: approx {got:,} hits, host loop {found:,} over {1 + m * (na - 1)} locates",
              flush=True)

    def timed(fn, reps, warm):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        ix.sync(sh)
        return a.elapsed_time(b) * 1000.0 / reps  # us per call (per whole loop)

    legs = {"locate": (lambda: locate(reads[(m0, 0)], m0), args.launches, args.warmup),
            "approx0": (lambda: approx(reads[(m0, 0)], m0, 0, 1), args.launches, args.warmup)}
    for (m, s), src in reads.items():
        for mm in (1, 2):
            for best in (False, True):
                legs[f"m{m}_s{s}_k{mm}" + ("_best" if best else "")] = (
                    lambda src=src, m=m, mm=mm, best=best: approx(src, m, mm, MAX_HITS, best, occ), args.heavy, 1)
        legs[f"loop_m{m}_s{s}"] = (lambda src=src, m=m: host_loop(src, m), 1, 0)
    runs = {k: [] for k in legs}
    for r in range(args.runs):
        for kind, (fn, reps, warm) in legs.items():
            us = timed(fn, reps, warm)
            runs[kind].append(us)
            print(f"run {r} {kind:18s} {us:12.2f} us/call", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    ya = runs["locate"]
    res = {"config": args.config, "text_len": n, "patterns": B, "lens": args.lens, "max_hits": MAX_HITS,
           "max_occ": occ, "launches": args.launches, "heavy": args.heavy, "runs_us": runs, "median_us": med,
           "locate_spread_us": max(ya) - min(ya), "approx0_over_locate": med["approx0"] / med["locate"],
           "loop_over_approx_k1": {f"m{m}_s{s}": med[f"loop_m{m}_s{s}"] / med[f"m{m}_s{s}_k1"]
                                   for (m, s) in reads}, "facts": facts}
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
