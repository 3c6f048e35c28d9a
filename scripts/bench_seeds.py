#!/usr/bin/env python3
"""Time fmx_seeds_batch_async against fmx_match_batch_async and against the
host loop it replaces.

One index (bench.py's C2 by default: 1 Gbp ACGT, u32 / Block3<u64>, k 3, sr 2,
built on the GPU from bench.py's seeded text), 100,000 reads per call, every
call on one stream, the legs alternating, --runs times each:

  match         (a) fmx_match_batch_async with locations on 20 bp reads cut
                from the text (each matches whole) — the yardstick, timed in
                the same run;
  seeds1        (b) fmx_seeds_batch_async, max_seeds = 1, the same reads: its
                spans, ranges, offsets and locations must equal (a)'s
                (asserted before anything is timed);
  seeds_s{0,1,3}  (c) fmx_seeds_batch_async, max_seeds = 8, skip = 1, min_len =
                12, max_occ = --max-occ, on 150 bp reads with 0, 1 and 3
                random substitutions;
  loop_s{0,1,3}   (d) the host loop (c) replaces, on the same reads: repeated
                fmx_match_batch_async (same min_len / max_occ) on device-side
                prefixes, each round's lengths cut by max(L + skip, 1) and the
                patterns that have symbols left re-packed with torch on the
                device (counted in the time), one host read-back per round to
                learn whether any are left.

(a)-(c): --launches back-to-back calls between two device events after --warmup
calls; (d): --loops whole loops between two device events after one warm-up
loop.  The last line is one JSON object with every run, the medians and the
yardstick's own run-to-run spread.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (CONFIGS, cut_patterns)

MAX_SEEDS, SKIP, MIN_LEN = 8, 1, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--text-len", type=int, default=0, help="override the config's text length")
    ap.add_argument("--patterns", type=int, default=100_000)
    ap.add_argument("--short-len", type=int, default=20)
    ap.add_argument("--long-len", type=int, default=150)
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of each leg (at least 3)")
    ap.add_argument("--launches", type=int, default=200, help="timed calls per run, legs (a)-(c)")
    ap.add_argument("--loops", type=int, default=10, help="timed host loops per run, leg (d)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seeds.py needs a GPU (unmeasured without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = bench.CONFIGS[args.config]
    n, B, P = args.text_len or cfg["text_len"], args.patterns, cfg["pos"]
    m20, m150, occ = args.short_len, args.long_len, args.max_occ
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
    pg.manual_seed(args.seed * 1000 + 11)
    pad = torch.zeros(64, dtype=torch.uint8, device=dev)
    row = torch.arange(B, device=dev)

    def reads_of(m, subs):
        starts = torch.randint(0, n - m + 1, (B,), device=dev, dtype=torch.int64, generator=pg)
        r = bench.cut_patterns(torch, d_text, starts, m).clone().view(B, m)
        for _ in range(subs):  # another letter at a random position
            pos = torch.randint(0, m, (B,), device=dev, generator=pg)
            rot = torch.randint(1, len(cfg["alphabet"]), (B,), device=dev, generator=pg)
            code = (r[row, pos][:, None] == alpha[None, :]).to(torch.int64).argmax(dim=1)
            r[row, pos] = alpha[(code + rot) % len(cfg["alphabet"])]
        return torch.cat([r.reshape(-1), pad])

    d_short = reads_of(m20, 0)
    d_long = {s: reads_of(m150, s) for s in (0, 1, 3)}
    off20 = (torch.arange(B + 1, device=dev, dtype=torch.int64) * m20).contiguous()
    off150 = (torch.arange(B + 1, device=dev, dtype=torch.int64) * m150).contiguous()
    S = B * MAX_SEEDS
    wsb = ix.locate_workspace_size(S)
    d_ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=dev)
    ws_ptr = d_ws.data_ptr() + (-d_ws.data_ptr()) % 256
    cap = S * occ + 4096
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    # (a)'s outputs, and one set for every seeds call
    a_lens, a_rng, a_loff, a_locs, a_need = z(B), z((B, 2), pdt), z(B + 1, torch.int64), z(cap, pdt), z(1, torch.int64)
    s_ns, s_rest, s_spans, s_rng = z(B), z(B), z((S, 2)), z((S, 2), pdt)
    s_loff, s_locs, s_need = z(S + 1, torch.int64), z(cap, pdt), z(1, torch.int64)
    # (d)'s outputs and re-packed prefixes (never larger than the first round's)
    l_lens, l_rng, l_loff, l_locs, l_need = z(B), z((B, 2), pdt), z(B + 1, torch.int64), z(cap, pdt), z(1, torch.int64)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    kb = lambda m: min(56, -(-256 * m // 1024))  # noqa: E731
    torch.cuda.synchronize()

    def match20():
        ix.match_batch_async(d_short.data_ptr(), off20.data_ptr(), B, a_lens.data_ptr(), a_rng.data_ptr(),
                             a_loff.data_ptr(), a_locs.data_ptr(), cap, a_need.data_ptr(), ws_ptr, wsb, stream=sh,
                             stage_kb=kb(m20), fixed_len=m20)

    def seeds(src, offs, m, ms, **kw):
        ix.seeds_batch_async(src.data_ptr(), offs.data_ptr(), B, s_ns.data_ptr(), s_rest.data_ptr(),
                             s_spans.data_ptr(), s_rng.data_ptr(), s_loff.data_ptr(), s_locs.data_ptr(), cap,
                             s_need.data_ptr(), ws_ptr, wsb, max_seeds=ms, stream=sh, stage_kb=kb(m), fixed_len=m, **kw)

    def host_loop(src):
        """(rounds, seeds found): match, cut, re-pack, until nothing is left."""
        rounds = found = 0
        with torch.cuda.stream(stream):
            data, offs, cnt = src, off150, B
            while cnt:
                ix.match_batch_async(data.data_ptr(), offs.data_ptr(), cnt, l_lens.data_ptr(), l_rng.data_ptr(),
                                     l_loff.data_ptr(), l_locs.data_ptr(), cap, l_need.data_ptr(), ws_ptr, wsb,
                                     min_len=MIN_LEN, max_occ=occ, stream=sh, stage_kb=kb(m150))
                L = l_lens[:cnt].to(torch.int64)
                e = offs[1:cnt + 1] - offs[:cnt]
                e2 = e - torch.minimum(e, torch.clamp(L + SKIP, min=1))
                keep = e2 > 0
                found += int((L >= MIN_LEN).sum().item())
                cnt2 = int(keep.sum().item())  # (the round's host read-back)
                rounds += 1
                if cnt2:
                    ln = e2[keep]
                    noff = torch.zeros(cnt2 + 1, dtype=torch.int64, device=dev)
                    torch.cumsum(ln, 0, out=noff[1:])
                    pid = torch.repeat_interleave(torch.arange(cnt2, device=dev), ln)
                    idx = torch.arange(int(noff[-1].item()), device=dev) - noff[pid] + offs[:cnt][keep][pid]
                    data, offs = torch.cat([data[idx], pad]), noff
                cnt = cnt2
        return rounds, found

    # results first
    match20()
    seeds(d_short, off20, m20, 1)
    ix.sync(sh)
    need = int(a_need.item())
    assert need <= cap and int(s_need.item()) == need and bool((a_lens == m20).all())
    assert bool((s_ns == 1).all()) and bool((s_rest == 0).all())
    assert torch.equal(s_spans[:B, 0], torch.full_like(a_lens, m20)) and torch.equal(s_spans[:B, 1], a_lens)
    assert torch.equal(s_rng[:B], a_rng) and torch.equal(s_loff[:B + 1], a_loff)
    assert torch.equal(s_locs[:need], a_locs[:need])
    print(f"parity ok: seeds(max_seeds=1) == match on {B:,} x {m20} bp, {need:,} locations", flush=True)
    facts = {}
    for s in (0, 1, 3):
        seeds(d_long[s], off150, m150, MAX_SEEDS, min_len=MIN_LEN, skip=SKIP, max_occ=occ)
        ix.sync(sh)
        nseeds, left, total = int(s_ns.sum().item()), int((s_rest > 0).sum().item()), int(s_need.item())
        assert total <= cap
        rounds, found = host_loop(d_long[s])
        ix.sync(sh)
        assert left or found == nseeds, (found, nseeds)  # (the same seeds, unless a chain ran out of slots)
        facts[s] = dict(seeds=nseeds, out_of_slots=left, locations=total, loop_rounds=rounds, loop_seeds=found)
        print(f"{s} substitutions: {nseeds:,} seeds, {total:,} locations, {left} reads out of slots; "
              f"host loop {rounds} rounds, {found:,} seeds", flush=True)

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

    legs = {"match": (match20, args.launches, args.warmup),
            "seeds1": (lambda: seeds(d_short, off20, m20, 1), args.launches, args.warmup)}
    for s in (0, 1, 3):
        legs[f"seeds_s{s}"] = (lambda s=s: seeds(d_long[s], off150, m150, MAX_SEEDS, min_len=MIN_LEN, skip=SKIP,
                                                 max_occ=occ), args.launches, args.warmup)
        legs[f"loop_s{s}"] = (lambda s=s: host_loop(d_long[s]), args.loops, 1)
    runs = {k: [] for k in legs}
    for r in range(args.runs):
        for kind, (fn, reps, warm) in legs.items():
            us = timed(fn, reps, warm)
            runs[kind].append(us)
            print(f"run {r} {kind:10s} {us:10.2f} us/call", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    ya = runs["match"]
    res = {"config": args.config, "text_len": n, "patterns": B, "short_len": m20, "long_len": m150,
           "max_seeds": MAX_SEEDS, "skip": SKIP, "min_len": MIN_LEN, "max_occ": occ, "launches": args.launches,
           "loops": args.loops, "runs_us": runs, "median_us": med, "match_spread_us": max(ya) - min(ya),
           "seeds1_over_match": med["seeds1"] / med["match"],
           "loop_over_seeds": {s: med[f"loop_s{s}"] / med[f"seeds_s{s}"] for s in (0, 1, 3)}, "facts": facts}
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
