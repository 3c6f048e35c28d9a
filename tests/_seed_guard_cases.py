"""Guard bands around fmx_seeds_batch_async: the one run that the emulator
tests (test_seeds_guard_simt.py) and the GPU tests (test_gpu_seeds_guard.py)
share.  The arena, its fill bytes and the two memories are _guard_cases.py's,
the batches and expected values _seed_cases.py's.

Every buffer of the call is carved at its exact size and weakest alignment
(d_nseeds, d_rest and d_spans 4 B past a 16-B boundary, d_ranges and d_locs P
bytes, the uint64 arrays 8, the workspace — fmx_locate_workspace_size(n *
max_seeds) bytes — 16 B past a 256-B boundary, the pattern bytes at the given
skew, flush against the end guard).  After the launch: every guard byte
intact, the inputs unchanged, every output the expected value,
d_locs[min(cap, total):cap] still the prefill.  Batches of 257 and 700
patterns run once more with a 1 KB stage: the unstaged path of k_seeds.
run_seeds also takes an explicit pattern list with its own parameters and
hints (tests/_long_cases.py: reads of mapper length, which tile is staged and
which is raw asserted from the offsets)."""
import numpy as np

from _guard_cases import FILL_OUT, Arena
from _seed_cases import batch, expected_arrays
from _strand_cases import staged_tiles

MAX_SEEDS, MIN_LEN, SKIP, MAX_OCC = 3, 2, 1, 3
BATCH_SIZES = (1, 257, 700)
SKEWS = (0, 1, 7, 15)
CAPS = ("total", "total-1", "zero-null")
# (P bytes, planes, vector bits): u32 and u64 positions
LAYOUTS = [(4, 3, 64), (8, 5, 128)]


def run_seeds(pkg, ix, mem_cls, case, orc, pb, n, cap_name, skew, reversed, locate=True, stage_kb=0, pats=None,
              params=None, fixed_len=0, long_patterns=False, tiles=None):
    """stage_kb: FMX_HINT_STAGE_KB; 1 leaves no tile of these batches room in
    LDS, so k_seeds reads every pattern from HBM (the unstaged prefix view: a
    reversed pattern's raw pointer advanced with each restart).
    pats: the patterns (n of them) in place of batch(case, n), whose class
    check is then the caller's; params: (max_seeds, min_len, skip, max_occ) in
    place of the module's; fixed_len, long_patterns: the other hints; tiles:
    the caller's list of staged (True) and raw tiles, asserted against
    _strand_cases.staged_tiles() in place of the stage_kb check below."""
    own = pats is None
    pats = batch(case, n) if own else pats
    assert len(pats) == n
    ms, min_len, skip, max_occ = params or (MAX_SEEDS, MIN_LEN, SKIP, MAX_OCC)
    exp = expected_arrays(case, orc, pats, ms, min_len, skip, max_occ)
    total = int(exp[4][-1])
    if own and n >= 256:
        cnt = np.diff(exp[4].astype(np.int64))
        stored = exp[2][:, :, 1].reshape(-1) > 0
        assert total > n and (cnt[stored] == 0).sum() >= 4 and (~stored).sum() >= 100, "every slot reports"
    cap = {"total": total, "total-1": total - 1, "zero-null": 0}[cap_name] if locate else 0
    if cap < 0:
        return  # (a batch with no location has no cap below its total)
    what = f"seeds n={n} cap={cap_name}({cap}) skew={skew} rev={reversed} locate={locate} stage_kb={stage_kb}"
    if tiles is not None:
        got = staged_tiles(pats, "forward", stage_kb, fixed_len, long_patterns)
        assert got == list(tiles), f"tiles staged by their offsets: {got}, expected {list(tiles)}"
    elif stage_kb:
        tile_bytes = [sum(len(p) for p in pats[t:t + 256]) for t in range(0, n, 256)]
        # (every full tile; the one-pattern last tile of a 257-pattern batch still fits)
        assert min(tile_bytes[:n // 256]) > 1024 * stage_kb, "a full tile fits the stage: not the unstaged path"
    P = np.uint32 if pb == 4 else np.uint64
    q = [p[::-1] for p in pats] if reversed else pats
    data, offsets = pkg.pack_patterns(q)
    arena = Arena(mem_cls)
    c = arena.carve
    S = n * ms
    if locate:
        wsb = ix.locate_workspace_size(S)
        c("ws", wsb, 16, 16, boundary=256)
    c("offsets", 8 * (n + 1), 8, 8, data=offsets)
    if locate:
        c("loc_offsets", 8 * (S + 1), 8, 8)
        c("needed", 8, 8, 8)
        if cap:
            # guard bytes for every location past cap: an emit that ignored cap stays inside the arena
            c("locs", pb * cap, pb, pb, tail=pb * max(total - cap, 0))
    c("nseeds", 4 * n, 4, 4)
    c("rest", 4 * n, 4, 4)
    c("spans", 8 * S, 4, 4)
    c("ranges", 2 * pb * S, pb, pb)
    c("bytes", data.size, 1, skew, data=data)
    arena.commit()
    off, nb = arena.bufs["bytes"]
    assert off + nb == arena.size - 4096, "the last pattern byte is not the byte before the end guard"
    p = arena.ptr
    assert p("bytes") % 16 == skew and p("spans") % 16 == 4 and p("nseeds") % 16 == 4 and p("ranges") % 16 == pb % 16
    kw = dict(max_seeds=ms, min_len=min_len, skip=skip, max_occ=max_occ, reversed=reversed, stage_kb=stage_kb,
              fixed_len=fixed_len, long_patterns=long_patterns)
    if locate:
        assert p("ws") % 256 == 16
        ix.seeds_batch_async(p("bytes"), p("offsets"), n, p("nseeds"), p("rest"), p("spans"), p("ranges"),
                             p("loc_offsets"), p("locs"), cap, p("needed"), p("ws"), wsb, **kw)
    else:
        ix.seeds_batch_async(p("bytes"), p("offsets"), n, p("nseeds"), p("rest"), p("spans"), p("ranges"), **kw)
    ix.sync()
    arena.image()
    arena.check_guards_and_inputs(what)
    v = arena.view
    assert np.array_equal(v("nseeds", np.uint32), exp[0]), f"{what}: d_nseeds"
    assert np.array_equal(v("rest", np.uint32), exp[1]), f"{what}: d_rest"
    assert np.array_equal(v("spans", np.uint32).reshape(n, ms, 2), exp[2]), f"{what}: d_spans"
    assert np.array_equal(v("ranges", P).reshape(n, ms, 2).astype(np.int64), exp[3]), f"{what}: d_ranges"
    if not locate:
        return
    assert np.array_equal(v("loc_offsets", np.uint64), exp[4]), f"{what}: d_loc_offsets"
    assert int(v("needed", np.uint64)[0]) == total, f"{what}: *d_needed"
    if cap:
        k = min(cap, total)
        assert np.array_equal(v("locs", P)[:k].astype(np.uint64), exp[5][:k]), f"{what}: d_locs[:min(cap, total)]"
        assert (v("locs", np.uint8)[k * pb:] == FILL_OUT).all(), f"{what}: d_locs written past min(cap, total)"
