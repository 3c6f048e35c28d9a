"""Guard bands around the device-buffer API on the CPU: the engine's own
sources under the SIMT shim (tests/simt, as tests/test_simt.py), every buffer
of a call carved at its exact size and weakest allowed alignment out of one
0xA5-filled array (tests/_guard_cases.py), and after every launch the whole
array compared with what include/fmx.h allows it to be: guards and inputs
untouched, offsets / needed / counts / lens / ranges the oracle's, the
location prefix the oracle's, d_locs[min(cap, total):cap] unwritten.

Every launch path (split, fused, grouped with packed and with id-only
records, chained emit; fmx_index_info's counters asserted), the group call,
the match with and without locations and the count, at every d_bytes skew (0,
1, 7, 15 past a 16-B boundary) and every cap (total, total-1, inside a heavy
pattern's run mid-wave, on a pattern boundary, 1, 0 with d_locs = NULL),
batch sizes, direction and batch shape rotating through them, every path
under two emulator schedules; layouts (4,3,64), (8,3,128) and (4,5,64) with 21 symbols,
load options 0 and 1, and every derived structure (63) for (4,3,64) in launch
order (a grouped launch needs the faithful index).  Host calls: the capacity
contract of fmx_locate_batch and fmx_match_batch."""
import itertools

import pytest

import _guard_cases as G
from _simt import simt_fixture

SEEDS = (0, 1)


simt = simt_fixture(launch_order=False)


@pytest.fixture
def fused(simt):
    """As tests/test_simt.py: the fused launch and the chained emit run with
    workgroups in a shuffled order (their tickets make that safe); the
    environment itself is set per path by _guard_cases.open_index."""
    simt.simt_block_order(0)
    yield simt


def seeded(params):
    """Every case under the first emulator schedule, the default index
    (options 1) of every path and layout under the second as well."""
    return [(p, seed) for p in params for seed in SEEDS if seed == 0 or p[-1] == 1]


@pytest.mark.parametrize("param,seed", seeded(G.LOCATE_PARAMS), ids=G.ids)
def test_locate_guard_simt(pkg, O, simt, fused, monkeypatch, param, seed):
    """fmx_locate_batch_async / fmx_locate_jobs_async on one path: every skew
    x every cap, the batch shape, size and direction rotating."""
    path, pb, planes, vb, nch, opt = param
    simt.simt_config(9000 + 31 * seed + pb + planes + opt, 0.5)
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, path)
    shapes = G.shapes_for(path, opt)
    if opt == 63:
        G.assert_scan_live(ix, case, orc, path)
    for (si, skew), (ci, cap) in itertools.product(enumerate(G.SKEWS), enumerate(G.CAP_NAMES)):
        # the first (shape, size) in rotated order whose batch has this cap
        cands = [(shapes[(si + ci + a) % len(shapes)], G.BATCH_SIZES[(2 * ci + si + seed + b) % 5])
                 for b in range(5) for a in range(len(shapes))]
        for shape, n in cands:
            if G.run_locate(pkg, ix, G.HostMem, case, orc, pb, path, shape, n, cap, skew, (si + ci + seed) % 2 == 1,
                            via_jobs=(si + ci) % 3 == 0):
                break
        else:
            raise AssertionError(f"no batch with cap {cap}")
    ix.close()


GROUP_PARAMS = [(path,) + ixp for path in G.PATHS for ixp in G.INDEXES if ixp[4] == 1]


@pytest.mark.parametrize("param,seed", seeded(GROUP_PARAMS), ids=G.ids)
def test_group_guard_simt(pkg, O, simt, fused, monkeypatch, param, seed):
    """fmx_locate_group_async: five batches with their own caps and
    workspaces in one arena, at every skew, forward and reversed."""
    path, pb, planes, vb, nch, opt = param
    simt.simt_config(9500 + 31 * seed + pb + planes, 0.5)
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, path)
    for si, skew in enumerate(G.SKEWS):
        G.run_group(pkg, ix, G.HostMem, case, orc, pb, path, skew, (si + seed) % 2 == 1)
    ix.close()


@pytest.mark.parametrize("ixp,seed", seeded(G.INDEXES), ids=G.ids)
def test_match_and_count_guard_simt(pkg, O, simt, monkeypatch, ixp, seed):
    """fmx_match_batch_async with locations (every skew x every cap) and
    without (no location buffers, no workspace), fmx_count_batch_async."""
    pb, planes, vb, nch, opt = ixp
    simt.simt_config(9700 + 31 * seed + pb + planes + opt, 0.5)
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, "split")
    for (si, skew), (ci, cap) in itertools.product(enumerate(G.SKEWS), enumerate(G.CAP_NAMES)):
        if cap == "mid-run" and nch > 8:
            continue  # (no reporting match of a 21-symbol text has a hundred occurrences)
        for b in range(5):
            if G.run_match(pkg, ix, G.HostMem, case, orc, pb, G.BATCH_SIZES[(2 * ci + si + seed + b) % 5], cap, skew,
                           (si + ci + seed) % 2 == 1):
                break
        else:
            raise AssertionError(f"no batch with cap {cap}")
    for si, skew in enumerate(G.SKEWS):
        for j, n in enumerate(G.BATCH_SIZES):
            rev = (si + j + seed) % 2 == 1
            G.run_match(pkg, ix, G.HostMem, case, orc, pb, n, None, skew, rev, locate=False)
            shape = ("ragged", "single", "heavy")[(si + j) % 3]
            G.run_count(pkg, ix, G.HostMem, case, orc, pb, shape, n, skew, rev, fixed=(si + j) % 2 == 0)
    ix.close()


@pytest.mark.parametrize("match", [False, True], ids=["locate", "match"])
@pytest.mark.parametrize("pb,planes,vb,nch", [lay for lay in G.LAYOUTS if lay[3] == 4], ids=G.ids)
def test_host_capacity_simt(pkg, O, simt, monkeypatch, pb, planes, vb, nch, match):
    """FMX_E_CAPACITY of the host-buffer calls: needed and offsets written,
    out_locs untouched; then the exact cap on the same index (two passes)."""
    simt.simt_config(9900 + pb, 0.5)
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, 1, "split")
    G.check_host_capacity(pkg, ix, case, orc, pb, match=match)
    ix.close()
