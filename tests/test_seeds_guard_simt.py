"""Guard bands around fmx_seeds_batch_async on the CPU: the engine's own
sources under the SIMT shim (tests/simt), every buffer of the call carved at
its exact size and weakest alignment out of one 0xA5-filled array
(_seed_guard_cases.py, on the arena of _guard_cases.py), pattern-byte skews 0,
1, 7 and 15, batches of 1, 257 and 700 patterns at max_seeds = 3, caps total,
total - 1 and 0 with d_locs = NULL, and spans and ranges only (no workspace,
no location buffers), and the unstaged path (a 1 KB stage): guards and inputs
untouched, every output the expected value, d_locs[min(cap, total):cap]
unwritten."""

import pytest

import _seed_guard_cases as SG
from _guard_cases import HostMem
from _seed_cases import case_for, open_index
from _simt import simt_fixture


simt = simt_fixture(launch_order=False)


@pytest.mark.parametrize("skew", SG.SKEWS)
@pytest.mark.parametrize("pb,planes,vb", SG.LAYOUTS)
def test_seeds_guard_simt(pkg, O, simt, pb, planes, vb, skew):
    simt.simt_config(9800 + pb + planes + skew, 0.5)
    case = case_for(planes)
    ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
    for j, n in enumerate(SG.BATCH_SIZES):
        for ci, cap in enumerate(SG.CAPS):
            SG.run_seeds(pkg, ix, HostMem, case, orc, pb, n, cap, skew, (j + ci + skew) % 2 == 1)
        SG.run_seeds(pkg, ix, HostMem, case, orc, pb, n, None, skew, (j + skew) % 2 == 0, locate=False)
        if n > 256:  # the patterns read from HBM (no tile fits a 1 KB stage), both directions
            for rev in (False, True):
                SG.run_seeds(pkg, ix, HostMem, case, orc, pb, n, "total", skew, rev, stage_kb=1)
    ix.close()
