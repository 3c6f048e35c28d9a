"""Guard bands around fmx_approx_batch_async on the GPU: the run of
tests/_approx_guard_cases.py (as tests/test_approx_guard_simt.py has it on the
emulator) on the gfx950 kernels — every buffer of the call carved out of ONE
0xA5-filled tensor at its exact size and weakest alignment, the whole tensor
read back after every launch.  Pattern-byte skews 0, 1, 7 and 15, batches of
1, 257 and 700 patterns at max_mm = 2 and max_hits = 3, forward and reversed,
caps total, total - 1 and 0 with d_locs = NULL, intervals only, and the
unstaged path of k_approx (a 1 KB stage).

Nothing a correct or a broken k_approx touches lies outside the tensor: the
guards are 4 KiB, a lane writes only its own pattern's slots, and d_locs is
followed by guard bytes for every location past cap."""
import pytest

import _approx_guard_cases as AG
from _approx_cases import case_for, open_index
from _guard_cases import TorchMem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("skew", AG.SKEWS)
@pytest.mark.parametrize("pb,planes,vb", AG.LAYOUTS)
def test_approx_guard(pkg, O, pb, planes, vb, skew):
    case = case_for(planes)
    ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
    for n in AG.BATCH_SIZES:
        for rev in (False, True):
            for cap in AG.CAPS:
                AG.run_approx(pkg, ix, TorchMem, case, orc, pb, n, cap, skew, rev, best=cap == "total-1")
            AG.run_approx(pkg, ix, TorchMem, case, orc, pb, n, None, skew, rev, locate=False)
            if n > 256:  # the patterns read from HBM (no tile fits a 1 KB stage)
                AG.run_approx(pkg, ix, TorchMem, case, orc, pb, n, "total", skew, rev, stage_kb=1)
                AG.run_approx(pkg, ix, TorchMem, case, orc, pb, n, None, skew, rev, locate=False, stage_kb=1)
    ix.close()
