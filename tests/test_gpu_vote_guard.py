"""Guard bands around fmx_vote_async on the GPU: the run of
tests/_vote_cases.py (run_vote_guard, as tests/test_vote_guard_simt.py has it
on the emulator) on the gfx950 kernel — every buffer of the call carved out of
ONE 0xA5-filled tensor at its exact size and weakest alignment, d_locs exactly
cap entries long with a chain whose offsets reach past it, the whole tensor
read back after the launch.

Nothing a correct or a broken k_vote touches lies far outside its buffers: a
wave reads its own chain's slots and at most 1,024 locations below cap and
writes its own chain's outputs; the guards are 4 KiB."""
import pytest

import _vote_cases as V
from _guard_cases import TorchMem
from _seed_cases import case_for, open_index

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_vote_guard(pkg, O, pb, planes, vb):
    ix, _ = open_index(pkg, O, case_for(planes), pb, planes, vb, 1)
    for n in (3, 257):
        for ms, band, mc, K in V.CONFIGS:
            V.run_vote_guard(pkg, ix, TorchMem, pb, n, ms, band, mc, K)
    ix.close()
