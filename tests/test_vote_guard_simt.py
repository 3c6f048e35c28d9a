"""Guard bands around fmx_vote_async on the CPU: the engine's own sources
under the SIMT shim (tests/simt), every buffer of the call carved at its exact
size and weakest alignment out of one 0xA5-filled array (_vote_cases.py, on
the arena of _guard_cases.py), d_locs exactly cap entries long with a chain
whose offsets reach past it: guards and inputs untouched, every output the
model's."""
import pytest

import _vote_cases as V
from _guard_cases import HostMem
from _seed_cases import case_for, open_index
from _simt import simt_fixture


simt = simt_fixture(launch_order=False)


@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_vote_guard_simt(pkg, O, simt, pb, planes, vb):
    simt.simt_config(8700 + pb, 0.5)
    ix, _ = open_index(pkg, O, case_for(planes), pb, planes, vb, 1)
    for n in (3, 257):
        for ms, band, mc, K in V.CONFIGS:
            V.run_vote_guard(pkg, ix, HostMem, pb, n, ms, band, mc, K)
    ix.close()
