"""Guard bands around the strand launches of fmx_match_batch_async,
fmx_seeds_batch_async and fmx_approx_batch_async on the CPU: the engine's own
sources under the SIMT shim (tests/simt), every buffer of the call carved at
its exact 2n-shaped size and weakest alignment out of one 0xA5-filled array
(_strand_cases.run_device, on the arena of _guard_cases.py as it stands),
pattern-byte skews 0, 1, 7 and 15, both flags, forward and reversed, caps
total, total - 1 and 0 with d_locs = NULL, ranges only, and the raw path (a
1 KB stage): guards and inputs untouched, every output the expected value,
d_locs[min(cap, total):cap] unwritten."""
import pytest

import _strand_cases as S
from _guard_cases import HostMem
from _simt import simt_fixture

simt = simt_fixture(launch_order=False)


@pytest.mark.parametrize("skew", S.SKEWS)
@pytest.mark.parametrize("pb,planes,vb", S.GUARD_LAYOUTS)
@pytest.mark.parametrize("query", S.QUERIES)
def test_strands_guard_simt(pkg, O, simt, query, pb, planes, vb, skew):
    simt.simt_config(9900 + pb + planes + skew, 0.5)
    S.guard_runs(pkg, O, HostMem, query, pb, planes, vb, skew)
