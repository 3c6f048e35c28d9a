"""Guard bands around the strand launches of fmx_match_batch_async,
fmx_seeds_batch_async and fmx_approx_batch_async on the GPU: the runs of
tests/test_strands_guard_simt.py on the gfx950 kernels — every buffer of the
call carved out of ONE 0xA5-filled tensor at its exact 2n-shaped size and
weakest alignment, the whole tensor read back after every launch.

Nothing a correct or a broken strand kernel touches lies outside the tensor:
the guards are 4 KiB, a lane writes only its own virtual pattern's slots, the
staging loop reads only the 16-B lines the reads' bytes touch, and d_locs is
followed by guard bytes for every location past cap."""
import pytest

import _strand_cases as S
from _guard_cases import TorchMem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("skew", S.SKEWS)
@pytest.mark.parametrize("pb,planes,vb", S.GUARD_LAYOUTS)
@pytest.mark.parametrize("query", S.QUERIES)
def test_strands_guard(pkg, O, query, pb, planes, vb, skew):
    S.guard_runs(pkg, O, TorchMem, query, pb, planes, vb, skew)
