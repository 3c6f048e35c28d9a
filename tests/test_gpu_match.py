"""Longest-suffix match on the GPU (fmx_match_batch: k_match, then the
locate's k_emit): the cases of tests/test_match_simt.py on the gfx950 kernels,
every layout, load options 0 (blob layout) and 1 (interleaved records), every
derived structure for two layouts (they must not change a result), forward
and reversed, batches of 1, 255, 256, 257 and 700 patterns.  Bodies and
expected values: _match_cases.py (the oracle's counts of growing suffixes, a
plainly sorted suffix list, the oracle's locate of the matched suffix)."""
import os

import pytest

import _match_cases as MC
from _util import ALL_LAYOUTS, TorchDev

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def sweep(pkg, O, case, pb, planes, vb, options):
    for occ in options:
        ix, orc = MC.open_index(pkg, O, case, pb, planes, vb, occ)
        for n in MC.BATCH_SIZES:
            pats = case.batch(n)
            exp = MC.check_match(pkg, ix, orc, case, pats)
            MC.check_match(pkg, ix, orc, case, pats, reversed=True)
            if n >= 256:
                MC.classes_and_full_match_check(ix, case, pats, exp)
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_match_every_layout(pkg, O, pb, planes, vb):
    sweep(pkg, O, MC.case_for(planes), pb, planes, vb, (0, 1))


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_match_ignores_derived_structures(pkg, O, pb, planes, vb):
    """FMX_OPT_DERIVED (deep table, full SA, text, row contexts, single-row
    entries): the match reads none of them (a loaded full SA serves the
    locations), and the answers are the same."""
    sweep(pkg, O, MC.case_for(planes), pb, planes, vb, (63,))


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_match_two_letters(pkg, O, sr):
    MC.two_letters(pkg, O, 700, sr, ((4, 64), (8, 32)))


@pytest.mark.parametrize("min_len", [1, 5])
@pytest.mark.parametrize("max_occ", [0, 1, 10, None])
def test_match_filters(pkg, O, min_len, max_occ):
    MC.filters(pkg, O, 700, min_len, max_occ)


def test_match_ranges_only_and_capacity(pkg, O):
    MC.ranges_only_and_capacity(pkg, O, 700)


def test_match_pass_through(pkg, O):
    MC.pass_through(pkg, O)


def test_match_async(pkg, O):
    """On HBM-resident buffers."""
    MC.device_call(pkg, O, TorchDev(), 700)
