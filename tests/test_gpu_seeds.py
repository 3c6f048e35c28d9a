"""Greedy seed chains on the GPU (fmx_seeds_batch: k_seeds, then the locate's
k_emit over the slots): the cases of tests/test_seeds_simt.py on the gfx950
kernels — every layout and load options 0 and 1 at max_seeds = 3, max_seeds 1
and 8 and every derived structure (63: they must not change a result) for two
layouts, skip 0 and 1, forward and reversed, batches of 1, 255, 256, 257 and
700 patterns.  Bodies and expected values: _seed_cases.py (the loop of
include/fmx.h run in Python over _match_cases.Case.expected)."""
import os

import numpy as np
import pytest

import _seed_cases as SC
from _util import ALL_LAYOUTS, TorchDev

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def sweep(pkg, O, case, pb, planes, vb, options, seed_counts):
    for occ in options:
        ix, orc = SC.open_index(pkg, O, case, pb, planes, vb, occ)
        for n in SC.BATCH_SIZES:
            pats = SC.batch(case, n)
            if n >= 256 and occ == options[0]:  # (on the expected values alone, before anything is compared)
                SC.assert_classes(case, orc, pats, 0)
                SC.assert_classes(case, orc, pats, 1)
            for ms in seed_counts:
                for skip in (0, 1):
                    _, got = SC.check_seeds(ix, orc, case, pats, max_seeds=ms, skip=skip, reversed=skip == 0)
                    SC.check_seeds(ix, orc, case, pats, max_seeds=ms, skip=skip, reversed=skip == 1)
                if n >= 256:
                    SC.cross_check(ix, pats, got)
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_seeds_every_layout(pkg, O, pb, planes, vb):
    sweep(pkg, O, SC.case_for(planes), pb, planes, vb, (0, 1), (3,))


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_seeds_slot_counts(pkg, O, pb, planes, vb):
    """max_seeds = 1: parsing stops after one seed with rest exact; 8: the
    20-seed pattern runs out of slots."""
    case = SC.case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (1,), (1, 8))
    ix, orc = SC.open_index(pkg, O, case, pb, planes, vb, 1)
    pats = SC.batch(case, 700)
    for ms in (1, 8):
        exp = SC.expected_arrays(case, orc, pats, ms, 1, 0, None)
        assert (exp[1] > 0).sum() >= (30 if ms == 1 else 1), "no pattern ran out of slots"
    ix.close()


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_seeds_ignore_derived_structures(pkg, O, pb, planes, vb):
    """FMX_OPT_DERIVED (deep table, full SA, text, row contexts, single-row
    entries): the search reads none of them (a loaded full SA serves the
    locations), and the results are identical."""
    case = SC.case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (63,), (3,))
    pats = SC.batch(case, 700)
    outs = []
    for occ in (1, 63):
        ix, _ = SC.open_index(pkg, O, case, pb, planes, vb, occ)
        outs.append(ix.seeds_batch(pats, max_seeds=3, skip=1))
        ix.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_seeds_two_letters(pkg, O, sr):
    SC.two_letters(pkg, O, 700, sr, ((4, 64), (8, 32)))


@pytest.mark.parametrize("min_len", [1, 5])
def test_seeds_filters(pkg, O, min_len):
    SC.filters(pkg, O, 700, min_len)


def test_seeds_ranges_only_and_capacity(pkg, O):
    SC.ranges_only_and_capacity(pkg, O, 700)


def test_seeds_pass_through(pkg, O):
    SC.pass_through(pkg, O)


def test_seeds_async(pkg, O):
    """On HBM-resident buffers."""
    SC.device_call(pkg, O, TorchDev(), 700)
