"""k-mismatch search on the GPU (fmx_approx_batch: k_approx, then the locate's
k_emit over the slots): the cases of tests/test_approx_simt.py on the gfx950
kernels — every layout and load options 0 and 1 at max_hits = 3, max_hits 1
and 8 and every derived structure (63: they must not change a result) for two
layouts, max_mm 0..3, FMX_APPROX_BEST, forward and reversed, batches of 1, 255,
256, 257 and 700 patterns, a two-letter text at sampling ratios 1..4, the
unstaged pattern path and a caller's stream.  Bodies and expected values: the
brute force of _approx_cases.py."""
import os

import numpy as np
import pytest

import _approx_cases as AC
from _util import ALL_LAYOUTS, TorchDev

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def sweep(pkg, O, case, pb, planes, vb, options, hit_counts):
    for occ in options:
        ix, orc = AC.open_index(pkg, O, case, pb, planes, vb, occ)
        for n in AC.BATCH_SIZES:
            p1, p2 = AC.batch(case, n, 1), AC.batch(case, n, 2)
            for mh in hit_counts:
                if n >= 256 and occ == options[0]:  # (on the expected values alone, before anything is compared)
                    AC.assert_classes(case, orc, p1, 1, mh)
                    AC.assert_classes(case, orc, p2, 2, mh)
                _, got = AC.check_approx(ix, orc, case, p1, max_mm=1, max_hits=mh, best=mh == 1)
                AC.check_approx(ix, orc, case, p2, max_mm=2, max_hits=mh, best=mh != 1, reversed=True)
            if n == 257:
                AC.cross_check(ix, case, p1, got)
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_approx_every_layout(pkg, O, pb, planes, vb):
    sweep(pkg, O, AC.case_for(planes), pb, planes, vb, (0, 1), (3,))


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_approx_slot_counts(pkg, O, pb, planes, vb):
    """max_hits = 1: the search stops at the second variant; 8: the classes
    of the issue; max_mm = 0 is the exact search; max_mm = 3 on patterns of at
    most 12 symbols."""
    case = AC.case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (1,), (1, 8))
    ix, orc = AC.open_index(pkg, O, case, pb, planes, vb, 1)
    pats = AC.batch(case, 700, 0)
    _, got = AC.check_approx(ix, orc, case, pats, max_mm=0, max_hits=1)
    AC.cross_check_exact(ix, pats, got)
    for best in (False, True):
        AC.three_mismatches(ix, orc, case, best)
    ix.close()


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_approx_ignore_derived_structures(pkg, O, pb, planes, vb):
    """FMX_OPT_DERIVED (deep table, full SA, text, row contexts, single-row
    entries): the search reads none of them (a loaded full SA serves the
    locations), and the results are identical."""
    case = AC.case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (63,), (3,))
    pats = AC.batch(case, 700, 2)
    outs = []
    for occ in (1, 63):
        ix, _ = AC.open_index(pkg, O, case, pb, planes, vb, occ)
        outs.append(ix.approx_batch(pats, max_mm=2, max_hits=3))
        ix.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("sr", [1, 2, 3, 4])
def test_approx_two_letters(pkg, O, sr):
    AC.two_letters(pkg, O, 700, sr, ((4, 64), (8, 32)))


def test_approx_filters(pkg, O):
    AC.filters(pkg, O, 700)


def test_approx_ranges_only_and_capacity(pkg, O):
    AC.ranges_only_and_capacity(pkg, O, 700)


def test_approx_pass_through(pkg, O):
    AC.pass_through(pkg, O)


def test_approx_unstaged_patterns(pkg, O):
    """A 1 KB stage: no full tile of the batch fits, so k_approx reads every
    pattern from HBM, forward and reversed."""
    case = AC.case_for(3, k=3, sr=2)
    ix, orc = AC.open_index(pkg, O, case, 4, 3, 64, 1)
    pats = AC.batch(case, 700, 2)
    assert min(sum(len(p) for p in pats[t:t + 256]) for t in (0, 256)) > 1024
    exp = AC.expected_arrays(case, orc, pats, 2, 3, False, 10)
    AC.device_call(pkg, TorchDev(), ix, pats, exp, 3, max_mm=2, max_occ=10, stage_kb=1)
    AC.device_call(pkg, TorchDev(), ix, [p[::-1] for p in pats], exp, 3, max_mm=2, max_occ=10, stage_kb=1,
                   reversed=True)
    ix.close()


def test_approx_async_on_a_caller_stream(pkg, O):
    """On HBM-resident buffers and a stream of the caller's."""
    AC.async_call(pkg, O, TorchDev(caller_stream=True), 700)
