"""k-mismatch search (fmx_approx_batch: k_approx, then the locate's k_emit over
the slots) on the CPU: the engine's own sources under the SIMT shim
(tests/simt, as tests/test_seeds_simt.py), every output against the brute-force
values of _approx_cases.py.  Batches of 1, 255, 256, 257 and 700 patterns,
max_mm 0..2 (3 on patterns of at most 12 symbols), max_hits 1, 3 and 8 (3:
pattern 85's slots straddle the first tile boundary), forward and reversed,
FMX_APPROX_BEST; max_occ; a two-letter text (more than 32 variants per pattern);
ranges only; capacity; PassThrough bytes; the device call; argument checks.
The bodies are _approx_cases.py's, shared with tests/test_gpu_approx.py."""
import pytest

import _approx_cases as AC
from _simt import simt_fixture
from _util import SIMT_LAYOUTS, HostDev


simt = simt_fixture(launch_order=True)


@pytest.mark.parametrize("n", AC.BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", SIMT_LAYOUTS)
def test_approx_simt(pkg, O, simt, pb, planes, vb, n):
    """max_mm = 1 forward and max_mm = 2 reversed with FMX_APPROX_BEST, three
    slots per pattern, both occ layouts."""
    simt.simt_config(pb * 131 + planes * 17 + vb + n + 5, 0.5)
    case = AC.case_for(planes)
    for occ in (0, 1):
        ix, orc = AC.open_index(pkg, O, case, pb, planes, vb, occ)
        p1, p2 = AC.batch(case, n, 1), AC.batch(case, n, 2)
        if n >= 256 and occ == 0:
            AC.assert_classes(case, orc, p1, 1, 3)
            AC.assert_classes(case, orc, p2, 2, 3)
        _, got = AC.check_approx(ix, orc, case, p1, max_mm=1, max_hits=3, best=bool(occ))
        AC.check_approx(ix, orc, case, p2, max_mm=2, max_hits=3, best=not occ, reversed=True)
        if n == 257 and occ == 1:
            AC.cross_check(ix, case, p1, got)
        ix.close()


@pytest.mark.parametrize("n", AC.BATCH_SIZES)
@pytest.mark.parametrize("max_hits", [1, 8])
def test_approx_slot_counts_simt(pkg, O, simt, max_hits, n):
    """max_hits = 1: the search stops at the second variant; 8: the classes
    of the issue; max_mm = 0 is the exact search."""
    simt.simt_config(max_hits * 1013 + n, 0.5)
    case = AC.case_for(3)
    ix, orc = AC.open_index(pkg, O, case, 4, 3, 64, 1)
    for max_mm, rev in ((1, False), (2, True)):
        pats = AC.batch(case, n, max_mm)
        if n >= 256:
            AC.assert_classes(case, orc, pats, max_mm, max_hits)
        AC.check_approx(ix, orc, case, pats, max_mm=max_mm, max_hits=max_hits, reversed=rev)
    pats = AC.batch(case, n, 0)
    _, got = AC.check_approx(ix, orc, case, pats, max_mm=0, max_hits=max_hits)
    if max_hits == 1:
        AC.cross_check_exact(ix, pats, got)
    ix.close()


@pytest.mark.parametrize("best", [False, True])
def test_approx_three_mismatches_simt(pkg, O, simt, best):
    simt.simt_config(333 + best, 0.5)
    case = AC.case_for(3)
    ix, orc = AC.open_index(pkg, O, case, 4, 3, 64, 1)
    AC.three_mismatches(ix, orc, case, best)
    ix.close()


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_approx_two_letters_simt(pkg, O, simt, sr):
    simt.simt_config(2900 + sr, 0.5)
    AC.two_letters(pkg, O, 257, sr, ((4, 64),))


def test_approx_filters_simt(pkg, O, simt):
    simt.simt_config(178, 0.5)
    AC.filters(pkg, O, 257)


def test_approx_ranges_only_and_capacity_simt(pkg, O, simt):
    simt.simt_config(5253, 0.5)
    AC.ranges_only_and_capacity(pkg, O, 300)


def test_approx_pass_through_simt(pkg, O, simt):
    simt.simt_config(708, 0.5)
    AC.pass_through(pkg, O)


def test_approx_async_simt(pkg, O, simt):
    """On the emulator, device memory is host memory."""
    simt.simt_config(617, 0.5)
    AC.async_call(pkg, O, HostDev(), 300)
