"""Greedy seed chains (fmx_seeds_batch: k_seeds, then the locate's k_emit over
the slots) on the CPU: the engine's own sources under the SIMT shim
(tests/simt, as tests/test_match_simt.py), every output against the values of
_seed_cases.py — the loop of include/fmx.h run in Python over
_match_cases.Case.expected.  Batches of 1, 255, 256, 257 and 700 patterns,
max_seeds 1, 3 and 8 (3: pattern 85's slots straddle the first tile boundary, a
257-pattern batch ends in a 3-slot tile), skip 0 and 1, forward and reversed;
min_len / max_occ; a two-letter text (hundreds of rows per seed); ranges only;
capacity; PassThrough bytes; the device call; argument checks.  The bodies are
_seed_cases.py's, shared with tests/test_gpu_seeds.py."""
import pytest

import _seed_cases as SC
from _simt import simt_fixture
from _util import SIMT_LAYOUTS, HostDev


simt = simt_fixture(launch_order=True)


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", SIMT_LAYOUTS)
def test_seeds_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 131 + planes * 17 + vb + n + 3, 0.5)
    case = SC.case_for(planes)
    pats = SC.batch(case, n)
    for occ in (0, 1):
        ix, orc = SC.open_index(pkg, O, case, pb, planes, vb, occ)
        if n >= 256 and occ == 0:
            SC.assert_classes(case, orc, pats, 0)
            SC.assert_classes(case, orc, pats, 1)
        _, got = SC.check_seeds(ix, orc, case, pats, max_seeds=3, skip=occ)
        SC.check_seeds(ix, orc, case, pats, max_seeds=3, skip=1 - occ, reversed=True)
        if n >= 256 and occ == 1:
            SC.cross_check(ix, pats, got)
        ix.close()


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
@pytest.mark.parametrize("max_seeds", [1, 8])
def test_seeds_slot_counts_simt(pkg, O, simt, max_seeds, n):
    """max_seeds = 1: parsing stops after one seed with rest exact; 8: the
    20-seed pattern runs out of slots."""
    simt.simt_config(max_seeds * 1009 + n, 0.5)
    case = SC.case_for(3)
    ix, orc = SC.open_index(pkg, O, case, 4, 3, 64, 1)
    pats = SC.batch(case, n)
    for skip, rev in ((0, False), (1, True)):
        exp, _ = SC.check_seeds(ix, orc, case, pats, max_seeds=max_seeds, skip=skip, reversed=rev)
        if n >= 256:
            assert (exp[1] > 0).sum() >= (30 if max_seeds == 1 else 1), "no pattern ran out of slots"
    ix.close()


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_seeds_two_letters_simt(pkg, O, simt, sr):
    simt.simt_config(1900 + sr, 0.5)
    SC.two_letters(pkg, O, 257, sr, ((4, 64),))


@pytest.mark.parametrize("min_len", [1, 5])
def test_seeds_filters_simt(pkg, O, simt, min_len):
    simt.simt_config(177 + min_len, 0.5)
    SC.filters(pkg, O, 257, min_len)


def test_seeds_ranges_only_and_capacity_simt(pkg, O, simt):
    simt.simt_config(5252, 0.5)
    SC.ranges_only_and_capacity(pkg, O, 300)  # (a batch of 300 ends with the 20-seed pattern)


def test_seeds_pass_through_simt(pkg, O, simt):
    simt.simt_config(707, 0.5)
    SC.pass_through(pkg, O)


def test_seeds_async_simt(pkg, O, simt):
    """On the emulator, device memory is host memory."""
    simt.simt_config(616, 0.5)
    SC.device_call(pkg, O, HostDev(), 300)
