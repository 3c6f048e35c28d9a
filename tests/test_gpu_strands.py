"""Both strands (FMX_PATTERN_REVCOMP / FMX_BOTH_STRANDS on match, seeds and
approx) on the gfx950 kernels: the cases of tests/_strand_cases.py (as
tests/test_strands_simt.py runs them on the emulator) on every layout with
load options 0 and 1 at max_seeds = max_hits = 3, every derived structure on
two layouts, the raw path and fixed-length reads from device calls, the
two-letter text and a map that is no involution.  Every answer against the
existing references run on the expanded batch built in Python, and against the
engine's own flag-less call on it."""
import os

import pytest

import _strand_cases as S
from _guard_cases import TorchMem
from _seed_cases import case_for, open_index
from _util import ALL_LAYOUTS

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")

# (reversed, locate) per load option: each direction with locations and ranges only across the two
PASSES = {0: ((False, True), (True, False)), 1: ((True, True), (False, False)), 63: ((False, True), (True, True))}


def sweep(pkg, O, case, cmap, pb, planes, vb, options, shapes):
    for occ in options:
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        ix.set_complement(cmap)
        for strands, n in shapes:
            reads = S.reads_for(case, cmap, n)
            for query in S.QUERIES:
                for rev, loc in PASSES[occ]:
                    S.check(ix, orc, case, query, reads, cmap, strands, reversed=rev, locate=loc)
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_strands_every_layout(pkg, O, pb, planes, vb):
    case = case_for(planes)
    sweep(pkg, O, case, S.involution(case), pb, planes, vb, (0, 1),
          [("both", n) for n in S.BOTH_SIZES] + [("reverse", n) for n in S.RC_SIZES])


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_strands_ignore_derived_structures(pkg, O, pb, planes, vb):
    case = case_for(planes)
    sweep(pkg, O, case, S.involution(case), pb, planes, vb, (63,), [("both", 300), ("reverse", 257)])


@pytest.mark.parametrize("query", S.QUERIES)
def test_strands_not_an_involution(pkg, O, query):
    case = case_for(3)
    cmap = S.cycle_map(case)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    ix.set_complement(cmap)
    S.check(ix, orc, case, query, S.reads_for(case, cmap, 129), cmap, "both")
    S.check(ix, orc, case, query, S.reads_for(case, cmap, 257), cmap, "reverse", reversed=True)
    ix.close()


@pytest.mark.parametrize("query", S.QUERIES)
def test_strands_two_letters(pkg, O, query):
    case = case_for(2, two_letters=True, k=3, sr=2)
    cmap = S.involution(case)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    ix.set_complement(cmap)
    S.check(ix, orc, case, query, S.reads_for(case, cmap, 129), cmap, "both")
    ix.close()


def test_strands_approx_two_mismatches_best(pkg, O):
    case = case_for(3)
    cmap = S.involution(case)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    ix.set_complement(cmap)
    S.check(ix, orc, case, "approx", S.reads_for(case, cmap, 129), cmap, "both", max_mm=2, best=True)
    ix.close()


@pytest.mark.parametrize("strands,n", [("both", 300), ("both", 129), ("reverse", 257)])
@pytest.mark.parametrize("query", S.QUERIES)
def test_strands_device_calls(pkg, O, query, strands, n):
    """Device calls: the raw path (a 1 KB stage, d_bytes at an odd address),
    fixed-length reads with the hint, and a hint the offsets disagree with."""
    for pb, planes, vb in ((4, 3, 64), (8, 4, 64)):
        case = case_for(planes)
        cmap = S.involution(case)
        ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
        ix.set_complement(cmap)
        reads, fixed = S.reads_for(case, cmap, n), S.reads_for(case, cmap, n, fixed=True)
        for rev in (False, True):
            S.run_device(pkg, ix, TorchMem, case, orc, pb, query, reads, cmap, strands, reversed=rev, skew=1,
                         stage_kb=1)
            S.run_device(pkg, ix, TorchMem, case, orc, pb, query, fixed, cmap, strands, reversed=rev,
                         fixed_len=S.FIXED_M)
        with pytest.raises(pkg.FmxError) as e:
            S.run_device(pkg, ix, TorchMem, case, orc, pb, query, fixed, cmap, strands, fixed_len=S.FIXED_M - 1)
        assert e.value.code == pkg._native.FMX_E_ARG
        ix.close()
