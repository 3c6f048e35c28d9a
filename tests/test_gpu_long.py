"""match, seeds, approx and the strand flags on reads of mapper length, on the
gfx950 kernels: the cases of tests/_long_cases.py (as tests/test_long_simt.py
runs them on the emulator).  Every answer against the existing references (and
a strand call against the engine's flag-less call on the expanded list), every
device call through the guard-band runners with d_bytes at an odd address.

  1. the ragged 100-300 symbol batches from host calls on the random and the
     repeat text: 300 reads flag-less and FMX_PATTERN_REVCOMP, 129 and 300
     FMX_BOTH_STRANDS, every layout with load options 0 and 1, every derived
     structure on two layouts;
  2. the stage edge: 224 and 225 symbols under FMX_HINT_STAGE_KB(56) and the
     fixed-length hint (257 + 44 reads, 129 + 22 under both strands), 150
     under both strands (the 38,400 B stage);
  3. the four hint forms on the ragged batch (513 reads; 300 under both strands);
  4. the two-letter text with 4^5 k-mer entries at 224 symbols: the largest
     dynamic LDS request, 57,344 + 4,096 B, must launch;
  5. reads of 65,535 and 65,536 symbols: the fixed-length hint's limit."""
import os

import pytest

import _long_cases as LC
import _strand_cases as S
from _guard_cases import TorchMem
from _util import ALL_LAYOUTS

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")

# (reversed, locate) per load option: each direction with locations and ranges only across the two
PASSES = {0: ((False, True), (True, False)), 1: ((True, True), (False, False)), 63: ((False, True), (True, True))}
QUERY_KW = (("match", LC.MATCH), ("seeds", LC.SEEDS), ("approx", LC.APPROX))
QUERY_IDS = [q for q, _ in QUERY_KW]


# ------------------------------------------------------------------- 1. sweep

@pytest.mark.parametrize("occ", (0, 1))
@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
@pytest.mark.parametrize("text", sorted(LC.TEXTS))
def test_long_sweep(pkg, O, text, pb, planes, vb, occ):
    LC.sweep(pkg, O, text, pb, planes, vb, occ, PASSES[occ])


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
@pytest.mark.parametrize("text", sorted(LC.TEXTS))
def test_long_sweep_ignores_derived_structures(pkg, O, text, pb, planes, vb):
    LC.sweep(pkg, O, text, pb, planes, vb, 63, PASSES[63])


def test_long_approx_two_mismatches_best(pkg, O):
    """max_mm = 2 with FMX_APPROX_BEST on 150-symbol reads of the repeat text."""
    case = LC.repeat_case(3)
    cmap = S.involution(case)
    ix, orc = LC.open_index(pkg, O, case, cmap, 4, 3, 64, 1)
    LC.check(ix, orc, case, "approx", LC.reads_for(case, cmap, 301, 150), cmap, "forward", **LC.APPROX_MM2)
    LC.check(ix, orc, case, "approx", LC.reads_for(case, cmap, 151, 150), cmap, "both", reversed=True,
             **LC.APPROX_MM2)
    ix.close()


@pytest.mark.parametrize("query,kw", QUERY_KW, ids=QUERY_IDS)
def test_long_fixed_300(pkg, O, query, kw):
    """Reads of exactly 300 symbols: whole matches, seeds and variants at the longest length."""
    case = LC.repeat_case(3)
    cmap = S.involution(case)
    ix, orc = LC.open_index(pkg, O, case, cmap, 4, 3, 64, 1)
    LC.check(ix, orc, case, query, LC.reads_for(case, cmap, 301, 300), cmap, "forward", **kw)
    LC.check(ix, orc, case, query, LC.reads_for(case, cmap, 151, 300), cmap, "both", reversed=True, **kw)
    ix.close()


# -------------------------------------------------------------- 2. stage edge

@pytest.mark.parametrize("m", (224, 225))
@pytest.mark.parametrize("strands,n", LC.EDGE_SHAPES)
@pytest.mark.parametrize("pb,planes,vb", LC.EDGE_LAYOUTS)
@pytest.mark.parametrize("query,kw", QUERY_KW, ids=QUERY_IDS)
def test_long_stage_edge(pkg, O, query, kw, pb, planes, vb, strands, n, m):
    LC.stage_edge(pkg, O, TorchMem, pb, planes, vb, query, kw, strands, n, m)


@pytest.mark.parametrize("query,kw", QUERY_KW, ids=QUERY_IDS)
def test_long_strand_stage_150(pkg, O, query, kw):
    """150 symbols under both strands with the fixed-length hint: the stage is
    256 x 150 = 38,400 B, which both copies of 128 reads fill exactly."""
    assert S.stage_bytes_of("both", 56, 150) == 38400
    LC.stage_edge(pkg, O, TorchMem, 4, 3, 64, query, kw, "both", 129 + 22, 150)


# -------------------------------------------------------------- 3. hint forms

@pytest.mark.parametrize("strands,n", (("forward", 513), ("reverse", 513), ("both", 300)))
@pytest.mark.parametrize("query,kw", QUERY_KW, ids=QUERY_IDS)
def test_long_hint_forms(pkg, O, query, kw, strands, n):
    for pb, planes, vb in LC.EDGE_LAYOUTS:
        LC.hint_forms(pkg, O, TorchMem, pb, planes, vb, query, kw, strands, n)


# -------------------------------------------------------- 4. largest LDS request

@pytest.mark.parametrize("strands,n", (("forward", 257 + 44), ("both", 129 + 22)))
@pytest.mark.parametrize("pb", (4, 8))
@pytest.mark.parametrize("query,kw", QUERY_KW, ids=QUERY_IDS)
def test_long_largest_lds(pkg, O, query, kw, pb, strands, n):
    LC.largest_lds(pkg, O, TorchMem, pb, query, kw, strands, n)


# ---------------------------------------------------- 5. fixed-length hint limit

def test_long_hint_limit(pkg, O):
    LC.hint_limit(pkg, O)
