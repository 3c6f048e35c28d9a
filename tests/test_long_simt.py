"""match, seeds, approx and the strand flags on reads of mapper length, on the
CPU: the engine's own sources under the SIMT shim (tests/simt), the cases of
tests/_long_cases.py.  Every answer against the existing references (and a
strand call against the engine's flag-less call on the expanded list), every
device call through the guard-band runners with d_bytes at an odd address.

  1. the ragged 100-300 symbol batches from host calls on the random and the
     repeat text: 300 reads flag-less and FMX_PATTERN_REVCOMP, 129 and 300
     FMX_BOTH_STRANDS, the four layouts of _strand_cases with load options 0
     and 1, each direction with locations and ranges only;
  2. the stage edge: 224 and 225 symbols under FMX_HINT_STAGE_KB(56) and the
     fixed-length hint (257 + 44 reads, 129 + 22 under both strands), 150
     under both strands (the 38,400 B stage);
  3. the four hint forms on the ragged batch (513 reads; 300 under both strands);
  4. the two-letter text with 4^5 k-mer entries at 224 symbols: the largest
     dynamic LDS request, 57,344 + 4,096 B;
  5. reads of 65,535 and 65,536 symbols: the fixed-length hint's limit.

The emulator logs every launch's dynamic LDS request and how many bytes of it
each workgroup wrote (simt_lds_log), so cases 2 to 4 also assert what the
kernel did with each tile: a staged tile wrote its span (both copies under
both strands), a raw one nothing but the k-mer table."""
import ctypes as C

import pytest

import _long_cases as LC
import _strand_cases as S
from _guard_cases import HostMem
from _simt import simt_fixture

simt = simt_fixture(launch_order=True)

# (reversed, locate) per load option: each direction with locations and ranges only across the two
PASSES = {0: ((False, True), (True, False)), 1: ((True, True), (False, False))}
QUERY_KW = (("match", LC.MATCH), ("seeds", LC.SEEDS), ("approx", LC.APPROX))


def observer(simt):
    """observe(go, tiles, spans, stage, kt_bytes=None) for _long_cases: go()
    makes one launch without locations (one kernel); its dynamic LDS request is
    the stage plus the k-mer table (at most 4,096 B; kt_bytes where the caller
    knows it), a staged tile's workgroup wrote its span — all but the bytes that
    happen to equal the random fill, fewer than 3 in 100 — and a raw one at most
    the k-mer table."""
    def observe(go, tiles, spans, stage, kt_bytes=None):
        simt.simt_lds_log(1)
        go()
        simt.simt_lds_log(0)
        dyn, changed = C.c_uint64(), (C.c_uint32 * len(tiles))()
        nwg = simt.simt_lds_log_get(0, C.byref(dyn), changed, len(tiles))
        assert nwg == len(tiles) and simt.simt_lds_log_get(1, C.byref(dyn), changed, 0) == 0, "not one launch"
        nwg = simt.simt_lds_log_get(0, C.byref(dyn), changed, len(tiles))
        if kt_bytes is None:
            assert stage <= dyn.value <= stage + 4096, (dyn.value, stage)
        else:
            assert dyn.value == stage + kt_bytes, (dyn.value, stage, kt_bytes)
        kt = dyn.value - stage
        for t, (staged, span, got) in enumerate(zip(tiles, spans, list(changed))):
            if staged:
                assert span <= stage and 0.97 * span <= got <= span + kt, f"tile {t}: staged, {got} of {span} B written"
            else:
                assert span > stage and got <= kt, f"tile {t}: raw, {got} B written (k-mer table {kt} B)"
    return observe


# ------------------------------------------------------------------- 1. sweep

@pytest.mark.parametrize("occ", (0, 1))
@pytest.mark.parametrize("strands,n", LC.SWEEP_SHAPES)
@pytest.mark.parametrize("pb,planes,vb", S.LAYOUTS)
@pytest.mark.parametrize("text", sorted(LC.TEXTS))
def test_long_sweep_simt(pkg, O, simt, text, pb, planes, vb, strands, n, occ):
    simt.simt_config(pb * 139 + planes * 23 + vb + n + occ, 0.5)
    LC.sweep(pkg, O, text, pb, planes, vb, occ, PASSES[occ], shapes=[(strands, n)])


def test_long_approx_two_mismatches_best_simt(pkg, O, simt):
    """max_mm = 2 with FMX_APPROX_BEST on 150-symbol reads of the repeat text."""
    simt.simt_config(401, 0.5)
    case = LC.repeat_case(3)
    cmap = S.involution(case)
    ix, orc = LC.open_index(pkg, O, case, cmap, 4, 3, 64, 1)
    LC.check(ix, orc, case, "approx", LC.reads_for(case, cmap, 301, 150), cmap, "forward", **LC.APPROX_MM2)
    LC.check(ix, orc, case, "approx", LC.reads_for(case, cmap, 151, 150), cmap, "both", reversed=True,
             **LC.APPROX_MM2)
    ix.close()


@pytest.mark.parametrize("query,kw", QUERY_KW, ids=[q for q, _ in QUERY_KW])
def test_long_fixed_300_simt(pkg, O, simt, query, kw):
    """Reads of exactly 300 symbols: whole matches, seeds and variants at the longest length."""
    simt.simt_config(409, 0.5)
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
@pytest.mark.parametrize("query,kw", QUERY_KW, ids=[q for q, _ in QUERY_KW])
def test_long_stage_edge_simt(pkg, O, simt, query, kw, pb, planes, vb, strands, n, m):
    simt.simt_config(419 + m + n + pb, 0.5)
    LC.stage_edge(pkg, O, HostMem, pb, planes, vb, query, kw, strands, n, m, observe=observer(simt))


@pytest.mark.parametrize("query,kw", QUERY_KW, ids=[q for q, _ in QUERY_KW])
def test_long_strand_stage_150_simt(pkg, O, simt, query, kw):
    """150 symbols under both strands with the fixed-length hint: the stage is
    256 x 150 = 38,400 B, which both copies of 128 reads fill exactly."""
    simt.simt_config(421, 0.5)
    assert S.stage_bytes_of("both", 56, 150) == 38400
    LC.stage_edge(pkg, O, HostMem, 4, 3, 64, query, kw, "both", 129 + 22, 150, observe=observer(simt))


# -------------------------------------------------------------- 3. hint forms

@pytest.mark.parametrize("strands,n", (("forward", 513), ("reverse", 513), ("both", 300)))
@pytest.mark.parametrize("query,kw", QUERY_KW, ids=[q for q, _ in QUERY_KW])
def test_long_hint_forms_simt(pkg, O, simt, query, kw, strands, n):
    simt.simt_config(431 + n, 0.5)
    LC.hint_forms(pkg, O, HostMem, 4, 3, 64, query, kw, strands, n, observe=observer(simt))


# -------------------------------------------------------- 4. largest LDS request

@pytest.mark.parametrize("strands,n", (("forward", 257 + 44), ("both", 129 + 22)))
@pytest.mark.parametrize("pb", (4, 8))
@pytest.mark.parametrize("query,kw", QUERY_KW, ids=[q for q, _ in QUERY_KW])
def test_long_largest_lds_simt(pkg, O, simt, query, kw, pb, strands, n):
    simt.simt_config(433 + n + pb, 0.5)
    LC.largest_lds(pkg, O, HostMem, pb, query, kw, strands, n, observe=observer(simt))


# ---------------------------------------------------- 5. fixed-length hint limit

def test_long_hint_limit_simt(pkg, O, simt):
    simt.simt_config(439, 0.5)
    LC.hint_limit(pkg, O)
