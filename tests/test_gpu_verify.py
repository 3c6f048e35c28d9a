"""Verifying placements on the GPU (fmx_verify_async: k_verify; fmx_map_batch:
seeds -> locations -> vote -> verify; FMX_OPT_VERIFY_TEXT): the cases of
tests/test_verify_simt.py on the gfx950 kernel, every output slot against the
model of _verify_cases.py — the contract of include/fmx.h in NumPy.  Synthetic
candidates: 1, 3, 4, 5, 255, 256 and 257 reads of 0 to 129, 300 and 65,536
symbols at every band and max_cands class, positions off both ends of the
text, for u32 and u64 positions, a random and a two-letter text.  The pipeline:
batches of 1, 255, 256, 257 and 700 real reads, skip 0 and 1, forward and
reversed, both strands, chunked, planted reads; the load option against an
option-1 index."""
import os

import pytest

import _verify_cases as VC
from _guard_cases import TorchMem

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_synthetic(pkg, O, pb, planes, vb):
    case = VC.case_for(planes)
    ix, _ = VC.text_index(pkg, O, case, pb, planes, vb)
    dev = VC.TorchDev()
    for n in VC.READ_COUNTS:
        VC.synthetic(pkg, dev, ix, case, n)
    ix.close()


def test_verify_two_letters(pkg, O):
    """Ends and starts tie all over a two-letter text."""
    case = VC.case_for(2, two_letters=True)
    ix, _ = VC.text_index(pkg, O, case, 4, 2, 64)
    for n in (5, 257):
        VC.synthetic(pkg, VC.TorchDev(), ix, case, n)
    ix.close()


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_lengths(pkg, O, pb, planes, vb):
    case = VC.case_for(planes)
    ix, _ = VC.text_index(pkg, O, case, pb, planes, vb)
    VC.lengths(pkg, VC.TorchDev(), ix, case)
    ix.close()


def test_verify_strand_flags(pkg, O):
    case = VC.case_for(3)
    ix, _ = VC.text_index(pkg, O, case, 4, 3, 64)
    VC.strand_flags(pkg, VC.TorchDev(), ix, case)
    ix.close()


def test_verify_timer_and_arguments(pkg, O):
    """The "verify" timer counts one launch and nv * max_cands units, n = 0
    launches nothing, and the FMX_E_ARG cases of the contract."""
    for pb, planes, vb in VC.LAYOUTS:
        case = VC.case_for(planes)
        VC.check_arguments(pkg, VC.TorchDev(), VC.text_index(pkg, O, case, pb, planes, vb)[0], case)


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_map(pkg, O, pb, planes, vb):
    VC.map_runs(pkg, O, pb, planes, vb, VC.BATCH_SIZES)


def test_map_both_strands(pkg, O):
    VC.map_both_strands(pkg, O, (257, 700))


def test_map_chunks(pkg, O, monkeypatch):
    VC.map_chunks(pkg, O, monkeypatch, 700)


def test_map_planted_reads(pkg, O):
    VC.planted(pkg, O, VC.LAYOUTS)


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_text_load_option(pkg, O, pb, planes, vb):
    VC.load_option(pkg, O, VC.TorchDev(), VC.case_for(3, k=3, sr=2), pb, 3, vb)


def test_verify_text_index_still_grouped(pkg, O, monkeypatch):
    VC.still_grouped(pkg, O, monkeypatch, TorchMem)
