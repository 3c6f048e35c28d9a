"""Placing reads on the GPU (fmx_vote_async: k_vote; fmx_place_batch: seeds ->
locations -> vote): the cases of tests/test_vote_simt.py on the gfx950 kernel,
every output slot against the model of _vote_cases.py — the contract of
include/fmx.h in plain Python.  Synthetic inputs: 1, 3, 4, 5, 255, 256 and 257
chains of 0 to 1,025 hits at every max_seeds, band, min_cover and max_cands
class, for u32 and u64 positions.  The pipeline: batches of 1, 255, 256, 257
and 700 real reads, skip 0 and 1, band 0 and 8, forward and reversed, load
options 1 and 63, both strands, chunked, planted reads."""
import os

import pytest

import _vote_cases as V

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_vote_synthetic(pkg, O, pb, planes, vb):
    ix, _ = V.open_index(pkg, O, V.case_for(planes), pb, planes, vb, 1)
    dev = V.TorchDev()
    for n in V.CHAIN_COUNTS:
        V.synthetic(dev, ix, n, pb)
    ix.close()


def test_vote_timer_and_arguments(pkg, O):
    """The "vote" timer counts one launch, n_chains = 0 launches nothing, and
    the FMX_E_ARG cases of the contract."""
    V.check_arguments(pkg, V.TorchDev(), V.open_index(pkg, O, V.case_for(3), 4, 3, 64, 1)[0], 4)
    V.check_arguments(pkg, V.TorchDev(), V.open_index(pkg, O, V.case_for(5), 8, 5, 128, 1)[0], 8)


@pytest.mark.parametrize("options", [1, 63])
@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_place(pkg, O, pb, planes, vb, options):
    case = V.case_for(3, k=3, sr=2)
    ix, orc = V.open_index(pkg, O, case, pb, planes, vb, options)
    for n in V.BATCH_SIZES:
        V.place_runs(V.TorchDev(), pkg, ix, orc, case, pb, n, V.PLACE_RUNS)
    ix.close()


def test_place_two_letters(pkg, O):
    V.two_letters(pkg, O, (257, 700))


def test_place_both_strands(pkg, O):
    V.both_strands(pkg, O, (257, 700))


def test_place_chunks_and_limits(pkg, O, monkeypatch):
    V.chunks_and_limits(pkg, O, monkeypatch)


def test_place_planted_reads(pkg, O):
    V.planted(pkg, O, V.LAYOUTS)
