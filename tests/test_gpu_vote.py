"""Placing reads on the GPU (fmx_vote_async: k_vote; fmx_place_batch: seeds ->
locations -> vote): the cases of tests/test_vote_simt.py on the gfx950 kernel,
every output slot against the model of _vote_cases.py — the contract of
include/fmx.h in plain Python.  Synthetic inputs: 1, 3, 4, 5, 255, 256 and 257
chains of 0 to 1,025 hits at every max_seeds, band, min_cover and max_cands
class, for u32 and u64 positions.  The pipeline: batches of 1, 255, 256, 257
and 700 real reads, skip 0 and 1, band 0 and 8, forward and reversed, load
options 1 and 63, both strands, chunked, planted reads."""
import os

import numpy as np
import pytest

import _vote_cases as V
from _seed_cases import BATCH_SIZES, batch, case_for, open_index
from _strand_cases import expand, involution

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_vote_synthetic(pkg, O, pb, planes, vb):
    ix, _ = open_index(pkg, O, case_for(planes), pb, planes, vb, 1)
    dev = V.TorchDev()
    for n in V.CHAIN_COUNTS:
        for ms, band, mc, K in V.CONFIGS:
            arrays = V.make_batch(n, ms, pb, band, K)
            exp = V.model(*arrays[:4], ms, arrays[4], band, mc, K)
            V.assert_classes(arrays, ms, pb, band, mc, K, exp)
            got = V.run_vote(dev, ix, arrays, ms, band, mc, K)
            V.compare(f"vote n={n} max_seeds={ms} band={band} min_cover={mc} max_cands={K}", got, exp)
    ix.close()


def test_vote_timer_and_arguments(pkg, O):
    """The "vote" timer counts one launch, n_chains = 0 launches nothing, and
    the FMX_E_ARG cases of the contract."""
    V.check_arguments(pkg, V.TorchDev(), open_index(pkg, O, case_for(3), 4, 3, 64, 1)[0], 4)
    V.check_arguments(pkg, V.TorchDev(), open_index(pkg, O, case_for(5), 8, 5, 128, 1)[0], 8)


@pytest.mark.parametrize("options", [1, 63])
@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_place(pkg, O, pb, planes, vb, options):
    """place_batch against the model, and against seeds_batch_async +
    vote_async run here on buffers of the test's own."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, pb, planes, vb, options)
    for n in BATCH_SIZES:
        pats = batch(case, n)
        for skip, band, rev in V.PLACE_RUNS:
            exp, got = V.check_place(ix, orc, case, pats, skip, band, rev)
            if n >= 255:
                assert (exp[0] > 1).sum() >= 20 and (exp[0] == 0).sum() >= 2 and (exp[5] > exp[0]).sum() >= 1
            if not rev:
                dgot = V.place_device(V.TorchDev(), pkg, ix, pb, pats, skip, band)
                V.compare("seeds_batch_async + vote_async", dgot, exp)
    ix.close()


def test_place_two_letters(pkg, O):
    """A two-letter text: most seeds have more than max_occ occurrences and
    bring none, the others bring up to 16 each."""
    case = case_for(2, two_letters=True, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    for n in (257, 700):
        exp, _ = V.check_place(ix, orc, case, batch(case, n), 1, 8)
        assert (exp[0] > 0).sum() >= 50
        V.check_place(ix, orc, case, batch(case, n), 0, 0, True, max_cands=16, min_cover=1)
    ix.close()


def test_place_both_strands(pkg, O):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    cmap = involution(case)
    ix.set_complement(cmap)
    for n in (257, 700):
        reads = batch(case, n)
        both = ix.place_batch(reads, skip=1, band=8, strands="both", **V.PLACE)
        flat = ix.place_batch(expand(reads, cmap, "both"), skip=1, band=8, **V.PLACE)
        assert both[0].shape == (2 * n,) and all(np.array_equal(a, b) for a, b in zip(both, flat))
    assert ix.place(reads[3], strands="both") == (ix.place(reads[3]), ix.place(expand(reads[3:4], cmap, "reverse")[0]))
    ix.close()


def test_place_chunks_and_limits(pkg, O, monkeypatch):
    """FMX_PLACE_CHUNK=100 (read at load): 700 reads in seven chunks, the
    results those of one; max_seeds * max_occ = 1,024 is accepted, 1,025 is
    FMX_E_ARG."""
    case = case_for(3, k=3, sr=2)
    pats = batch(case, 700)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    whole = ix.place_batch(pats, skip=1, band=8, **V.PLACE)
    ix.close()
    monkeypatch.setenv("FMX_PLACE_CHUNK", "100")
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    V.check_place(ix, orc, case, pats, 1, 8)
    parts = ix.place_batch(pats, skip=1, band=8, **V.PLACE)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    V.check_limits(pkg, ix, pats[:40])
    ix.close()


def test_place_planted_reads(pkg, O):
    case = case_for(3, k=3, sr=2)
    for pb, planes, vb in V.LAYOUTS:
        ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
        V.check_planted(ix, orc, case)
        ix.close()
