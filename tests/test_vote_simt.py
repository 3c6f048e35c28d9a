"""Placing reads (fmx_vote_async: k_vote; fmx_place_batch: seeds -> locations
-> vote) on the CPU: the engine's own sources under the SIMT shim (tests/simt),
every output slot against the model of _vote_cases.py — the contract of
include/fmx.h in plain Python.  Synthetic inputs hit the kernel's edges
exactly (chains of 0 to 1,025 hits, 1 to 257 chains, every max_seeds, band,
min_cover and max_cands class; _vote_cases.make_batch / assert_classes); the
pipeline runs real reads, its expected values the model over
_seed_cases.expected_arrays."""
import numpy as np
import pytest

import _vote_cases as V
from _seed_cases import BATCH_SIZES, batch, case_for, open_index
from _simt import simt_fixture
from _strand_cases import expand, involution


simt = simt_fixture(launch_order=True)


@pytest.mark.parametrize("n", V.CHAIN_COUNTS)
@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_vote_synthetic_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 1000 + n, 0.5)
    ix, _ = open_index(pkg, O, case_for(planes), pb, planes, vb, 1)
    dev = V.HostDev()
    for ms, band, mc, K in V.CONFIGS:
        arrays = V.make_batch(n, ms, pb, band, K)
        exp = V.model(*arrays[:4], ms, arrays[4], band, mc, K)
        V.assert_classes(arrays, ms, pb, band, mc, K, exp)
        got = V.run_vote(dev, ix, arrays, ms, band, mc, K)
        V.compare(f"vote n={n} max_seeds={ms} band={band} min_cover={mc} max_cands={K}", got, exp)
    ix.close()


def test_vote_timer_and_arguments_simt(pkg, O, simt):
    """The "vote" timer counts one launch, n_chains = 0 launches nothing, and
    the FMX_E_ARG cases of the contract."""
    simt.simt_config(4141, 0.5)
    V.check_arguments(pkg, V.HostDev(), open_index(pkg, O, case_for(3), 4, 3, 64, 1)[0], 4)
    V.check_arguments(pkg, V.HostDev(), open_index(pkg, O, case_for(5), 8, 5, 128, 1)[0], 8)


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_place_simt(pkg, O, simt, pb, planes, vb, n):
    """place_batch against the model, and against seeds_batch_async +
    vote_async run here on buffers of the test's own."""
    simt.simt_config(pb * 77 + n, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
    pats = batch(case, n)
    for skip, band, rev in V.PLACE_RUNS if n < 700 else V.PLACE_RUNS[:2]:  # (the emulator: seconds per 700-read run)
        exp, got = V.check_place(ix, orc, case, pats, skip, band, rev)
        if n >= 255:
            assert (exp[0] > 1).sum() >= 20 and (exp[0] == 0).sum() >= 2 and (exp[5] > exp[0]).sum() >= 1
        if not rev:
            dgot = V.place_device(V.HostDev(), pkg, ix, pb, pats, skip, band)
            V.compare("seeds_batch_async + vote_async", dgot, exp)
    ix.close()


def test_place_two_letters_simt(pkg, O, simt):
    """A two-letter text: most seeds have more than max_occ occurrences and
    bring none, the others bring up to 16 each."""
    simt.simt_config(2323, 0.5)
    case = case_for(2, two_letters=True, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    exp, _ = V.check_place(ix, orc, case, batch(case, 257), 1, 8)
    assert (exp[0] > 0).sum() >= 50
    V.check_place(ix, orc, case, batch(case, 257), 0, 0, True, max_cands=16, min_cover=1)
    ix.close()


def test_place_both_strands_simt(pkg, O, simt):
    simt.simt_config(2424, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    cmap = involution(case)
    ix.set_complement(cmap)
    reads = batch(case, 257)
    both = ix.place_batch(reads, skip=1, band=8, strands="both", **V.PLACE)
    flat = ix.place_batch(expand(reads, cmap, "both"), skip=1, band=8, **V.PLACE)
    assert both[0].shape == (514,) and all(np.array_equal(a, b) for a, b in zip(both, flat))
    assert ix.place(reads[3], strands="both") == (ix.place(reads[3]), ix.place(expand(reads[3:4], cmap, "reverse")[0]))
    ix.close()


def test_place_chunks_and_limits_simt(pkg, O, simt, monkeypatch):
    """FMX_PLACE_CHUNK=100 (read at load): 700 reads in seven chunks, the
    results those of one; max_seeds * max_occ = 1,024 is accepted, 1,025 is
    FMX_E_ARG."""
    simt.simt_config(2525, 0.5)
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


def test_place_planted_reads_simt(pkg, O, simt):
    simt.simt_config(2626, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    V.check_planted(ix, orc, case)
    ix.close()
