"""Placing reads (fmx_vote_async: k_vote; fmx_place_batch: seeds -> locations
-> vote) on the CPU: the engine's own sources under the SIMT shim (tests/simt),
every output slot against the model of _vote_cases.py — the contract of
include/fmx.h in plain Python.  Synthetic inputs hit the kernel's edges
exactly (chains of 0 to 1,025 hits, 1 to 257 chains, every max_seeds, band,
min_cover and max_cands class; _vote_cases.make_batch / assert_classes); the
pipeline runs real reads, its expected values the model over
_seed_cases.expected_arrays.  The bodies are _vote_cases.py's, shared with
tests/test_gpu_vote.py."""
import pytest

import _vote_cases as V
from _simt import simt_fixture


simt = simt_fixture(launch_order=True)


@pytest.mark.parametrize("n", V.CHAIN_COUNTS)
@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_vote_synthetic_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 1000 + n, 0.5)
    ix, _ = V.open_index(pkg, O, V.case_for(planes), pb, planes, vb, 1)
    V.synthetic(V.HostDev(), ix, n, pb)
    ix.close()


def test_vote_timer_and_arguments_simt(pkg, O, simt):
    """The "vote" timer counts one launch, n_chains = 0 launches nothing, and
    the FMX_E_ARG cases of the contract."""
    simt.simt_config(4141, 0.5)
    V.check_arguments(pkg, V.HostDev(), V.open_index(pkg, O, V.case_for(3), 4, 3, 64, 1)[0], 4)
    V.check_arguments(pkg, V.HostDev(), V.open_index(pkg, O, V.case_for(5), 8, 5, 128, 1)[0], 8)


@pytest.mark.parametrize("n", V.BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", V.LAYOUTS)
def test_place_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 77 + n, 0.5)
    case = V.case_for(3, k=3, sr=2)
    ix, orc = V.open_index(pkg, O, case, pb, planes, vb, 1)
    runs = V.PLACE_RUNS if n < 700 else V.PLACE_RUNS[:2]  # (the emulator: seconds per 700-read run)
    V.place_runs(V.HostDev(), pkg, ix, orc, case, pb, n, runs)
    ix.close()


def test_place_two_letters_simt(pkg, O, simt):
    simt.simt_config(2323, 0.5)
    V.two_letters(pkg, O, (257,))


def test_place_both_strands_simt(pkg, O, simt):
    simt.simt_config(2424, 0.5)
    V.both_strands(pkg, O, (257,))


def test_place_chunks_and_limits_simt(pkg, O, simt, monkeypatch):
    simt.simt_config(2525, 0.5)
    V.chunks_and_limits(pkg, O, monkeypatch)


def test_place_planted_reads_simt(pkg, O, simt):
    simt.simt_config(2626, 0.5)
    V.planted(pkg, O, V.LAYOUTS[:1])
