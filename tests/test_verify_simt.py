"""Verifying placements (fmx_verify_async: k_verify; fmx_map_batch: seeds ->
locations -> vote -> verify; FMX_OPT_VERIFY_TEXT) on the CPU: the engine's own
sources under the SIMT shim (tests/simt), every output slot against the model
of _verify_cases.py — the contract of include/fmx.h in NumPy, itself checked
here against the recurrences written cell by cell.  Synthetic candidates hit
the kernel's edges exactly (reads of 0 to 129, 300 and 65,536 symbols, bands
0 to 31, 1 to 16 candidates, 1 to 257 reads, positions off both ends of the
text; _verify_cases.make_batch / assert_classes) over a random text and the
two-letter text; the pipeline runs real and planted reads, its expected values
the model over _vote_cases.place_expected.  The bodies are _verify_cases.py's,
shared with tests/test_gpu_verify.py."""
import pytest

import _verify_cases as VC
from _guard_cases import HostMem
from _simt import simt_fixture


simt = simt_fixture(launch_order=True)


def test_verify_model_against_plain_recurrences():
    VC.check_model(VC.case_for(3))
    VC.check_model(VC.case_for(2, two_letters=True), seed=1)


@pytest.mark.parametrize("n", VC.READ_COUNTS)
@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_synthetic_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 1000 + n, 0.5)
    case = VC.case_for(planes)
    ix, _ = VC.text_index(pkg, O, case, pb, planes, vb)
    VC.synthetic(pkg, VC.HostDev(), ix, case, n)
    ix.close()


@pytest.mark.parametrize("n", (5, 257))
def test_verify_two_letters_simt(pkg, O, simt, n):
    """Ends and starts tie all over a two-letter text."""
    simt.simt_config(5100 + n, 0.5)
    case = VC.case_for(2, two_letters=True)
    ix, _ = VC.text_index(pkg, O, case, 4, 2, 64)
    VC.synthetic(pkg, VC.HostDev(), ix, case, n)
    ix.close()


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_lengths_simt(pkg, O, simt, pb, planes, vb):
    simt.simt_config(5200 + pb, 0.5)
    case = VC.case_for(planes)
    ix, _ = VC.text_index(pkg, O, case, pb, planes, vb)
    VC.lengths(pkg, VC.HostDev(), ix, case)
    ix.close()


def test_verify_strand_flags_simt(pkg, O, simt):
    simt.simt_config(5300, 0.5)
    case = VC.case_for(3)
    ix, _ = VC.text_index(pkg, O, case, 4, 3, 64)
    VC.strand_flags(pkg, VC.HostDev(), ix, case)
    ix.close()


def test_verify_timer_and_arguments_simt(pkg, O, simt):
    """The "verify" timer counts one launch and nv * max_cands units, n = 0
    launches nothing, and the FMX_E_ARG cases of the contract."""
    simt.simt_config(5400, 0.5)
    for pb, planes, vb in VC.LAYOUTS:
        case = VC.case_for(planes)
        VC.check_arguments(pkg, VC.HostDev(), VC.text_index(pkg, O, case, pb, planes, vb)[0], case)


@pytest.mark.parametrize("n", (1, 255, 256, 257))
@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_map_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 79 + n, 0.5)
    VC.map_runs(pkg, O, pb, planes, vb, (n,), runs=VC.V.PLACE_RUNS[:2])


def test_map_both_strands_simt(pkg, O, simt):
    simt.simt_config(5500, 0.5)
    VC.map_both_strands(pkg, O, (257,))


def test_map_chunks_simt(pkg, O, simt, monkeypatch):
    simt.simt_config(5600, 0.5)
    VC.map_chunks(pkg, O, monkeypatch, 257)


def test_map_planted_reads_simt(pkg, O, simt):
    simt.simt_config(5700, 0.5)
    VC.planted(pkg, O, VC.LAYOUTS[:1])


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_text_load_option_simt(pkg, O, simt, pb, planes, vb):
    simt.simt_config(5800 + pb, 0.5)
    VC.load_option(pkg, O, VC.HostDev(), VC.case_for(3, k=3, sr=2), pb, 3, vb)


def test_verify_text_index_still_grouped_simt(pkg, O, simt, monkeypatch):
    simt.simt_config(5900, 0.5)
    VC.still_grouped(pkg, O, monkeypatch, HostMem)
