"""Longest-suffix match (fmx_match_batch: k_match, then the locate's k_emit)
on the CPU: the engine's own sources under the SIMT shim (tests/simt, as
tests/test_simt.py), every answer against the values of _match_cases.py —
lengths from the oracle's counts of growing suffixes, intervals from a plainly
sorted suffix list, locations from the oracle's locate of the matched suffix.
A subset of the layouts the GPU file sweeps, every case class: full matches
of m = 1, 2, k-1, k, k+1, 7, 40; one substitution inside the last k symbols
(seed fallback), at m-k-1 (first LF step fails) and further left; an absent
last byte (L = 0); an empty pattern in mid-batch; matches that reach the text
start; unique substrings behind a wrong symbol (sampled-row rollback); a
two-letter text (hundreds of rows per match); capacity; min_len / max_occ;
ranges only; PassThrough bytes >= symbol_count; the device call.  The bodies
are _match_cases.py's, shared with tests/test_gpu_match.py."""
import pytest

import _match_cases as MC
from _simt import simt_fixture
from _util import SIMT_LAYOUTS, HostDev


simt = simt_fixture(launch_order=True)


@pytest.mark.parametrize("n", MC.BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", SIMT_LAYOUTS)
def test_match_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 131 + planes * 17 + vb + n, 0.5)
    case = MC.case_for(planes)
    pats = case.batch(n)
    for occ in (0, 1):
        ix, orc = MC.open_index(pkg, O, case, pb, planes, vb, occ)
        exp = MC.check_match(pkg, ix, orc, case, pats)
        if occ == 1 or n < 256:
            MC.check_match(pkg, ix, orc, case, pats, reversed=True)
        if n >= 256:
            MC.classes_and_full_match_check(ix, case, pats, exp)
        ix.close()


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_match_two_letters_simt(pkg, O, simt, sr):
    simt.simt_config(900 + sr, 0.5)
    MC.two_letters(pkg, O, 257, sr, ((4, 64),))


@pytest.mark.parametrize("min_len", [1, 5])
@pytest.mark.parametrize("max_occ", [0, 1, 10, None])
def test_match_filters_simt(pkg, O, simt, min_len, max_occ):
    simt.simt_config(77 + min_len, 0.5)
    MC.filters(pkg, O, 257, min_len, max_occ)


def test_match_ranges_only_and_capacity_simt(pkg, O, simt):
    simt.simt_config(4242, 0.5)
    MC.ranges_only_and_capacity(pkg, O, 300)


def test_match_pass_through_simt(pkg, O, simt):
    simt.simt_config(606, 0.5)
    MC.pass_through(pkg, O)


def test_match_async_simt(pkg, O, simt):
    """On the emulator, device memory is host memory."""
    simt.simt_config(515, 0.5)
    MC.device_call(pkg, O, HostDev(), 300)
