"""Guard bands around fmx_verify_async on the CPU: the engine's own sources
under the SIMT shim (tests/simt), every buffer of the call carved at its exact
size and weakest alignment out of one 0xA5-filled array (_verify_cases.py, on
the arena of _guard_cases.py), d_bytes at every alignment class the guard tests
use: guards and inputs untouched, every output the model's."""
import pytest

import _verify_cases as VC
from _guard_cases import HostMem
from _simt import simt_fixture


simt = simt_fixture(launch_order=False)


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_guard_simt(pkg, O, simt, pb, planes, vb):
    simt.simt_config(8800 + pb, 0.5)
    VC.guard(pkg, O, HostMem, pb, planes, vb)
