"""Guard bands around fmx_verify_async on the GPU: the run of
tests/_verify_cases.py (run_verify_guard, as tests/test_verify_guard_simt.py
has it on the emulator) on the gfx950 kernel — every buffer of the call carved
out of ONE 0xA5-filled tensor at its exact size and weakest alignment, d_bytes
at every alignment class the guard tests use, the whole tensor read back after
the launch.

Nothing a correct or a broken k_verify touches lies far outside its buffers: a
wave reads its own read's bytes, its pattern's ncands word and its slot's
position, text bytes checked against [0, n), and writes its own slot's three
outputs; the guards are 4 KiB."""
import pytest

import _verify_cases as VC
from _guard_cases import TorchMem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pb,planes,vb", VC.LAYOUTS)
def test_verify_guard(pkg, O, pb, planes, vb):
    VC.guard(pkg, O, TorchMem, pb, planes, vb)
