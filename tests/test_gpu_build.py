"""The blob builder on the GPU (fmx_build / fmx_build_device: fmx_build.hip's
kernels, rocPRIM's sorts, scans and selects) at the edges its other GPU tests
do not visit, the cases of tests/test_build_simt.py: the doubling depth around
K0 * 2^r for sigma 2, 4, 21 and 64 on both suffix-array paths, the 64-bit
path's buckets (one, single-suffix ones, 1,000 of sigma 64's 4,225 — the
33.8 KB of dynamic LDS of k_bucket_scatter), n + 1 around one workgroup,
1,023 / 1,024 / 1,025 / 2,049 checkpoint blocks, the k-mer histogram on
either side of its LDS limit, sampling ratios, FMX_E_SYMBOL by position with a
correct build after every failure, and guard bands around fmx_build_device.
The reference is the oracle's builder, blob byte for byte.  Bodies and floors
(asserted on the inputs and the reference alone): _build_cases.py.  The
every-layout sweep is tests/test_gpu.py's; no test here uses layout
(4, 6, 64)."""
import pytest

import _build_cases as B
from _guard_cases import SKEWS, TorchMem
from _util import SIMT_LAYOUTS

pytestmark = pytest.mark.gpu
PATHS = ("32", "64")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sigma", B.DOUBLING_SIGMAS)
def test_build_doubling(pkg, O, sigma, path):
    for group in B.DOUBLING_GROUPS:
        B.doubling(pkg, O, sigma, group, path)


@pytest.mark.parametrize("name", [c[0] for c in B.bucket_cases()])
def test_build_buckets(pkg, O, name):
    B.buckets(pkg, O, name)


@pytest.mark.parametrize("path", PATHS)
def test_build_small_sizes(pkg, O, path):
    B.small_sizes(pkg, O, path)


@pytest.mark.parametrize("blocks_len", sorted(B.BLOCK_EDGES))
def test_build_block_edges(pkg, O, blocks_len):
    B.block_edge(pkg, O, blocks_len)


@pytest.mark.parametrize("side", ["lds", "global"])
def test_build_kmer_table_edge(pkg, O, side):
    B.kt_edge(pkg, O, side)


def test_build_sampling_edges(pkg, O):
    B.sampling_edges(pkg, O)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", B.ERROR_CASES, ids=str)
def test_build_errors(pkg, O, case, path):
    B.error_case(pkg, O, case, path)


@pytest.mark.parametrize("n", [3, 257])
@pytest.mark.parametrize("lay", [SIMT_LAYOUTS[0], SIMT_LAYOUTS[2]], ids=str)
def test_build_device_guard(pkg, O, lay, n):
    for skew in SKEWS:
        B.device_guard(pkg, O, TorchMem, lay, n, skew)
