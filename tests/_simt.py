"""The `simt` fixture of the SIMT test modules: tests/simt/libfmx_simt.so (the
engine's own sources compiled for the CPU against the SIMT shim) built, bound
with the package's SIGNATURES and swapped in for the engine library while the
module's tests run.  A module binds it with `simt = simt_fixture(...)`.
simt_lds_log / simt_lds_log_get: the shim's log of each launch's dynamic LDS
request and of the bytes of it every workgroup wrote (test_long_simt.py)."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SIMT_DIR = os.path.join(HERE, "simt")
SIMT_LIB = os.path.join(SIMT_DIR, "libfmx_simt.so")

# the shim's own entry points (simt_rt.cpp)
SHIM = {
    "simt_config": (None, [C.c_uint64, C.c_double]),
    "simt_stats": (None, [C.POINTER(C.c_uint64)] * 3),
    "simt_memset_fault": (None, [C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64]),
    "simt_defer": (None, [C.c_int, C.c_double]),
    "simt_selftest_defer": (C.c_int, []),
    "simt_block_order": (None, [C.c_int]),
    "simt_lds_log": (None, [C.c_int]),
    "simt_lds_log_get": (C.c_uint64, [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint64]),
}


def simt_fixture(launch_order):
    """launch_order: FMX_FUSED = FMX_EMIT_CHAIN = 0 while the module runs —
    workgroups run one at a time in a shuffled order here, so the fused launch
    (k_locate: a workgroup waits for its batch's earlier tiles) and k_emit_chain,
    which ends grouped launches the same way, are off unless a test turns them
    on with index-ordered workgroups.  False: the environment is left alone
    (the guard-band modules set it per path)."""
    env = {"FMX_FUSED": "0", "FMX_EMIT_CHAIN": "0"} if launch_order else {}

    @pytest.fixture(scope="module")
    def simt(pkg):
        subprocess.check_call(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", SIMT_DIR])
        n = pkg._native
        L = C.CDLL(SIMT_LIB)
        for name, (res, args) in list(n.SIGNATURES.items()) + list(SHIM.items()):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        # deferred streams for every test: work queued on a stream runs at a
        # random later host call or when the host synchronises, copies read and
        # write host memory when they run (simt_rt.cpp)
        L.simt_defer(1, 0.25)
        saved_env = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        saved = n._lib
        n._lib = L
        yield L
        n._lib = saved
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    return simt
