"""The blob builder (fmx_build.hip) on the CPU: the engine's own source under
the SIMT shim (tests/simt, as tests/test_simt.py) with its rocPRIM calls
served by tests/simt/shim/rocprim/rocprim.hpp — workgroups shuffled,
work-items interleaved, every hipMalloc random, streams deferred, the sorts'
current buffer drawn at random and their other buffer and temporary storage
scribbled on.  The reference is the oracle's builder, blob byte for byte;
where a blob is loaded, the oracle's counts and locations.  Bodies and floors:
_build_cases.py, shared with tests/test_gpu_build.py.

(a) every layout x four alphabet sizes; (b) the doubling depth around
K0 * 2^r for sigma 2, 4, 21, 64; (c) both suffix-array paths on those texts,
and the 64-bit path's buckets (one, single-suffix ones, 1,000 of 4,225);
(d) n + 1 around one workgroup, n = 0 and 1, 1,023 / 1,024 / 1,025 checkpoint
blocks, the k-mer histogram on either side of its LDS limit, sampling ratios;
(e) FMX_E_SYMBOL by position, FMX_E_CONFIG, FMX_E_ALIGN, a correct build after
each; (f) guard bands around fmx_build_device; (g) (a) and (e) under three
deferred-stream schedules.  Then the inputs of
tests/test_gpu.py::test_builder_and_queries_every_layout[4-6-64], which once
aborted on the GPU: built here and queried through the whole parity sequence
under three emulator seeds, and replayed by a stand-alone program
(tests/simt/replay.cpp) linked against the emulator's objects rebuilt under
the host's address and undefined-behaviour sanitizers (the layouts it never
calls excepted)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import _build_cases as B
from _guard_cases import SKEWS, HostMem
from _simt import SIMT_DIR, simt_fixture
from _util import ALL_LAYOUTS, SIMT_LAYOUTS

simt = simt_fixture(launch_order=True)

PATHS = ("32", "64")
DEFER = ((1, 0.0), (2, 0.25), (3, 0.75))  # (emulator seed, chance that a host call runs queued work)


@pytest.fixture
def defer(simt):
    """Deferred streams with a progress chance of the test's own; the module's 0.25 afterwards."""
    yield lambda p: simt.simt_defer(1, p)
    simt.simt_defer(1, 0.25)


# ---------------------------------------------------------------------- (a)

@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_build_every_layout_simt(pkg, O, simt, pb, planes, vb):
    simt.simt_config(pb * 1000 + planes * 100 + vb, 0.5)
    B.every_layout(pkg, O, pb, planes, vb, load=(pb, planes, vb) in SIMT_LAYOUTS)


# ---------------------------------------------------------------- (b), (c)

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("group", B.DOUBLING_GROUPS)
@pytest.mark.parametrize("sigma", B.DOUBLING_SIGMAS)
def test_build_doubling_simt(pkg, O, simt, sigma, group, path):
    simt.simt_config(sigma * 7 + len(group) + int(path), 0.5)
    B.doubling(pkg, O, sigma, group, path)


@pytest.mark.parametrize("name", [c[0] for c in B.bucket_cases()])
def test_build_buckets_simt(pkg, O, simt, name):
    simt.simt_config(6400 + len(name), 0.5)
    B.buckets(pkg, O, name)


# ---------------------------------------------------------------------- (d)

@pytest.mark.parametrize("path", PATHS)
def test_build_small_sizes_simt(pkg, O, simt, path):
    simt.simt_config(255 + int(path), 0.5)
    B.small_sizes(pkg, O, path)


@pytest.mark.parametrize("blocks_len", [1023, 1024, 1025])
def test_build_block_edges_simt(pkg, O, simt, blocks_len):
    """(2,049 blocks: tests/test_gpu_build.py only — two chunks and a block are
    65,543 symbols, past what one emulator test may cost.)"""
    simt.simt_config(blocks_len, 0.5)
    B.block_edge(pkg, O, blocks_len)


@pytest.mark.parametrize("side", ["lds", "global"])
def test_build_kmer_table_edge_simt(pkg, O, simt, side):
    """... and which histogram ran: at kt_len = 8,192 the one launch with
    dynamic LDS asked for 4 * kt_len bytes and every workgroup wrote into them;
    at the next size up no launch asks for any."""
    simt.simt_config(8192 + len(side), 0.5)
    simt.simt_lds_log(1)
    try:
        kt_len = B.kt_edge(pkg, O, side)
        launches = []
        dyn, changed = C.c_uint64(), (C.c_uint32 * 64)()
        while True:
            wgs = simt.simt_lds_log_get(len(launches), C.byref(dyn), changed, 64)
            if not wgs:
                break
            launches.append((dyn.value, list(changed[:min(wgs, 64)])))
    finally:
        simt.simt_lds_log(0)
    if side == "lds":
        assert [d for d, _ in launches] == [4 * kt_len], launches
        assert all(c > 0 for c in launches[0][1]), "a workgroup's LDS histogram was never written"
    else:
        assert launches == [], launches


def test_build_sampling_edges_simt(pkg, O, simt):
    simt.simt_config(1010, 0.5)
    B.sampling_edges(pkg, O)


# ---------------------------------------------------------------------- (e)

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", B.ERROR_CASES, ids=str)
def test_build_errors_simt(pkg, O, simt, case, path):
    simt.simt_config(600 + int(path), 0.5)
    B.error_case(pkg, O, case, path)


# ---------------------------------------------------------------------- (f)

@pytest.mark.parametrize("n", [3, 257])
@pytest.mark.parametrize("lay", [SIMT_LAYOUTS[0], SIMT_LAYOUTS[2]], ids=str)
def test_build_device_guard_simt(pkg, O, simt, lay, n):
    simt.simt_config(sum(lay) + n, 0.5)
    for skew in SKEWS:
        B.device_guard(pkg, O, HostMem, lay, n, skew)


# ---------------------------------------------------------------------- (g)

@pytest.mark.parametrize("seed,progress", DEFER)
@pytest.mark.parametrize("pb,planes,vb", SIMT_LAYOUTS)
def test_build_deferred_simt(pkg, O, simt, defer, pb, planes, vb, seed, progress):
    simt.simt_config(seed * 7919 + pb + planes + vb, 0.5)
    defer(progress)
    B.every_layout(pkg, O, pb, planes, vb)


@pytest.mark.parametrize("seed,progress", DEFER)
def test_build_errors_deferred_simt(pkg, O, simt, defer, seed, progress):
    simt.simt_config(seed * 104729, 0.5)
    defer(progress)
    for i, case in enumerate(B.ERROR_CASES):
        B.error_case(pkg, O, case, PATHS[(i + seed) % 2])


# ------------------------------------- the layout-sweep case (4, 6, 64), replayed

REPLAY_LAYOUT = (4, 6, 64)
REPLAY_SEEDS = (4664, 1, 2)


def replay_inputs():
    """test_builder_and_queries_every_layout[4-6-64]'s own inputs: the same
    generator (seed 4 * 1000 + 6 * 100 + 64 = 4664), the same draws."""
    return list(B.every_layout_inputs(*REPLAY_LAYOUT))


@pytest.mark.parametrize("sub", range(4))
@pytest.mark.parametrize("seed", REPLAY_SEEDS)
def test_replay_4_6_64_simt(pkg, O, simt, monkeypatch, seed, sub):
    """One of the case's four alphabet sizes (2, 3, 33, 64): the blob built on
    the emulator, then check_parity's whole sequence at options 0, 1 and 63."""
    monkeypatch.setenv("FMX_DEEP_LUT_MB", "1")  # (as tests/test_gpu.py sets it)
    simt.simt_config(seed, 0.5)
    pb, planes, vb = REPLAY_LAYOUT
    sigma, chars, table, text, k, sr, pats = replay_inputs()[sub]
    assert sigma == (2, 3, 33, 64)[sub] and len(pats) == 353
    blob = B.assert_blob(pkg, O, text, sigma, REPLAY_LAYOUT, k, sr, table)
    for occ in B.OCC_MODES:
        B.check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)


def _put(f, *arrays):
    for a in arrays:
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        f.write(struct.pack("<Q", a.size))
        f.write(a.tobytes())


def _get(buf, at):
    n = struct.unpack_from("<Q", buf, at)[0]
    return np.frombuffer(buf, np.uint8, n, at + 8), at + 8 + n


def replay_jobs(pkg, part):
    """(expected fmx_build status, text, table or None, sigma, layout, k, sr,
    patterns, load options, blob length to claim or 0, blob skew) per job.
    part "sub0" .. "sub3": one of the four sub-cases of [4-6-64] (sigma 2, 3,
    33, 64: a test each, to keep each within an emulator test's time);
    "errors": every failing build
    of (e) — a symbol out of range at the first, the last and the 300th byte
    under both encoders, a wrong blob_len (fmx_build has uploaded the text
    through its pinned stage by the time build_device rejects it), a
    misaligned blob — each followed by a correct build that is then queried."""
    n_ = pkg._native
    if part.startswith("sub"):
        sigma, chars, table, text, k, sr, pats = replay_inputs()[int(part[3:])]
        return [(0, text, table, sigma, REPLAY_LAYOUT, k, sr, pats, B.OCC_MODES, 0, 0)]
    jobs = []
    rng = np.random.default_rng(600)
    good = bytes(rng.choice(np.frombuffer(B.ACGT, np.uint8), size=600))
    bad_table = bytearray(B.ACGT_TABLE)
    bad_table[ord("!")] = 4
    lay, ask = B.ERROR_LAYOUT, [good[5:17], b"ACG", b"\x00"]
    for at in (0, 599, 300):
        bad = bytearray(good)
        bad[at] = ord("!")
        jobs.append((n_.FMX_E_SYMBOL, bytes(bad), bytes(bad_table), 4, lay, 2, 2, [], (), 0, 0))
        jobs.append((0, good, bytes(bad_table), 4, lay, 2, 2, ask, (1,), 0, 0))
        idx = bytearray(rng.integers(0, 4, size=600).astype(np.uint8))
        ok = bytes(idx)
        idx[at] = 4
        jobs.append((n_.FMX_E_SYMBOL, bytes(idx), None, 4, lay, 2, 2, [], (), 0, 0))
        jobs.append((0, ok, None, 4, lay, 2, 2, [ok[5:17], ok[:3]], (0,), 0, 0))
    jobs.append((n_.FMX_E_CONFIG, good, B.ACGT_TABLE, 4, lay, 2, 2, [], (), 16, 0))
    jobs.append((0, good, B.ACGT_TABLE, 4, lay, 2, 2, ask, (0, 1), 0, 0))
    jobs.append((n_.FMX_E_ALIGN, good, B.ACGT_TABLE, 4, lay, 2, 2, [], (), 0, 4))
    jobs.append((0, good, B.ACGT_TABLE, 4, lay, 2, 2, ask, (1,), 0, 8))   # (8 past a 16-byte boundary is aligned enough)
    return jobs


@pytest.fixture(scope="module")
def replay_program():
    """tests/simt/build_asan/replay, built once (make replay: minutes in a clean tree, nothing after)."""
    subprocess.check_call(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", SIMT_DIR, "replay"])
    return os.path.join(SIMT_DIR, "build_asan", "replay")


@pytest.mark.parametrize("part", ["sub0", "sub1", "sub2", "sub3", "errors"])
@pytest.mark.parametrize("path", PATHS)
def test_replay_program_sanitized(pkg, O, tmp_path, replay_program, path, part):
    """tests/simt/replay.cpp, a program of its own linked against the emulator's
    objects rebuilt under -fsanitize=address,undefined (make replay: a build
    directory of its own, nothing of it loaded into this process; the layouts
    the replay never calls are linked as the emulator library has them):
    fmx_build, fmx_load, fmx_locate_batch, fmx_count_batch, the count and the
    locate again reversed, fmx_free — check_parity's order — for the jobs of
    replay_jobs().  Its answers equal the oracle's and neither sanitizer
    reports an error (the exit-time leak pass is off)."""
    jobs = replay_jobs(pkg, part)
    src, dst = tmp_path / "replay.in", tmp_path / "replay.out"
    with open(src, "wb") as f:
        f.write(struct.pack("<Q", len(jobs)))
        for st, text, table, sigma, lay, k, sr, pats, opts, claim, skew in jobs:
            data, offsets = pkg.pack_patterns(pats) if pats else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
            head = np.array([st, sigma, lay[0], lay[1], lay[2], 0 if table is not None else 1, k, sr, len(pats),
                             len(opts)] + list(opts) + [0] * (4 - len(opts)) + [claim, skew], np.uint64)
            _put(f, head, np.frombuffer(text, np.uint8), np.frombuffer(table or b"", np.uint8), data, offsets)
    env = {k: v for k, v in os.environ.items() if k != "FMX_BUILD_SA64"}
    env.update(FMX_DEEP_LUT_MB="1", FMX_FUSED="0", FMX_EMIT_CHAIN="0", SIMT_SEED="4664", SIMT_DEFER="1",
               # (no leak pass at exit: it needs ptrace, which a sandboxed test run may not have, and the
               # replay is after memory errors and undefined behaviour)
               ASAN_OPTIONS="abort_on_error=0:exitcode=99:detect_leaks=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    if path == "64":
        env["FMX_BUILD_SA64"] = "1"
    r = subprocess.run([replay_program, str(src), str(dst)], env=env,
                       capture_output=True, text=True)
    report = r.stderr[-4000:]
    assert r.returncode == 0, f"replay (SA path {path}) exited {r.returncode}: {report}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    buf = open(dst, "rb").read()
    at = 0
    for st, text, table, sigma, lay, k, sr, pats, opts, claim, skew in jobs:
        got, at = _get(buf, at)
        assert int(got.view(np.uint64)[0]) == st, (path, "fmx_build status", int(got.view(np.uint64)[0]), st)
        blob, at = _get(buf, at)
        if st:
            continue
        L = O.layout(lay[0], lay[1], lay[2])
        ref = O.build(text, sigma, L, k, sr, table)
        assert np.array_equal(blob, ref), (path, "blob", sigma, k, sr)
        enc = 0 if table is not None else 1
        data, offsets = pkg.pack_patterns(pats)
        ooff, olocs = O.OracleIndex(ref, O.layout(lay[0], lay[1], lay[2], enc)).locate_batch(data, offsets)
        for occ in opts:
            for what in ("forward", "reversed"):
                goff, at = _get(buf, at)
                glocs, at = _get(buf, at)
                gcnt, at = _get(buf, at)
                P = np.uint32 if lay[0] == 4 else np.uint64
                assert np.array_equal(goff.view(np.uint64), ooff), (path, sigma, occ, what, "offsets")
                assert np.array_equal(glocs.view(P), olocs.astype(P)), (path, sigma, occ, what, "locations")
                assert np.array_equal(gcnt.view(P).astype(np.uint64), np.diff(ooff)), (path, sigma, occ, what)
    assert at == len(buf)
