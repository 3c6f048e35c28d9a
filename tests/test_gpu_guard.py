"""Guard bands around the device-buffer API on the GPU: the cases and the
check of tests/_guard_cases.py (as tests/test_guard_simt.py runs them on the
emulator) on the gfx950 kernels, every buffer of a call carved out of ONE
0xA5-filled tensor at its exact size and weakest allowed alignment, the whole
tensor read back after every launch.

The full matrix: every launch path (split, fused, grouped with packed and
with id-only records, chained emit; fmx_index_info's counters asserted) x
layouts (4,3,64), (8,3,128), (4,5,64) with 21 symbols x load options 0 and 1
(and every derived structure, 63, for (4,3,64) in launch order) x d_bytes
skews 0, 1, 7, 15 x forward / reversed x batch shapes x batches of 1, 255,
256, 257 and 700 patterns x caps total, total-1, inside a heavy pattern's run
mid-wave, on a pattern boundary, 1, and 0 with d_locs = NULL; the group call
(five batches, own caps and workspaces, one arena); the match with and
without locations; the count; the host calls' capacity contract.

Nothing a correct or a broken kernel of this engine touches lies outside the
tensor (the guards are 4 KiB, the widest access 16 B, and d_locs is followed
by guard bytes for every location past cap): a regression fails an assert
here."""
import os

import pytest

import _guard_cases as G

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")

GROUP_PARAMS = [(path,) + ixp for path in G.PATHS for ixp in G.INDEXES if ixp[4] != 63]


@pytest.mark.parametrize("skew", G.SKEWS)
@pytest.mark.parametrize("param", G.LOCATE_PARAMS, ids=G.ids)
def test_locate_guard(pkg, O, monkeypatch, param, skew):
    """fmx_locate_batch_async (forward) / fmx_locate_jobs_async (reversed) on
    one path at one skew: every shape x size x cap, both directions."""
    path, pb, planes, vb, nch, opt = param
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, path)
    shapes = G.shapes_for(path, opt)
    if opt == 63:
        G.assert_scan_live(ix, case, orc, path)
    ran = dict.fromkeys(G.CAP_NAMES, 0)
    for shape in shapes:
        for n in G.BATCH_SIZES:
            for cap in G.CAP_NAMES:
                for rev in (False, True):
                    ran[cap] += G.run_locate(pkg, ix, G.TorchMem, case, orc, pb, path, shape, n, cap, skew, rev,
                                             via_jobs=rev)
    assert all(ran.values()), f"a cap never ran: {ran}"
    ix.close()


@pytest.mark.parametrize("param", GROUP_PARAMS, ids=G.ids)
def test_group_guard(pkg, O, monkeypatch, param):
    """fmx_locate_group_async: five batches with their own caps and
    workspaces in one arena, at every skew, forward and reversed."""
    path, pb, planes, vb, nch, opt = param
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, path)
    for skew in G.SKEWS:
        for rev in (False, True):
            G.run_group(pkg, ix, G.TorchMem, case, orc, pb, path, skew, rev)
    ix.close()


@pytest.mark.parametrize("ixp", G.INDEXES, ids=G.ids)
def test_match_guard(pkg, O, monkeypatch, ixp):
    """fmx_match_batch_async with locations (min_len / max_occ keep some
    patterns from reporting) and with lengths and intervals only."""
    pb, planes, vb, nch, opt = ixp
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, "split")
    ran = dict.fromkeys(G.CAP_NAMES, 0)
    for skew in G.SKEWS:
        for rev in (False, True):
            for n in G.BATCH_SIZES:
                for cap in G.CAP_NAMES:
                    ran[cap] += G.run_match(pkg, ix, G.TorchMem, case, orc, pb, n, cap, skew, rev)
                G.run_match(pkg, ix, G.TorchMem, case, orc, pb, n, None, skew, rev, locate=False)
    # (no reporting match of a 21-symbol text has a hundred occurrences: no cap inside such a run)
    assert all(v for c, v in ran.items() if c != "mid-run" or nch <= 8), f"a cap never ran: {ran}"
    ix.close()


@pytest.mark.parametrize("ixp", G.INDEXES, ids=G.ids)
def test_count_guard(pkg, O, monkeypatch, ixp):
    """fmx_count_batch_async, ragged and with the fixed-length hint."""
    pb, planes, vb, nch, opt = ixp
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, opt, "split")
    for skew in G.SKEWS:
        for rev in (False, True):
            for n in G.BATCH_SIZES:
                for shape, fixed in (("ragged", False), ("single", True), ("heavy", True), ("heavy", False)):
                    G.run_count(pkg, ix, G.TorchMem, case, orc, pb, shape, n, skew, rev, fixed=fixed)
    ix.close()


@pytest.mark.parametrize("match", [False, True], ids=["locate", "match"])
@pytest.mark.parametrize("pb,planes,vb,nch", [lay for lay in G.LAYOUTS if lay[3] == 4], ids=G.ids)
def test_host_capacity(pkg, O, monkeypatch, pb, planes, vb, nch, match):
    """FMX_E_CAPACITY of the host-buffer calls: needed and offsets written,
    out_locs untouched; then the exact cap on the same index (two passes)."""
    case = G.case_for(nch)
    ix, orc = G.open_index(pkg, O, monkeypatch, case, pb, planes, vb, 1, "split")
    G.check_host_capacity(pkg, ix, case, orc, pb, match=match)
    ix.close()
