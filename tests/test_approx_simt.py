"""k-mismatch search (fmx_approx_batch: k_approx, then the locate's k_emit over
the slots) on the CPU: the engine's own sources under the SIMT shim
(tests/simt, as tests/test_seeds_simt.py), every output against the brute-force
values of _approx_cases.py.  Batches of 1, 255, 256, 257 and 700 patterns,
max_mm 0..2 (3 on patterns of at most 12 symbols), max_hits 1, 3 and 8 (3:
pattern 85's slots straddle the first tile boundary), forward and reversed,
FMX_APPROX_BEST; max_occ; a two-letter text (more than 32 variants per pattern);
ranges only; capacity; PassThrough bytes; the device call; argument checks."""
import ctypes as C

import numpy as np
import pytest

from _approx_cases import (BATCH_SIZES, assert_classes, batch, case_for, check_approx, compare, cross_check,
                           cross_check_exact, expected_arrays, open_index, variants)
from _match_cases import ABSENT
from _simt import simt_fixture


simt = simt_fixture(launch_order=True)


# (P bytes, planes, vector bits): the layouts of tests/test_seeds_simt.py
LAYOUTS = [(4, 3, 64), (8, 2, 32), (4, 5, 128), (8, 4, 64)]


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", LAYOUTS)
def test_approx_simt(pkg, O, simt, pb, planes, vb, n):
    """max_mm = 1 forward and max_mm = 2 reversed with FMX_APPROX_BEST, three
    slots per pattern, both occ layouts."""
    simt.simt_config(pb * 131 + planes * 17 + vb + n + 5, 0.5)
    case = case_for(planes)
    for occ in (0, 1):
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        p1, p2 = batch(case, n, 1), batch(case, n, 2)
        if n >= 256 and occ == 0:
            assert_classes(case, orc, p1, 1, 3)
            assert_classes(case, orc, p2, 2, 3)
        _, got = check_approx(ix, orc, case, p1, max_mm=1, max_hits=3, best=bool(occ))
        check_approx(ix, orc, case, p2, max_mm=2, max_hits=3, best=not occ, reversed=True)
        if n == 257 and occ == 1:
            cross_check(ix, case, p1, got)
        ix.close()


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("max_hits", [1, 8])
def test_approx_slot_counts_simt(pkg, O, simt, max_hits, n):
    """max_hits = 1: the search stops at the second variant; 8: the classes
    of the issue; max_mm = 0 is the exact search."""
    simt.simt_config(max_hits * 1013 + n, 0.5)
    case = case_for(3)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    for max_mm, rev in ((1, False), (2, True)):
        pats = batch(case, n, max_mm)
        if n >= 256:
            assert_classes(case, orc, pats, max_mm, max_hits)
        check_approx(ix, orc, case, pats, max_mm=max_mm, max_hits=max_hits, reversed=rev)
    pats = batch(case, n, 0)
    _, got = check_approx(ix, orc, case, pats, max_mm=0, max_hits=max_hits)
    if max_hits == 1:
        cross_check_exact(ix, pats, got)
    ix.close()


@pytest.mark.parametrize("best", [False, True])
def test_approx_three_mismatches_simt(pkg, O, simt, best):
    """max_mm = 3 (patterns of at most 12 symbols): all three frames."""
    simt.simt_config(333 + best, 0.5)
    case = case_for(3)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 257, 3, 12)
    exp, _ = check_approx(ix, orc, case, pats, max_mm=3, max_hits=8, best=best, reversed=best)
    assert set(np.unique(exp[2][exp[4][:, :, 1] > 0]).tolist()) == {0, 1, 2, 3}
    ix.close()


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_approx_two_letters_simt(pkg, O, simt, sr):
    """A two-letter text: dozens of variants per pattern (max_hits = 32 is
    exceeded), hits with hundreds of rows, and every sampling ratio's walk."""
    simt.simt_config(2900 + sr, 0.5)
    case = case_for(2, two_letters=True, k=3, sr=sr)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    pats = batch(case, 257, 2)
    exp, _ = check_approx(ix, orc, case, pats, max_mm=2, max_hits=32)
    assert exp[1].sum() >= 1 and (exp[0] == 32).sum() >= 1 and int(np.diff(exp[5]).max()) >= 100
    check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, reversed=True, max_occ=40)
    ix.close()


def test_approx_filters_simt(pkg, O, simt):
    """max_occ only selects which hits are located: everything else is the
    same across max_occ."""
    simt.simt_config(178, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 257, 1)
    first = None
    for max_occ in (0, 1, 10, None):
        exp, got = check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, max_occ=max_occ)
        first = first or got
        assert all(np.array_equal(got[j], first[j]) for j in range(5))
        if max_occ == 0:
            assert got[6].size == 0
    ix.close()


def test_approx_ranges_only_and_capacity_simt(pkg, O, simt):
    simt.simt_config(5253, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 300, 1)
    check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, locate=False)
    for p in (pats[5], pats[40], pats[200]):
        assert ix.approx(p, 2, 8) == [x[:4] for x in variants(case, orc, p, 2)[:8]]
        assert ix.approx(p, 2, 8, best=True) == [x[:4] for x in variants(case, orc, p, 2) if
                                                x[0] == variants(case, orc, p, 2)[0][0]][:8]
    assert ix.approx(b"") == [] and ix.approx(bytes([ABSENT]) * 2) == []
    # a cap below needed: FMX_E_CAPACITY, needed exact, everything but the locations written
    mh, n = 3, len(pats)
    exp = expected_arrays(case, orc, pats, 1, mh, False, None)
    total = int(exp[5][-1])
    data, offsets = pkg.pack_patterns(pats)
    lib, nat = pkg._native.lib(), pkg._native

    def call(cap, nh_ptr=True, max_mm=1, max_hits=mh, mode=0):
        o = [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full((n, mh), 7, np.uint32),
             np.full((n, mh, 3, 2), 7, np.uint32), np.full((n, mh, 2), 7, np.uint32), np.full(n * mh + 1, 7, np.uint64),
             np.full(max(total, 1), 7, np.uint32)]
        needed = C.c_uint64(99)
        st = lib.fmx_approx_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, max_mm, max_hits, mode,
                                  (1 << 64) - 1, o[0].ctypes.data if nh_ptr else None, o[1].ctypes.data,
                                  o[2].ctypes.data, o[3].ctypes.data, o[4].ctypes.data, o[5].ctypes.data,
                                  o[6].ctypes.data, cap, C.byref(needed))
        return st, needed.value, o
    short = total - 1
    st, needed, o = call(short)
    assert st == nat.FMX_E_CAPACITY and needed == total
    compare(o[:5], exp, locate=False)
    assert np.array_equal(o[5], exp[5])
    st, needed, o = call(total)
    assert st == 0 and needed == total
    compare(o[:6] + [o[6][:total]], exp)
    # argument checks
    assert call(total, max_mm=4)[0] == nat.FMX_E_ARG
    assert call(total, max_hits=0)[0] == nat.FMX_E_ARG and call(total, max_hits=33)[0] == nat.FMX_E_ARG
    assert call(total, mode=2)[0] == nat.FMX_E_ARG and call(total, mode=3)[0] == nat.FMX_E_ARG
    assert call(total, nh_ptr=False)[0] == nat.FMX_E_ARG
    ix.close()


def test_approx_pass_through_simt(pkg, O, simt):
    """PassThrough: a byte >= symbol_count is matched only by substituting it
    (no FMX_E_SYMBOL, nothing latched)."""
    simt.simt_config(708, 0.5)
    rng = np.random.default_rng(14)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, where = [], []
    for m in (1, 2, 5, 9, 12) * 8:
        s = int(rng.integers(0, len(text) - m))
        for bad in (9, 200, 5):
            j = int(rng.integers(0, m))
            q = bytearray(text[s:s + m])
            q[j] = bad
            pats.append(bytes(q))
            where.append(j)
    two = bytearray(text[100:110])
    two[3], two[8] = 77, 6
    pats.append(bytes(two))
    where.append(None)
    nh0 = ix.approx_batch(pats, max_mm=0, max_hits=4, locate=False)[0]
    assert not nh0.any()
    nh, more, mm, subs, rg, loff, locs = ix.approx_batch(pats, max_mm=1, max_hits=4)
    for i, (p, j) in enumerate(zip(pats, where)):
        if j is None:
            assert nh[i] == 0
            continue
        want = []
        for c in range(4):  # ascending symbol order; the own symbol cannot be kept
            v = p[:j] + bytes([c]) + p[j + 1:]
            if orc.count(v):
                want.append((c, v))
        assert nh[i] == len(want) >= 1 and more[i] == 0, (i, p)
        for h, (c, v) in enumerate(want):
            assert mm[i, h] == 1 and subs[i, h].tolist() == [[j, c], [0, 0], [0, 0]]
            assert int(rg[i, h, 1] - rg[i, h, 0]) == orc.count(v)
            assert locs[int(loff[4 * i + h]):int(loff[4 * i + h + 1])].tolist() == orc.locate(v)
    nh2, _, mm2, subs2, _ = ix.approx_batch(pats[-1:], max_mm=2, max_hits=32, locate=False)
    assert nh2[0] >= 1 and (mm2[0, :nh2[0]] == 2).all()
    assert (subs2[0, :nh2[0], 0, 0] == 8).all() and (subs2[0, :nh2[0], 1, 0] == 3).all()
    ix.sync()  # nothing latched
    ix.close()


def test_approx_async_simt(pkg, O, simt):
    """fmx_approx_batch_async (on the emulator, device memory is host memory):
    with locations over a garbage workspace and prefilled outputs, ranges only
    with no workspace, a disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the
    "approx" timer, the argument checks."""
    simt.simt_config(617, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 300, 2)
    mh, n = 3, len(pats)
    exp = expected_arrays(case, orc, pats, 2, mh, True, 10)
    total = int(exp[5][-1])
    data, offsets = pkg.pack_patterns(pats)
    rnd = np.random.default_rng(4)
    mk = lambda shape, dt=np.uint32: rnd.integers(1, 2**31, shape).astype(dt)  # noqa: E731
    o = [mk(n), mk(n), mk((n, mh)), mk((n, mh, 3, 2)), mk((n, mh, 2)), mk(n * mh + 1, np.uint64), mk(total + 4)]
    tail = o[6][total:].copy()
    need = mk(1, np.uint64)
    wsb = ix.locate_workspace_size(n * mh)
    ws = pkg.aligned_buffer(wsb)
    ws[:] = rnd.integers(0, 256, wsb).astype(np.uint8)
    ptr = [x.ctypes.data for x in o]
    ix.timing_enable(True)
    ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *ptr, total + 4, need.ctypes.data, ws.ctypes.data,
                          wsb, max_mm=2, max_hits=mh, best=True, max_occ=10)
    ix.sync()
    t = ix.timing_read()["approx"]
    assert t["launches"] == 1 and t["units"] == n * mh
    ix.timing_enable(False)
    assert int(need[0]) == total
    compare(o[:6] + [o[6][:total]], exp)
    assert np.array_equal(o[6][total:], tail)
    # ranges only: no workspace, no location arguments
    o2 = [mk(n), mk(n), mk((n, mh)), mk((n, mh, 3, 2)), mk((n, mh, 2))]
    p2 = [x.ctypes.data for x in o2]
    ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *p2, max_mm=2, max_hits=mh, best=True)
    ix.sync()
    compare(o2, exp, locate=False)
    # argument checks
    for kw in (dict(max_hits=0), dict(max_hits=33), dict(max_mm=4)):
        with pytest.raises(pkg.FmxError) as e:
            ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *p2, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    for z in range(5):  # every required pointer
        q = list(p2)
        q[z] = 0
        with pytest.raises(pkg.FmxError) as e:
            ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *q, max_hits=mh)
        assert e.value.code == pkg._native.FMX_E_ARG
    lib = pkg._native.lib()
    v = C.c_void_p
    assert lib.fmx_approx_batch_async(ix.handle, v(data.ctypes.data), v(offsets.ctypes.data), n, 0, 1, mh, 2, 0,
                                      *[v(x) for x in p2], None, None, 0, None, None, 0, None) == pkg._native.FMX_E_ARG
    # locations without a workspace, or without d_needed
    with pytest.raises(pkg.FmxError) as e:
        ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *ptr, total, need.ctypes.data, 0, 0, max_hits=mh)
    assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *ptr, total, 0, ws.ctypes.data, wsb, max_hits=mh)
    assert e.value.code == pkg._native.FMX_E_ARG
    # more slots than a launch's tiles hold (checked before any pointer is used)
    assert lib.fmx_approx_batch_async(ix.handle, v(data.ctypes.data), v(offsets.ctypes.data), (1 << 40), 0, 1, 32, 0, 0,
                                      *[v(x) for x in p2], None, None, 0, None, None, 0, None) == pkg._native.FMX_E_ARG
    # a fixed-length hint the offsets disagree with
    ix.approx_batch_async(data.ctypes.data, offsets.ctypes.data, n, *p2, max_hits=mh, fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
