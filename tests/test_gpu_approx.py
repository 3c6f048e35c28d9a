"""k-mismatch search on the GPU (fmx_approx_batch: k_approx, then the locate's
k_emit over the slots): the cases of tests/test_approx_simt.py on the gfx950
kernels — every layout and load options 0 and 1 at max_hits = 3, max_hits 1
and 8 and every derived structure (63: they must not change a result) for two
layouts, max_mm 0..3, FMX_APPROX_BEST, forward and reversed, batches of 1, 255,
256, 257 and 700 patterns, a two-letter text at sampling ratios 1..4, the
unstaged pattern path and a caller's stream.  Expected values: the brute force
of _approx_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

from _approx_cases import (BATCH_SIZES, assert_classes, batch, case_for, check_approx, compare, cross_check,
                           cross_check_exact, expected_arrays, open_index, variants)
from _match_cases import ABSENT
from _util import ALL_LAYOUTS

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def sweep(pkg, O, case, pb, planes, vb, options, hit_counts):
    for occ in options:
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        for n in BATCH_SIZES:
            p1, p2 = batch(case, n, 1), batch(case, n, 2)
            for mh in hit_counts:
                if n >= 256 and occ == options[0]:  # (on the expected values alone, before anything is compared)
                    assert_classes(case, orc, p1, 1, mh)
                    assert_classes(case, orc, p2, 2, mh)
                _, got = check_approx(ix, orc, case, p1, max_mm=1, max_hits=mh, best=mh == 1)
                check_approx(ix, orc, case, p2, max_mm=2, max_hits=mh, best=mh != 1, reversed=True)
            if n == 257:
                cross_check(ix, case, p1, got)
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_approx_every_layout(pkg, O, pb, planes, vb):
    sweep(pkg, O, case_for(planes), pb, planes, vb, (0, 1), (3,))


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_approx_slot_counts(pkg, O, pb, planes, vb):
    """max_hits = 1: the search stops at the second variant; 8: the classes
    of the issue; max_mm = 0 is the exact search; max_mm = 3 on patterns of at
    most 12 symbols."""
    case = case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (1,), (1, 8))
    ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
    pats = batch(case, 700, 0)
    _, got = check_approx(ix, orc, case, pats, max_mm=0, max_hits=1)
    cross_check_exact(ix, pats, got)
    pats = batch(case, 257, 3, 12)
    for best in (False, True):
        exp, _ = check_approx(ix, orc, case, pats, max_mm=3, max_hits=8, best=best, reversed=best)
    assert set(np.unique(exp[2][exp[4][:, :, 1] > 0]).tolist()) == {0, 1, 2, 3}
    ix.close()


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_approx_ignore_derived_structures(pkg, O, pb, planes, vb):
    """FMX_OPT_DERIVED (deep table, full SA, text, row contexts, single-row
    entries): the search reads none of them (a loaded full SA serves the
    locations), and the results are identical."""
    case = case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (63,), (3,))
    pats = batch(case, 700, 2)
    outs = []
    for occ in (1, 63):
        ix, _ = open_index(pkg, O, case, pb, planes, vb, occ)
        outs.append(ix.approx_batch(pats, max_mm=2, max_hits=3))
        ix.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("sr", [1, 2, 3, 4])
def test_approx_two_letters(pkg, O, sr):
    """A two-letter text: dozens of variants per pattern (max_hits = 32 is
    exceeded), hits with hundreds of rows (the row dealing of k_emit), under
    every sampling ratio's walk."""
    case = case_for(2, two_letters=True, k=3, sr=sr)
    for pb, vb in ((4, 64), (8, 32)):
        ix, orc = open_index(pkg, O, case, pb, 2, vb, 1)
        pats = batch(case, 700, 2)
        exp, _ = check_approx(ix, orc, case, pats, max_mm=2, max_hits=32)
        assert exp[1].sum() >= 1 and (exp[0] == 32).sum() >= 1 and int(np.diff(exp[5]).max()) >= 100
        check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, reversed=True, max_occ=40)
        ix.close()


def test_approx_filters(pkg, O):
    """max_occ only selects which hits are located: everything else is the
    same across max_occ."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700, 1)
    first = None
    for max_occ in (0, 1, 10, None):
        exp, got = check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, max_occ=max_occ)
        first = first or got
        assert all(np.array_equal(got[j], first[j]) for j in range(5))
        if max_occ == 0:
            assert got[6].size == 0
    ix.close()


def test_approx_ranges_only_and_capacity(pkg, O):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700, 1)
    check_approx(ix, orc, case, pats, max_mm=1, max_hits=3, locate=False)
    for p in (pats[5], pats[40], pats[200]):
        v = variants(case, orc, p, 2)
        assert ix.approx(p, 2, 8) == [x[:4] for x in v[:8]]
        assert ix.approx(p, 2, 8, best=True) == [x[:4] for x in v if x[0] == v[0][0]][:8]
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
    st, needed, o = call(total - 1)
    assert st == nat.FMX_E_CAPACITY and needed == total
    compare(o[:5], exp, locate=False)
    assert np.array_equal(o[5], exp[5])
    st, needed, o = call(total)
    assert st == 0 and needed == total
    compare(o[:6] + [o[6][:total]], exp)
    # argument checks
    assert call(total, max_mm=4)[0] == nat.FMX_E_ARG
    assert call(total, max_hits=0)[0] == nat.FMX_E_ARG and call(total, max_hits=33)[0] == nat.FMX_E_ARG
    assert call(total, mode=2)[0] == nat.FMX_E_ARG
    assert call(total, nh_ptr=False)[0] == nat.FMX_E_ARG
    ix.close()


def test_approx_pass_through(pkg, O):
    """PassThrough: a byte >= symbol_count is matched only by substituting it
    (no FMX_E_SYMBOL, nothing latched)."""
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
    assert not ix.approx_batch(pats, max_mm=0, max_hits=4, locate=False)[0].any()
    nh, more, mm, subs, rg, loff, locs = ix.approx_batch(pats, max_mm=1, max_hits=4)
    for i, (p, j) in enumerate(zip(pats, where)):
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
    ix.sync()  # nothing latched
    ix.close()


def _device_call(pkg, ix, torch, pats, exp, mh, stream, **kw):
    """One fmx_approx_batch_async over HBM-resident buffers with prefilled
    outputs and a garbage workspace; returns the outputs as numpy arrays."""
    n, total = len(pats), int(exp[5][-1])
    data, offsets = pkg.pack_patterns(pats)
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    fill = lambda shape, dt=torch.int32: torch.full(shape, -1, dtype=dt, device=dev)  # noqa: E731
    o = [fill((n,)), fill((n,)), fill((n, mh)), fill((n, mh, 3, 2)), fill((n, mh, 2)),
         fill((n * mh + 1,), torch.int64), fill((total + 4,))]
    d_need = fill((1,), torch.int64)
    wsb = ix.locate_workspace_size(n * mh)
    d_ws = torch.randint(0, 256, (wsb,), dtype=torch.uint8, device=dev)  # (a workspace needs no initialisation)
    torch.cuda.synchronize()  # (buffers made on torch's stream)
    ix.approx_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *[x.data_ptr() for x in o], total + 4,
                          d_need.data_ptr(), d_ws.data_ptr(), wsb, max_hits=mh, stream=stream, **kw)
    ix.sync(stream)
    assert int(d_need.item()) == total
    h = [x.cpu().numpy() for x in o]
    assert (h[6][total:] == -1).all()
    got = [x.view(np.uint32) for x in h[:5]] + [h[5].view(np.uint64), h[6].view(np.uint32)[:total]]
    compare(got, exp)
    return o, (d_data, d_off)


def test_approx_unstaged_patterns(pkg, O):
    """A 1 KB stage: no full tile of the batch fits, so k_approx reads every
    pattern from HBM, forward and reversed."""
    import torch
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700, 2)
    assert min(sum(len(p) for p in pats[t:t + 256]) for t in (0, 256)) > 1024
    exp = expected_arrays(case, orc, pats, 2, 3, False, 10)
    _device_call(pkg, ix, torch, pats, exp, 3, 0, max_mm=2, max_occ=10, stage_kb=1)
    _device_call(pkg, ix, torch, [p[::-1] for p in pats], exp, 3, 0, max_mm=2, max_occ=10, stage_kb=1, reversed=True)
    ix.close()


def test_approx_async_on_a_caller_stream(pkg, O):
    """fmx_approx_batch_async on a stream of the caller's: with locations,
    ranges only with no workspace, a disagreeing FMX_HINT_FIXED_LEN still
    FMX_E_ARG, the "approx" timer, the argument checks."""
    import torch
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700, 2)
    mh, n = 3, len(pats)
    exp = expected_arrays(case, orc, pats, 2, mh, True, 10)
    st = torch.cuda.Stream()
    ix.timing_enable(True)
    o, (d_data, d_off) = _device_call(pkg, ix, torch, pats, exp, mh, st.cuda_stream, max_mm=2, best=True, max_occ=10)
    t = ix.timing_read()["approx"]
    assert t["launches"] == 1 and t["units"] == n * mh
    ix.timing_enable(False)
    fill = lambda shape: torch.full(shape, -1, dtype=torch.int32, device=d_data.device)  # noqa: E731
    o2 = [fill((n,)), fill((n,)), fill((n, mh)), fill((n, mh, 3, 2)), fill((n, mh, 2))]
    p2 = [x.data_ptr() for x in o2]
    torch.cuda.synchronize()
    ix.approx_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *p2, max_mm=2, max_hits=mh, best=True,
                          stream=st.cuda_stream)
    ix.sync(st.cuda_stream)
    assert all(torch.equal(a, b) for a, b in zip(o2, o[:5]))
    for kw in (dict(max_hits=0), dict(max_hits=33), dict(max_mm=4)):
        with pytest.raises(pkg.FmxError) as e:
            ix.approx_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *p2, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        ix.approx_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, 0, *p2[1:], max_hits=mh)
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.approx_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *p2, max_hits=mh, fixed_len=7, stream=st.cuda_stream)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync(st.cuda_stream)
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
