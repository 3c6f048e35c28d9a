"""Greedy seed chains on the GPU (fmx_seeds_batch: k_seeds, then the locate's
k_emit over the slots): the cases of tests/test_seeds_simt.py on the gfx950
kernels — every layout and load options 0 and 1 at max_seeds = 3, max_seeds 1
and 8 and every derived structure (63: they must not change a result) for two
layouts, skip 0 and 1, forward and reversed, batches of 1, 255, 256, 257 and
700 patterns.  Expected values: _seed_cases.py (the loop of include/fmx.h run
in Python over _match_cases.Case.expected)."""
import ctypes as C
import os

import numpy as np
import pytest

from _match_cases import ABSENT
from _seed_cases import (BATCH_SIZES, assert_classes, batch, case_for, chain, check_seeds, compare, cross_check,
                         expected_arrays, open_index)
from _util import ALL_LAYOUTS

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def sweep(pkg, O, case, pb, planes, vb, options, seed_counts):
    for occ in options:
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        for n in BATCH_SIZES:
            pats = batch(case, n)
            if n >= 256 and occ == options[0]:  # (on the expected values alone, before anything is compared)
                assert_classes(case, orc, pats, 0)
                assert_classes(case, orc, pats, 1)
            for ms in seed_counts:
                for skip in (0, 1):
                    _, got = check_seeds(ix, orc, case, pats, max_seeds=ms, skip=skip, reversed=skip == 0)
                    check_seeds(ix, orc, case, pats, max_seeds=ms, skip=skip, reversed=skip == 1)
                if n >= 256:
                    cross_check(ix, pats, got)
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_seeds_every_layout(pkg, O, pb, planes, vb):
    sweep(pkg, O, case_for(planes), pb, planes, vb, (0, 1), (3,))


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_seeds_slot_counts(pkg, O, pb, planes, vb):
    """max_seeds = 1: parsing stops after one seed with rest exact; 8: the
    20-seed pattern runs out of slots."""
    case = case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (1,), (1, 8))
    ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
    pats = batch(case, 700)
    for ms in (1, 8):
        exp = expected_arrays(case, orc, pats, ms, 1, 0, None)
        assert (exp[1] > 0).sum() >= (30 if ms == 1 else 1), "no pattern ran out of slots"
    ix.close()


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_seeds_ignore_derived_structures(pkg, O, pb, planes, vb):
    """FMX_OPT_DERIVED (deep table, full SA, text, row contexts, single-row
    entries): the search reads none of them (a loaded full SA serves the
    locations), and the results are identical."""
    case = case_for(planes)
    sweep(pkg, O, case, pb, planes, vb, (63,), (3,))
    pats = batch(case, 700)
    outs = []
    for occ in (1, 63):
        ix, _ = open_index(pkg, O, case, pb, planes, vb, occ)
        outs.append(ix.seeds_batch(pats, max_seeds=3, skip=1))
        ix.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_seeds_two_letters(pkg, O, sr):
    """A two-letter text: seeds with hundreds of rows (the row dealing of
    k_emit), under every sampling ratio's walk."""
    case = case_for(2, two_letters=True, k=3, sr=sr)
    for pb, vb in ((4, 64), (8, 32)):
        ix, orc = open_index(pkg, O, case, pb, 2, vb, 1)
        pats = batch(case, 700)
        exp, _ = check_seeds(ix, orc, case, pats, max_seeds=3, skip=1)
        assert int(np.diff(exp[4]).max()) >= 300
        check_seeds(ix, orc, case, pats, max_seeds=3, reversed=True, max_occ=400)
        ix.close()


@pytest.mark.parametrize("min_len", [1, 5])
def test_seeds_filters(pkg, O, min_len):
    """min_len decides what is a seed; max_occ only which seeds are located:
    spans and ranges are the same across max_occ."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700)
    first = None
    for max_occ in (0, 1, 10, None):
        exp, got = check_seeds(ix, orc, case, pats, max_seeds=3, min_len=min_len, skip=1, max_occ=max_occ)
        first = first or got
        assert np.array_equal(got[2], first[2]) and np.array_equal(got[3], first[3])
        if max_occ == 0:
            assert got[5].size == 0
    if min_len == 5:
        assert (exp[0] == 0).sum() >= 30 and (exp[2][:, :, 1][exp[2][:, :, 1] > 0] >= 5).all()
    ix.close()


def test_seeds_ranges_only_and_capacity(pkg, O):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700)
    check_seeds(ix, orc, case, pats, max_seeds=3, skip=1, locate=False)
    s, rest = chain(case, orc, pats[5], 8, 1, 0)
    assert ix.seeds(pats[5]) == [x[:4] for x in s] and rest == 0
    assert ix.seeds(b"") == [] and ix.seeds(bytes([ABSENT])) == []
    many = bytes([ABSENT, case.chars[0]]) * 20
    assert many in pats and len(ix.seeds(many, max_seeds=32)) == 20
    # a cap below needed: FMX_E_CAPACITY, needed exact, everything but the locations written
    ms, n = 3, len(pats)
    exp = expected_arrays(case, orc, pats, ms, 1, 0, None)
    total = int(exp[4][-1])
    data, offsets = pkg.pack_patterns(pats)
    lib, nat = pkg._native.lib(), pkg._native

    def call(cap, ns_ptr=True, max_seeds=ms):
        o = [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full((n, ms, 2), 7, np.uint32),
             np.full((n, ms, 2), 7, np.uint32), np.full(n * ms + 1, 7, np.uint64), np.full(max(total, 1), 7, np.uint32)]
        needed = C.c_uint64(99)
        st = lib.fmx_seeds_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, max_seeds, 1, 0, (1 << 64) - 1,
                                 o[0].ctypes.data if ns_ptr else None, o[1].ctypes.data, o[2].ctypes.data,
                                 o[3].ctypes.data, o[4].ctypes.data, o[5].ctypes.data, cap, C.byref(needed))
        return st, needed.value, o
    st, needed, o = call(total - 1)
    assert st == nat.FMX_E_CAPACITY and needed == total
    compare(o[:4], exp, locate=False)
    assert np.array_equal(o[4], exp[4])
    st, needed, o = call(total)
    assert st == 0 and needed == total
    compare(o[:5] + [o[5][:total]], exp)
    # argument checks
    assert call(total, max_seeds=0)[0] == nat.FMX_E_ARG and call(total, max_seeds=33)[0] == nat.FMX_E_ARG
    assert call(total, ns_ptr=False)[0] == nat.FMX_E_ARG
    ix.close()


def test_seeds_pass_through(pkg, O):
    """PassThrough: bytes >= symbol_count in mid-pattern split it into seeds
    on both sides (no FMX_E_SYMBOL, nothing latched)."""
    rng = np.random.default_rng(13)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, parts = [], []
    for la, lb in [(1, 1), (2, 3), (3, 2), (9, 4), (4, 9), (12, 12)] * 6:
        a0, b0 = int(rng.integers(0, len(text) - la)), int(rng.integers(0, len(text) - lb))
        a, b = text[a0:a0 + la], text[b0:b0 + lb]
        for bad in (bytes([9]), bytes([200]), bytes([4, 77])):
            pats.append(a + bad + b)
            parts.append((a, bad, b))
    for skip in (0, 1):
        ns, rest, spans, rg, loff, locs = ix.seeds_batch(pats, max_seeds=4, skip=skip)
        for i, (a, bad, b) in enumerate(parts):
            m = len(pats[i])
            assert ns[i] == 2 and rest[i] == 0, (i, pats[i])
            assert spans[i, :2].tolist() == [[m, len(b)], [len(a), len(a)]] and spans[i, 2:].tolist() == [[0, 0]] * 2
            for j, sub in enumerate((b, a)):
                assert int(rg[i, j, 1] - rg[i, j, 0]) == orc.count(sub)
                assert locs[int(loff[4 * i + j]):int(loff[4 * i + j + 1])].tolist() == orc.locate(sub)
    ix.sync()  # nothing latched
    ix.close()


def test_seeds_async(pkg, O):
    """fmx_seeds_batch_async on HBM-resident buffers: with locations over a
    garbage workspace and prefilled outputs, ranges only with no workspace, a
    disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the "seeds" timer, the
    argument checks."""
    import torch
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 700)
    ms, n = 3, len(pats)
    exp = expected_arrays(case, orc, pats, ms, 5, 1, 10)
    total = int(exp[4][-1])
    data, offsets = pkg.pack_patterns(pats)
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    fill = lambda shape, dt=torch.int32: torch.full(shape, -1, dtype=dt, device=dev)  # noqa: E731
    o = [fill((n,)), fill((n,)), fill((n, ms, 2)), fill((n, ms, 2)), fill((n * ms + 1,), torch.int64), fill((total + 4,))]
    d_need = fill((1,), torch.int64)
    wsb = ix.locate_workspace_size(n * ms)
    d_ws = torch.randint(0, 256, (wsb,), dtype=torch.uint8, device=dev)  # (a workspace needs no initialisation)
    torch.cuda.synchronize()  # (buffers made on torch's stream; the index launches on its own)
    ptr = [x.data_ptr() for x in o]
    ix.timing_enable(True)
    ix.seeds_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5],
                         total + 4, d_need.data_ptr(), d_ws.data_ptr(), wsb, max_seeds=ms, min_len=5, skip=1, max_occ=10)
    ix.sync()
    assert ix.timing_read()["seeds"]["launches"] == 1
    ix.timing_enable(False)
    assert int(d_need.item()) == total
    h = [x.cpu().numpy() for x in o]
    compare([h[0].view(np.uint32), h[1].view(np.uint32), h[2].view(np.uint32), h[3].view(np.uint32),
             h[4].view(np.uint64), h[5].view(np.uint32)[:total]], exp)
    assert (h[5][total:] == -1).all()
    o2 = [fill((n,)), fill((n,)), fill((n, ms, 2)), fill((n, ms, 2))]
    p2 = [x.data_ptr() for x in o2]
    torch.cuda.synchronize()
    ix.seeds_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *p2, max_seeds=ms, min_len=5, skip=1)
    ix.sync()
    assert all(torch.equal(a, b) for a, b in zip(o2, o[:4]))
    for kw in (dict(max_seeds=0), dict(max_seeds=33)):
        with pytest.raises(pkg.FmxError) as e:
            ix.seeds_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *p2, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        ix.seeds_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, 0, *p2[1:], max_seeds=ms)
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.seeds_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, *p2, max_seeds=ms, fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
