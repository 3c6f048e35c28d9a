"""Greedy seed chains (fmx_seeds_batch: k_seeds, then the locate's k_emit over
the slots) on the CPU: the engine's own sources under the SIMT shim
(tests/simt, as tests/test_match_simt.py), every output against the values of
_seed_cases.py — the loop of include/fmx.h run in Python over
_match_cases.Case.expected.  Batches of 1, 255, 256, 257 and 700 patterns,
max_seeds 1, 3 and 8 (3: pattern 85's slots straddle the first tile boundary, a
257-pattern batch ends in a 3-slot tile), skip 0 and 1, forward and reversed;
min_len / max_occ; a two-letter text (hundreds of rows per seed); ranges only;
capacity; PassThrough bytes; the device call; argument checks."""
import ctypes as C

import numpy as np
import pytest

from _match_cases import ABSENT
from _seed_cases import (BATCH_SIZES, assert_classes, batch, case_for, chain, check_seeds, compare, cross_check,
                         expected_arrays, open_index)
from _simt import simt_fixture


simt = simt_fixture(launch_order=True)


# (P bytes, planes, vector bits): the layouts of tests/test_match_simt.py
LAYOUTS = [(4, 3, 64), (8, 2, 32), (4, 5, 128), (8, 4, 64)]


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", LAYOUTS)
def test_seeds_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 131 + planes * 17 + vb + n + 3, 0.5)
    case = case_for(planes)
    pats = batch(case, n)
    for occ in (0, 1):
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        if n >= 256 and occ == 0:
            assert_classes(case, orc, pats, 0)
            assert_classes(case, orc, pats, 1)
        _, got = check_seeds(ix, orc, case, pats, max_seeds=3, skip=occ)
        check_seeds(ix, orc, case, pats, max_seeds=3, skip=1 - occ, reversed=True)
        if n >= 256 and occ == 1:
            cross_check(ix, pats, got)
        ix.close()


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("max_seeds", [1, 8])
def test_seeds_slot_counts_simt(pkg, O, simt, max_seeds, n):
    """max_seeds = 1: parsing stops after one seed with rest exact; 8: the
    20-seed pattern runs out of slots."""
    simt.simt_config(max_seeds * 1009 + n, 0.5)
    case = case_for(3)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, n)
    for skip, rev in ((0, False), (1, True)):
        exp, _ = check_seeds(ix, orc, case, pats, max_seeds=max_seeds, skip=skip, reversed=rev)
        if n >= 256:
            assert (exp[1] > 0).sum() >= (30 if max_seeds == 1 else 1), "no pattern ran out of slots"
    ix.close()


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_seeds_two_letters_simt(pkg, O, simt, sr):
    """A two-letter text: seeds with hundreds of rows (the row dealing of
    k_emit), and every sampling ratio's walk."""
    simt.simt_config(1900 + sr, 0.5)
    case = case_for(2, two_letters=True, k=3, sr=sr)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    pats = batch(case, 257)
    exp, _ = check_seeds(ix, orc, case, pats, max_seeds=3, skip=1)
    assert int(np.diff(exp[4]).max()) >= 300
    check_seeds(ix, orc, case, pats, max_seeds=3, reversed=True, max_occ=400)
    ix.close()


@pytest.mark.parametrize("min_len", [1, 5])
def test_seeds_filters_simt(pkg, O, simt, min_len):
    """min_len decides what is a seed; max_occ only which seeds are located:
    spans and ranges are the same across max_occ."""
    simt.simt_config(177 + min_len, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 257)
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


def test_seeds_ranges_only_and_capacity_simt(pkg, O, simt):
    simt.simt_config(5252, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 300)
    check_seeds(ix, orc, case, pats, max_seeds=3, skip=1, locate=False)
    s, rest = chain(case, orc, pats[5], 8, 1, 0)
    assert ix.seeds(pats[5]) == [x[:4] for x in s] and rest == 0
    assert ix.seeds(b"") == [] and ix.seeds(bytes([ABSENT])) == []
    assert len(ix.seeds(pats[-1], max_seeds=32)) == 20  # (a batch of 300 ends with the 20-seed pattern)
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


def test_seeds_pass_through_simt(pkg, O, simt):
    """PassThrough: bytes >= symbol_count in mid-pattern split it into seeds
    on both sides (no FMX_E_SYMBOL, nothing latched)."""
    simt.simt_config(707, 0.5)
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


def test_seeds_async_simt(pkg, O, simt):
    """fmx_seeds_batch_async (on the emulator, device memory is host memory):
    with locations over a garbage workspace and prefilled outputs, ranges only
    with no workspace, a disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the
    "seeds" timer, the argument checks."""
    simt.simt_config(616, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = batch(case, 300)
    ms, n = 3, len(pats)
    exp = expected_arrays(case, orc, pats, ms, 5, 1, 10)
    total = int(exp[4][-1])
    data, offsets = pkg.pack_patterns(pats)
    rnd = np.random.default_rng(4)
    mk = lambda shape, dt=np.uint32: rnd.integers(1, 2**31, shape).astype(dt)  # noqa: E731
    o = [mk(n), mk(n), mk((n, ms, 2)), mk((n, ms, 2)), mk(n * ms + 1, np.uint64), mk(total + 4)]
    tail = o[5][total:].copy()
    need = mk(1, np.uint64)
    wsb = ix.locate_workspace_size(n * ms)
    ws = pkg.aligned_buffer(wsb)
    ws[:] = rnd.integers(0, 256, wsb).astype(np.uint8)
    ptr = [x.ctypes.data for x in o]
    ix.timing_enable(True)
    ix.seeds_batch_async(data.ctypes.data, offsets.ctypes.data, n, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5],
                         total + 4, need.ctypes.data, ws.ctypes.data, wsb, max_seeds=ms, min_len=5, skip=1, max_occ=10)
    ix.sync()
    assert ix.timing_read()["seeds"]["launches"] == 1
    ix.timing_enable(False)
    assert int(need[0]) == total
    compare(o[:5] + [o[5][:total]], exp)
    assert np.array_equal(o[5][total:], tail)
    # ranges only: no workspace, no location arguments
    o2 = [mk(n), mk(n), mk((n, ms, 2)), mk((n, ms, 2))]
    p2 = [x.ctypes.data for x in o2]
    ix.seeds_batch_async(data.ctypes.data, offsets.ctypes.data, n, *p2, max_seeds=ms, min_len=5, skip=1)
    ix.sync()
    compare(o2, exp, locate=False)
    # argument checks
    for kw in (dict(max_seeds=0), dict(max_seeds=33)):
        with pytest.raises(pkg.FmxError) as e:
            ix.seeds_batch_async(data.ctypes.data, offsets.ctypes.data, n, *p2, **kw)
        assert e.value.code == pkg._native.FMX_E_ARG
    with pytest.raises(pkg.FmxError) as e:
        ix.seeds_batch_async(data.ctypes.data, offsets.ctypes.data, n, 0, *p2[1:], max_seeds=ms)
    assert e.value.code == pkg._native.FMX_E_ARG
    # a fixed-length hint the offsets disagree with
    ix.seeds_batch_async(data.ctypes.data, offsets.ctypes.data, n, *p2, max_seeds=ms, fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
