"""Longest-suffix match on the GPU (fmx_match_batch: k_match, then the
locate's k_emit): the cases of tests/test_match_simt.py on the gfx950 kernels,
every layout, load options 0 (blob layout) and 1 (interleaved records), every
derived structure for two layouts (they must not change a result), forward
and reversed, batches of 1, 255, 256, 257 and 700 patterns.  Expected values:
_match_cases.py (the oracle's counts of growing suffixes, a plainly sorted
suffix list, the oracle's locate of the matched suffix)."""
import ctypes as C
import os

import numpy as np
import pytest

from _match_cases import ABSENT, BATCH_SIZES, Case, check_match
from _util import ALL_LAYOUTS

pytestmark = pytest.mark.gpu
# (as tests/test_gpu.py: a 1 MB deep-table budget for the loads with every derived structure)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def pos_of(pkg, pb):
    return pkg.u32 if pb == 4 else pkg.u64


def block_of(pkg, planes, vb):
    return getattr(pkg.blocks, f"Block{planes}")(pkg.Vector(vb))


def open_index(pkg, O, case, pb, planes, vb, occ):
    blob = case.blob(O, pb, planes, vb)
    orc = O.OracleIndex(blob, O.layout(pb, planes, vb, 0))
    return pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=occ), orc


_CASES = {}


def case_for(planes, two_letters=False, **kw):
    """One text per alphabet size (its expected values are computed once)."""
    key = (planes, two_letters, tuple(sorted(kw.items())))
    if key not in _CASES:
        nchars = 2 if two_letters else min((1 << planes) - 1, 20)
        _CASES[key] = Case(planes * 11 + (5 if two_letters else 0), nchars, **kw)
    return _CASES[key]


def sweep(pkg, O, case, pb, planes, vb, options):
    for occ in options:
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        for n in BATCH_SIZES:
            pats = case.batch(n)
            exp = check_match(pkg, ix, orc, case, pats)
            check_match(pkg, ix, orc, case, pats, reversed=True)
            if n < 256:
                continue
            L = np.array([e[0] for e in exp])
            m = np.array([len(p) for p in pats])
            assert (L == 0).sum() >= 4 and (L == m).sum() >= 20 and (L == case.k).sum() >= 1 \
                and (L > case.k).sum() >= 20 and (case.k == 1 or ((L > 0) & (L < case.k)).sum() >= 1), \
                "case classes missing from the batch"
            # a fully matching pattern: exactly what locate_batch returns for it
            full = [p for p, e in zip(pats, exp) if e[0] == len(p) and len(p)]
            _, rng, loff, locs = ix.match_batch(full)
            woff, wlocs = ix.locate_batch(full)
            assert np.array_equal(loff, woff) and np.array_equal(locs, wlocs)
            assert np.array_equal((rng[:, 1] - rng[:, 0]).astype(np.uint64), np.diff(woff))
        ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_match_every_layout(pkg, O, pb, planes, vb):
    sweep(pkg, O, case_for(planes), pb, planes, vb, (0, 1))


@pytest.mark.parametrize("pb,planes,vb", [(4, 3, 64), (8, 5, 128)])
def test_match_ignores_derived_structures(pkg, O, pb, planes, vb):
    """FMX_OPT_DERIVED (deep table, full SA, text, row contexts, single-row
    entries): the match reads none of them (a loaded full SA serves the
    locations), and the answers are the same."""
    sweep(pkg, O, case_for(planes), pb, planes, vb, (63,))


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_match_two_letters(pkg, O, sr):
    """A two-letter text: short matched suffixes have hundreds of rows (the
    row dealing of k_emit), under every sampling ratio's walk."""
    case = case_for(2, two_letters=True, k=3, sr=sr)
    for pb, vb in ((4, 64), (8, 32)):
        ix, orc = open_index(pkg, O, case, pb, 2, vb, 1)
        pats = case.batch(700)
        exp = check_match(pkg, ix, orc, case, pats)
        assert max(e[2] - e[1] for e in exp) >= 300
        check_match(pkg, ix, orc, case, pats, reversed=True, max_occ=400)
        ix.close()


@pytest.mark.parametrize("min_len", [1, 5])
@pytest.mark.parametrize("max_occ", [0, 1, 10, None])
def test_match_filters(pkg, O, min_len, max_occ):
    """min_len / max_occ: lengths and ranges unchanged, locations only for the
    reporting patterns."""
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    check_match(pkg, ix, orc, case, case.batch(700), min_len=min_len, max_occ=max_occ)
    ix.close()


def test_match_ranges_only_and_capacity(pkg, O):
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = case.batch(700)
    exp = check_match(pkg, ix, orc, case, pats, locate=False)
    assert ix.match(pats[5]) == exp[5][:3]
    assert ix.match(b"") == (0, 0, 0) and ix.match(bytes([ABSENT])) == (0, 0, 0)
    # a cap below needed: FMX_E_CAPACITY, needed exact, lengths / ranges / offsets written all the same
    total = sum(e[2] - e[1] for e in exp if e[0] >= 1)
    data, offsets = pkg.pack_patterns(pats)
    n = len(pats)
    lens, rng = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32)
    loff, locs, needed = np.zeros(n + 1, np.uint64), np.zeros(total, np.uint32), C.c_uint64()
    lib = pkg._native.lib()
    args = lambda cap: (ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, (1 << 64) - 1, lens.ctypes.data,  # noqa
                        rng.ctypes.data, loff.ctypes.data, locs.ctypes.data, cap, C.byref(needed))
    assert lib.fmx_match_batch(*args(total - 1)) == pkg._native.FMX_E_CAPACITY
    assert needed.value == total and int(loff[-1]) == total
    assert lens.tolist() == [e[0] for e in exp] and rng[:, 0].tolist() == [e[1] for e in exp]
    assert lib.fmx_match_batch(*args(total)) == 0 and needed.value == total
    assert locs.tolist() == [x for e in exp for x in e[3]]
    ix.close()


def test_match_pass_through(pkg, O):
    """PassThrough: a byte >= symbol_count ends the match before it (no
    FMX_E_SYMBOL), among the seed's symbols and beyond them."""
    rng = np.random.default_rng(12)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, want = [], []
    for m in [1, 2, 3, 4, 9, 30] * 8:
        s = int(rng.integers(0, len(text) - m))
        p = text[s:s + m]
        for bad in (9, 200):
            for cut in sorted({0, 1, min(2, m), min(k, m), m}):  # valid symbols after the bad byte
                q = p[:m - cut] + bytes([bad]) + p[m - cut:]
                pats.append(q)
                want.append(q[len(q) - cut:])
    lens, rg, loff, locs = ix.match_batch(pats)
    for i, (p, w) in enumerate(zip(pats, want)):
        L = len(w)
        while L and orc.count(w[len(w) - L:]) == 0:  # (the valid tail itself may not occur whole)
            L -= 1
        assert lens[i] == L, (i, p, w)
        S = w[len(w) - L:]
        assert int(rg[i, 1] - rg[i, 0]) == (orc.count(S) if L else 0)
        assert locs[int(loff[i]):int(loff[i + 1])].tolist() == (orc.locate(S) if L else [])
    ix.sync()  # nothing latched
    ix.close()


def test_match_async(pkg, O):
    """fmx_match_batch_async on HBM-resident buffers: with locations, ranges
    only with no workspace, a disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG,
    the "match" timer."""
    import torch
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = case.batch(700)
    exp = [case.expected(orc, p) for p in pats]
    data, offsets = pkg.pack_patterns(pats)
    n = len(pats)
    dev = torch.device("cuda:0")
    rep = [e[0] >= 5 and e[2] - e[1] <= 10 for e in exp]
    total = sum(e[2] - e[1] for e, r in zip(exp, rep) if r)
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    d_lens = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_rng = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
    d_loff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_locs = torch.zeros(total + 4, dtype=torch.int32, device=dev)
    d_need = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = ix.locate_workspace_size(n)
    d_ws = torch.randint(0, 256, (wsb,), dtype=torch.uint8, device=dev)  # (a workspace needs no initialisation)
    torch.cuda.synchronize()  # (buffers made on torch's stream; the index launches on its own)
    ix.timing_enable(True)
    ix.match_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, d_lens.data_ptr(), d_rng.data_ptr(),
                         d_loff.data_ptr(), d_locs.data_ptr(), total + 4, d_need.data_ptr(), d_ws.data_ptr(), wsb,
                         min_len=5, max_occ=10)
    ix.sync()
    assert ix.timing_read()["match"]["launches"] == 1
    ix.timing_enable(False)
    assert d_lens.cpu().tolist() == [e[0] for e in exp]
    assert d_rng.cpu().tolist() == [[e[1], e[2]] for e in exp]
    assert int(d_need.item()) == total
    assert np.diff(d_loff.cpu().numpy()).tolist() == [e[2] - e[1] if r else 0 for e, r in zip(exp, rep)]
    assert d_locs.cpu()[:total].tolist() == [x for e, r in zip(exp, rep) if r for x in e[3]]
    d_lens2, d_rng2 = torch.zeros_like(d_lens), torch.zeros_like(d_rng)
    torch.cuda.synchronize()
    ix.match_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, d_lens2.data_ptr(), d_rng2.data_ptr())
    ix.sync()
    assert torch.equal(d_lens2, d_lens) and torch.equal(d_rng2, d_rng)
    ix.match_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, d_lens2.data_ptr(), d_rng2.data_ptr(), fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
