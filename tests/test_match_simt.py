"""Longest-suffix match (fmx_match_batch: k_match, then the locate's k_emit)
on the CPU: the engine's own sources under the SIMT shim (tests/simt, as
tests/test_simt.py), every answer against the values of _match_cases.py —
lengths from the oracle's counts of growing suffixes, intervals from a plainly
sorted suffix list, locations from the oracle's locate of the matched suffix.
A subset of the layouts the GPU file sweeps, every case class: full matches
of m = 1, 2, k-1, k, k+1, 7, 40; one substitution inside the last k symbols
(seed fallback), at m-k-1 (first LF step fails) and further left; an absent
last byte (L = 0); an empty pattern in mid-batch; matches that reach the text
start; unique substrings behind a wrong symbol (sampled-row rollback); a
two-letter text (hundreds of rows per match); capacity; min_len / max_occ;
ranges only; PassThrough bytes >= symbol_count; the device call."""
import ctypes as C

import numpy as np
import pytest

from _match_cases import ABSENT, BATCH_SIZES, Case, check_match
from _simt import simt_fixture


simt = simt_fixture(launch_order=True)


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
    key = (planes, two_letters, tuple(sorted(kw.items())))
    if key not in _CASES:
        nchars = 2 if two_letters else min((1 << planes) - 1, 20)
        _CASES[key] = Case(planes * 11 + (5 if two_letters else 0), nchars, **kw)
    return _CASES[key]


# (P bytes, planes, vector bits): u32 and u64 positions, every vector width, symbol-mask, paired and
# plain records among them
LAYOUTS = [(4, 3, 64), (8, 2, 32), (4, 5, 128), (8, 4, 64)]


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", LAYOUTS)
def test_match_simt(pkg, O, simt, pb, planes, vb, n):
    simt.simt_config(pb * 131 + planes * 17 + vb + n, 0.5)
    case = case_for(planes)
    pats = case.batch(n)
    for occ in (0, 1):
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        exp = check_match(pkg, ix, orc, case, pats)
        if occ == 1 or n < 256:
            check_match(pkg, ix, orc, case, pats, reversed=True)
        if n >= 256:
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


@pytest.mark.parametrize("sr", [1, 2, 3])
def test_match_two_letters_simt(pkg, O, simt, sr):
    """A two-letter text: short matched suffixes have hundreds of rows (the
    row dealing of k_emit), and every sampling ratio's walk."""
    simt.simt_config(900 + sr, 0.5)
    case = case_for(2, two_letters=True, k=3, sr=sr)
    ix, orc = open_index(pkg, O, case, 4, 2, 64, 1)
    pats = case.batch(257)
    exp = check_match(pkg, ix, orc, case, pats)
    assert max(e[2] - e[1] for e in exp) >= 300
    check_match(pkg, ix, orc, case, pats, reversed=True, max_occ=400)
    ix.close()


@pytest.mark.parametrize("min_len", [1, 5])
@pytest.mark.parametrize("max_occ", [0, 1, 10, None])
def test_match_filters_simt(pkg, O, simt, min_len, max_occ):
    """min_len / max_occ: lengths and ranges unchanged, locations only for the
    reporting patterns."""
    simt.simt_config(77 + min_len, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    check_match(pkg, ix, orc, case, case.batch(257), min_len=min_len, max_occ=max_occ)
    ix.close()


def test_match_ranges_only_and_capacity_simt(pkg, O, simt):
    simt.simt_config(4242, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = case.batch(300)
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
    # argument checks: no outputs, locations without a buffer
    assert lib.fmx_match_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, 0, None, rng.ctypes.data,
                               None, None, 0, None) == pkg._native.FMX_E_ARG
    assert lib.fmx_match_batch(ix.handle, data.ctypes.data, offsets.ctypes.data, n, 0, 1, 0, lens.ctypes.data,
                               rng.ctypes.data, loff.ctypes.data, None, 5, None) == pkg._native.FMX_E_ARG
    ix.close()


def test_match_pass_through_simt(pkg, O, simt):
    """PassThrough: a byte >= symbol_count ends the match before it (no
    FMX_E_SYMBOL), in the seed's symbols and beyond them."""
    simt.simt_config(606, 0.5)
    rng = np.random.default_rng(12)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    pats, want = [], []
    for j, m in enumerate([1, 2, 3, 4, 9, 30] * 8):
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


def test_match_async_simt(pkg, O, simt):
    """fmx_match_batch_async (on the emulator, device memory is host memory):
    with locations over a garbage workspace, ranges only with no workspace,
    a disagreeing FMX_HINT_FIXED_LEN still FMX_E_ARG, the "match" timer."""
    simt.simt_config(515, 0.5)
    case = case_for(3, k=3, sr=2)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    pats = [p for p in case.batch(300)]
    exp = [case.expected(orc, p) for p in pats]
    data, offsets = pkg.pack_patterns(pats)
    data = np.concatenate([data, np.zeros(16, np.uint8)])
    n = len(pats)
    rnd = np.random.default_rng(3)
    total = sum(e[2] - e[1] for e in exp if e[0] >= 5 and e[2] - e[1] <= 10)
    lens, rng = rnd.integers(0, 2**31, n).astype(np.uint32), rnd.integers(0, 2**31, (n, 2)).astype(np.uint32)
    loff, locs = rnd.integers(0, 2**62, n + 1).astype(np.uint64), np.zeros(total + 4, np.uint32)
    need = np.zeros(1, np.uint64)
    wsb = ix.locate_workspace_size(n)
    ws = pkg.aligned_buffer(wsb)
    ws[:] = rnd.integers(0, 256, wsb).astype(np.uint8)
    ix.timing_enable(True)
    ix.match_batch_async(data.ctypes.data, offsets.ctypes.data, n, lens.ctypes.data, rng.ctypes.data,
                         loff.ctypes.data, locs.ctypes.data, locs.size, need.ctypes.data, ws.ctypes.data, wsb,
                         min_len=5, max_occ=10)
    ix.sync()
    assert ix.timing_read()["match"]["launches"] == 1
    ix.timing_enable(False)
    assert lens.tolist() == [e[0] for e in exp]
    assert rng.tolist() == [[e[1], e[2]] for e in exp]
    rep = [e[0] >= 5 and e[2] - e[1] <= 10 for e in exp]
    assert int(need[0]) == total and np.diff(loff).tolist() == [e[2] - e[1] if r else 0 for e, r in zip(exp, rep)]
    assert locs[:total].tolist() == [x for e, r in zip(exp, rep) if r for x in e[3]]
    # ranges only: no workspace, no location arguments
    lens2, rng2 = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32)
    ix.match_batch_async(data.ctypes.data, offsets.ctypes.data, n, lens2.ctypes.data, rng2.ctypes.data)
    ix.sync()
    assert np.array_equal(lens2, lens) and np.array_equal(rng2, rng)
    # a fixed-length hint the offsets disagree with
    ix.match_batch_async(data.ctypes.data, offsets.ctypes.data, n, lens2.ctypes.data, rng2.ctypes.data, fixed_len=7)
    with pytest.raises(pkg.FmxError) as e:
        ix.sync()
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()
