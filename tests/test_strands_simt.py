"""Both strands (FMX_PATTERN_REVCOMP / FMX_BOTH_STRANDS on match, seeds and
approx) on the CPU: the engine's own sources under the SIMT shim (tests/simt),
every answer against the existing references run on the expanded batch that
_strand_cases.py builds in Python, and against the engine's own flag-less call
on it.  FMX_BOTH_STRANDS with 1, 127, 128, 129 and 300 reads (the 128-read tile
edge, a slot tile straddling it at 3 slots per pattern), FMX_PATTERN_REVCOMP
with 1, 255, 256 and 257, each with and without FMX_PATTERN_REVERSED, with
locations and ranges only, ragged and fixed-length reads, the raw path (a 1 KB
stage) from a device call with d_bytes at an odd address, max_mm 1 everywhere
and 2 with FMX_APPROX_BEST, a capacity overflow, a map that is no involution,
PassThrough with an out-of-range byte in the map's image, the two-letter text,
every FMX_E_ARG case and the map's round trip."""
import ctypes as C

import numpy as np
import pytest

import _strand_cases as S
from _guard_cases import HostMem
from _seed_cases import case_for, open_index
from _simt import simt_fixture

simt = simt_fixture(launch_order=True)

# (reversed, locate) per load option: each direction with locations and ranges only across the two
PASSES = {0: ((False, True), (True, False)), 1: ((True, True), (False, False))}


def sweep(pkg, O, query, pb, planes, vb, strands, n, cmap_of=S.involution, two_letters=False, **over):
    case = case_for(planes, two_letters=two_letters, **({"k": 3, "sr": 2} if two_letters else {}))
    cmap = cmap_of(case)
    reads = S.reads_for(case, cmap, n)
    for occ in (0, 1):
        ix, orc = open_index(pkg, O, case, pb, planes, vb, occ)
        ix.set_complement(cmap)
        for rev, loc in PASSES[occ]:
            S.check(ix, orc, case, query, reads, cmap, strands, reversed=rev, locate=loc, **over)
        ix.close()


@pytest.mark.parametrize("n", S.BOTH_SIZES)
@pytest.mark.parametrize("pb,planes,vb", S.LAYOUTS)
@pytest.mark.parametrize("query", S.QUERIES)
def test_both_strands_simt(pkg, O, simt, query, pb, planes, vb, n):
    simt.simt_config(pb * 131 + planes * 17 + vb + n, 0.5)
    sweep(pkg, O, query, pb, planes, vb, "both", n)


@pytest.mark.parametrize("n", S.RC_SIZES)
@pytest.mark.parametrize("pb,planes,vb", S.LAYOUTS)
@pytest.mark.parametrize("query", S.QUERIES)
def test_revcomp_simt(pkg, O, simt, query, pb, planes, vb, n):
    simt.simt_config(pb * 137 + planes * 19 + vb + n, 0.5)
    sweep(pkg, O, query, pb, planes, vb, "reverse", n)


@pytest.mark.parametrize("query", S.QUERIES)
def test_not_an_involution_simt(pkg, O, simt, query):
    """a -> b -> c -> a: rc(rc(p)) != p, so a map applied twice or not at all shows."""
    simt.simt_config(311, 0.5)
    sweep(pkg, O, query, 4, 3, 64, "both", 129, cmap_of=S.cycle_map)
    sweep(pkg, O, query, 4, 3, 64, "reverse", 257, cmap_of=S.cycle_map)


@pytest.mark.parametrize("query", S.QUERIES)
def test_two_letters_simt(pkg, O, simt, query):
    """Hundreds of rows per slot (k_emit's row dealing over the 2n-shaped slots)."""
    simt.simt_config(313, 0.5)
    sweep(pkg, O, query, 4, 2, 64, "both", 129, two_letters=True)


def test_approx_two_mismatches_best_simt(pkg, O, simt):
    simt.simt_config(317, 0.5)
    sweep(pkg, O, "approx", 4, 3, 64, "both", 129, max_mm=2, best=True)


@pytest.mark.parametrize("strands,n", [("both", 129), ("both", 300), ("reverse", 257)])
@pytest.mark.parametrize("query", S.QUERIES)
def test_fixed_length_simt(pkg, O, simt, query, strands, n):
    """Fixed-length reads: the host call sets FMX_HINT_FIXED_LEN itself; the
    device call is given it, and a hint the reads' offsets disagree with is
    still FMX_E_ARG."""
    simt.simt_config(331 + n, 0.5)
    case = case_for(3)
    cmap = S.involution(case)
    reads = S.reads_for(case, cmap, n, fixed=True)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    ix.set_complement(cmap)
    S.check(ix, orc, case, query, reads, cmap, strands)
    S.check(ix, orc, case, query, reads, cmap, strands, reversed=True, locate=False)
    for rev in (False, True):
        S.run_device(pkg, ix, HostMem, case, orc, 4, query, reads, cmap, strands, reversed=rev, fixed_len=S.FIXED_M)
    with pytest.raises(pkg.FmxError) as e:
        S.run_device(pkg, ix, HostMem, case, orc, 4, query, reads, cmap, strands, fixed_len=S.FIXED_M - 1)
    assert e.value.code == pkg._native.FMX_E_ARG
    ix.close()


@pytest.mark.parametrize("strands,n", [("both", 300), ("both", 129), ("reverse", 257)])
@pytest.mark.parametrize("query", S.QUERIES)
def test_raw_path_simt(pkg, O, simt, query, strands, n):
    """A 1 KB stage: no full tile fits, the strands are views of the bytes in
    HBM (rev toggled, enc_rc); d_bytes at an odd address, both directions."""
    simt.simt_config(349 + n, 0.5)
    for pb, planes, vb in ((4, 3, 64), (8, 4, 64)):
        case = case_for(planes)
        cmap = S.involution(case)
        reads = S.reads_for(case, cmap, n)
        ix, orc = open_index(pkg, O, case, pb, planes, vb, 1)
        ix.set_complement(cmap)
        for rev in (False, True):
            S.run_device(pkg, ix, HostMem, case, orc, pb, query, reads, cmap, strands, reversed=rev, skew=1,
                         stage_kb=1)
            S.run_device(pkg, ix, HostMem, case, orc, pb, query, reads, cmap, strands, reversed=rev, skew=7,
                         locate=False)
        ix.close()


@pytest.mark.parametrize("query", S.QUERIES)
def test_capacity_simt(pkg, O, simt, query):
    """cap below the total: *d_needed exact, nothing written past cap; the
    host call: FMX_E_CAPACITY with needed exact."""
    simt.simt_config(353, 0.5)
    case = case_for(3)
    cmap = S.involution(case)
    reads = S.reads_for(case, cmap, 129)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    ix.set_complement(cmap)
    for cap in ("total-1", "zero-null"):
        S.run_device(pkg, ix, HostMem, case, orc, 4, query, reads, cmap, "both", cap_name=cap)
    if query != "match":  # (fmx_match_batch grows its device buffer; the other two have the caller's cap)
        kw = S.kw_for(query)
        exp = S.expected(query, case, orc, S.expand(reads, cmap, "both"), kw)
        total = int(exp[-2][-1])
        data, offsets = pkg.pack_patterns(reads)
        nv, slots = 2 * len(reads), 2 * len(reads) * S.PER
        outs = [np.zeros(nv, np.uint32), np.zeros(nv, np.uint32)]
        outs += [np.zeros(2 * slots, np.uint32)] if query == "seeds" else [np.zeros(slots, np.uint32),
                                                                          np.zeros(6 * slots, np.uint32)]
        outs.append(np.zeros(2 * slots, np.uint32))
        loff, locs, needed = np.zeros(slots + 1, np.uint64), np.full(total, 0xFFFFFFFF, np.uint32), C.c_uint64()
        params = (S.PER, 1, 0) if query == "seeds" else (1, S.PER, 0)
        st = getattr(pkg._native.lib(), f"fmx_{query}_batch")(
            ix.handle, data.ctypes.data, offsets.ctypes.data, len(reads), pkg._native.FMX_BOTH_STRANDS, *params,
            (1 << 64) - 1, *[o.ctypes.data for o in outs], loff.ctypes.data, locs.ctypes.data, total - 1,
            C.byref(needed))
        assert st == pkg._native.FMX_E_CAPACITY and needed.value == total and int(loff[-1]) == total
        assert np.array_equal(outs[0], exp[0]) and locs[total - 1] == 0xFFFFFFFF
    ix.close()


def test_pass_through_simt(pkg, O, simt):
    """PassThrough: enc is the identity, so enc_rc is the map itself, and a byte
    of its image >= symbol_count ends a match as such a byte of a pattern does."""
    simt.simt_config(359, 0.5)
    rng = np.random.default_rng(12)
    sigma, k = 5, 3
    text = bytes(rng.integers(0, 4, size=1500).astype(np.uint8))  # symbols 0..3; 4 never occurs
    blob = O.build(text, sigma, O.layout(4, 3, 64), k, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough, options=1)
    cmap = bytearray(range(256))
    cmap[0], cmap[1], cmap[2], cmap[3] = 3, 2, 1, 200  # 3 -> 200: out of range
    cmap = bytes(cmap)
    ix.set_complement(cmap)
    reads = []
    for j in range(129):
        m = int(rng.integers(1, 31))
        s = int(rng.integers(0, len(text) - m))
        p = text[s:s + m]
        reads.append(p if j % 2 else S.rc(p, bytes([3, 2, 1, 0]) + cmap[4:]))  # (rc of a substring, by the true pairing)
    vpats = S.expand(reads, cmap, "both")
    lens, rg, loff, locs = ix.match_batch(reads, strands="both")
    n200 = 0
    for i, p in enumerate(vpats):
        cut = max((j for j, b in enumerate(p) if b >= sigma), default=-1)  # the valid tail: after the last bad byte
        w = p[cut + 1:]
        n200 += cut >= 0
        L = len(w)
        while L and orc.count(w[len(w) - L:]) == 0:
            L -= 1
        assert lens[i] == L, (i, p)
        Sfx = w[len(w) - L:]
        assert int(rg[i, 1] - rg[i, 0]) == (orc.count(Sfx) if L else 0)
        assert locs[int(loff[i]):int(loff[i + 1])].tolist() == (orc.locate(Sfx) if L else [])
    assert n200 >= 30, "few virtual patterns hold the out-of-range byte"
    for query in S.QUERIES:
        kw = S.kw_for(query)
        for strands in ("both", "reverse"):
            got = S.host_call(ix, query, reads, kw, strands)
            own = S.host_call(ix, query, S.expand(reads, cmap, strands), kw)
            assert all(np.array_equal(g, o) for g, o in zip(got, own)), (query, strands)
    ix.sync()  # nothing latched
    ix.close()


def test_single_pattern_pairs_simt(pkg, O, simt):
    """match / seeds / approx with strands="both": a (forward, reverse) pair."""
    simt.simt_config(367, 0.5)
    case = case_for(3)
    cmap = S.involution(case)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    ix.set_complement(cmap)
    p = S.reads_for(case, cmap, 129)[1]
    q = S.rc(p, cmap)
    assert q in case.text and p not in case.text
    fw, bw = ix.match(p, strands="both")
    assert fw == case.expected(orc, p)[:3] and bw == case.expected(orc, q)[:3] and bw[0] == len(p)
    assert ix.match(p, strands="reverse") == bw and ix.match(p) == fw
    sf, sb = ix.seeds(p, strands="both")
    assert sf == ix.seeds(p) and sb == ix.seeds(q) and sb[0][:2] == (len(p), len(p))
    af, ab = ix.approx(p, strands="both")
    assert af == ix.approx(p) and ab == ix.approx(q) and ab[0][0] == 0
    with pytest.raises(ValueError):
        ix.match(p, strands="sideways")
    ix.close()


def test_complement_round_trip_and_arg_errors_simt(pkg, O, simt):
    simt.simt_config(373, 0.5)
    nat = pkg._native
    case = case_for(3)
    cmap = S.involution(case)
    ix, orc = open_index(pkg, O, case, 4, 3, 64, 1)
    reads = S.reads_for(case, cmap, 129)
    E = nat.FMX_E_ARG

    def code(f, *a, **kw):
        with pytest.raises(pkg.FmxError) as e:
            f(*a, **kw)
        return e.value.code
    # no map: nothing to read back, either flag is an error in all six entry points
    assert ix.complement is None
    buf = np.zeros(1 << 16, np.uint64)
    d = buf.ctypes.data
    for query in S.QUERIES:
        n_out = len(S.OUTS[query])
        for strands in ("reverse", "both"):
            assert code(getattr(ix, query + "_batch"), reads, strands=strands) == E
            assert code(getattr(ix, query + "_batch_async"), d, d, 4, *[d] * n_out, strands=strands) == E
    ix.set_complement(cmap)
    assert ix.complement == cmap
    ix.set_complement(S.cycle_map(case))
    assert ix.complement == S.cycle_map(case)
    ix.set_complement(None)
    assert ix.complement is None and code(ix.match_batch, reads, strands="both") == E
    with pytest.raises(ValueError):
        ix.set_complement(b"AT")
    assert pkg.complement_map([(b"A", b"T"), (b"C", b"G")])[65:72] == b"TBGDEFC"
    ix.set_complement(cmap)
    # both flags together
    lib = nat.lib()
    data, offsets = pkg.pack_patterns(reads)
    n = len(reads)
    both = nat.FMX_PATTERN_REVCOMP | nat.FMX_BOTH_STRANDS
    o = [np.zeros(12 * 2 * n * S.PER, np.uint32) for _ in range(5)]
    op = [x.ctypes.data for x in o]
    hp = (ix.handle, data.ctypes.data, offsets.ctypes.data, n)
    assert lib.fmx_match_batch(*hp, both, 1, 0, op[0], op[1], None, None, 0, None) == E
    assert lib.fmx_match_batch_async(*hp, both, 1, 0, op[0], op[1], None, None, 0, None, None, 0, None) == E
    assert lib.fmx_seeds_batch(*hp, both, 3, 1, 0, 0, *op[:4], None, None, 0, None) == E
    assert lib.fmx_seeds_batch_async(*hp, both, 3, 1, 0, 0, *op[:4], None, None, 0, None, None, 0, None) == E
    assert lib.fmx_approx_batch(*hp, both, 1, 3, 0, 0, *op[:5], None, None, 0, None) == E
    assert lib.fmx_approx_batch_async(*hp, both, 1, 3, 0, 0, *op[:5], None, None, 0, None, None, 0, None) == E
    # count and locate take neither flag
    wsb = ix.locate_workspace_size(n)
    ws = pkg.aligned_buffer(wsb)
    loff, locs, need = np.zeros(n + 1, np.uint64), np.zeros(1 << 14, np.uint32), np.zeros(1, np.uint64)
    for flag in (nat.FMX_PATTERN_REVCOMP, nat.FMX_BOTH_STRANDS):
        assert lib.fmx_count_batch(*hp, flag, op[0]) == E
        assert lib.fmx_count_batch_async(*hp, flag, op[0], None) == E
        assert lib.fmx_locate_batch(*hp, flag, loff.ctypes.data, locs.ctypes.data, locs.size, None) == E
        assert lib.fmx_locate_batch_async(*hp, flag, None, loff.ctypes.data, locs.ctypes.data, locs.size,
                                          need.ctypes.data, ws.ctypes.data, wsb, None) == E
        job = ix.job_queue([ix.locate_job(data.ctypes.data, offsets.ctypes.data, n, loff.ctypes.data, locs.ctypes.data,
                                          locs.size, need.ctypes.data, ws.ctypes.data, wsb)])
        job[0].flags |= flag
        assert lib.fmx_locate_jobs_async(ix.handle, job, 1) == E
        assert lib.fmx_locate_group_async(ix.handle, job, 1, None) == E
    # the flags still work after all that
    S.check(ix, orc, case, "match", reads, cmap, "both")
    ix.close()
