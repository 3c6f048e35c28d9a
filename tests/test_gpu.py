"""GPU parity tests: every result of the gfx950 kernels is compared bit for bit
with the oracle (oracle/fmx_oracle.c) on the same inputs — counts, and
locations element-wise in suffix-array-row order — through the C ABI.
The GPU blob builder is compared byte for byte with the oracle's builder."""
import json
import os

import numpy as np
import pytest

from _build_cases import check_parity, every_layout_inputs  # (shared with the emulator's builder tests)
from _build_cases import engine_build as gpu_build
from _util import (ALL_LAYOUTS, encode, occurrences, rand_chr_list, rand_pattern, rand_text,
                   table_from_symbols)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# load options (FMX_OCC_INTERLEAVED=1 | FMX_OPT_DEEP_LUT=2 | FMX_OPT_FULL_SA=4 |
# FMX_OPT_TEXT=8 | FMX_OPT_ROW_CONTEXT=16 | FMX_OPT_LUT_ROWS=32): the blob as
# laid out, the default interleaved records (both faithful: SURVEY §8), and
# one set with every derived structure (opt-in, outside §8; each derived
# structure alone is covered on the CPU by tests/test_emu.py); a 1 MB table
# budget makes K > k even on the small test texts (K = 8 for sigma = 4)
OCC_MODES = (0, 1, 63)
os.environ.setdefault("FMX_DEEP_LUT_MB", "1")


def block_of(pkg, planes, vb):
    return getattr(pkg.blocks, f"Block{planes}")(pkg.Vector(vb))


def pos_of(pkg, pb):
    return pkg.u32 if pb == 4 else pkg.u64


def test_readme_known_answers_gpu(pkg, O):
    g = json.load(open(os.path.join(HERE, "golden", "readme.json")))
    table = pkg.text_encoders.EncodingTable.from_symbols([s.encode() for s in g["symbols"]])
    b = pkg.FmIndexBuilder(len(g["text"]), table.symbol_count(), table, pkg.u32, pkg.blocks.Block2(pkg.Vector.U64))
    blob = pkg.aligned_buffer(b.blob_size())
    b.build(g["text"].encode(), blob)
    for occ in OCC_MODES:
        fm = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block2(pkg.Vector.U64), pkg.text_encoders.EncodingTable,
                              options=occ)
        for case in g["cases"]:
            p = case["pattern"].encode()
            if "count" in case:
                assert fm.count(p) == case["count"]
            assert sorted(fm.locate(p)) == case["sorted_locations"]
        buf = [7]
        fm.locate_to_buffer(b"TA", buf)  # appends (locate/mod.rs:28,35)
        assert buf[0] == 7 and sorted(buf[1:]) == [5, 18]
        assert fm.count_rev_iter(iter(b"AT")) == 2
        fm.close()


def test_golden_blobs_on_gpu(pkg, O):
    """The committed golden blobs: GPU builder reproduces them, kernels answer them."""
    g = json.load(open(os.path.join(HERE, "golden", "oracle_cases.json")))
    for c in g["cases"]:
        pb, planes, vb = c["layout"]
        text, table = bytes.fromhex(c["text"]), bytes.fromhex(c["table"])
        blob = gpu_build(pkg, text, c["sigma"], pb, planes, vb, c["kmer_size"], c["sampling_ratio"], table)
        assert bytes(blob).hex() == c["blob"]
        for occ in OCC_MODES:
            ix = pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=occ)
            for q in c["queries"]:
                p = bytes.fromhex(q["pattern"])
                assert ix.count(p) == q["count"]
                assert ix.locate(p) == q["locations"]
            ix.close()


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_builder_and_queries_every_layout(pkg, O, pb, planes, vb):
    """get_accurate_result-style sweep on the GPU: builder bytes, then count and
    locate against the oracle for both device occ layouts."""
    for sigma, chars, table, text, k, sr, pats in every_layout_inputs(pb, planes, vb):
        blob = gpu_build(pkg, text, sigma, pb, planes, vb, k, sr, table)
        ref = O.build(text, sigma, O.layout(pb, planes, vb), k, sr, table)
        assert np.array_equal(blob, ref), f"builder differs sigma={sigma} k={k} sr={sr}"
        for occ in OCC_MODES:
            check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)


def expected_occ_record(pb, planes, vb, sigma, paired=True, onehot=True, walk=False):
    """The loader's record encoding (fmx_device.hpp interleaved_rec_bytes)."""
    b = planes * vb // 8
    pba = -(-b // pb) * pb
    need = pba + sigma * pb
    plain = 64 if need <= 64 else 128 if need <= 128 else 0
    u = vb // 8 + pb
    hot = 64 if sigma * u <= 64 else 128 if sigma * u <= 128 else 0
    if onehot and hot and u % 4 == 0 and (plain == 0 or hot <= plain):
        return hot | 2
    if onehot and walk and not hot and u % 4 == 0 and pba + sigma * pb <= 128:   # + a walk line
        for lines in (2, 3, 4):
            if sigma <= (lines - 1) * (128 // u):
                return 128 * lines | 2 | 4
    if onehot and not hot and u % 4 == 0 and u <= 128 - b:   # multi-line symbol masks
        for lines in (2, 3, 4):
            if sigma <= (lines - 1) * (128 // u) + (128 - b) // u:
                return 128 * lines | 2
    pt = b % 16
    pta = -(-pt // pb) * pb
    if paired and plain and pt and 16 - pta >= pb:
        per = (16 - pta) // pb
        if 16 * (b // 16 + -(-sigma // per)) <= plain:
            return plain | 1
    return plain


@pytest.mark.parametrize("pb,planes,vb", ALL_LAYOUTS)
def test_record_encodings(pkg, O, pb, planes, vb, monkeypatch):
    """Interleaved occ records — symbol-mask (one unit per symbol: its mask
    over the block + checkpoint; multi-line ones with or without a walk line,
    FMX_OCC_WALK), paired-chunk (every rank reads planes + one
    checkpoint chunk that repeats the planes' tail) and plain
    (FMX_OCC_ONEHOT=0, FMX_OCC_PAIRED=0): the loader picks the expected
    encoding and each answers like the oracle, on random texts and on texts
    with long single-symbol runs."""
    rng = np.random.default_rng(pb * 7 + planes * 5 + vb)
    for sigma in sorted({2, 3, min(5, 1 << planes), 1 << planes}):
        chars = rand_chr_list(rng, sigma)
        table = table_from_symbols([bytes([c]) for c in chars])
        for text in (rand_text(rng, chars, 500, 3000),
                     chars + chars[:1] * 700 + chars * 3 + chars[-1:] * 300 + chars[1:2] * 257):
            blob = gpu_build(pkg, text, sigma, pb, planes, vb, 3 if sigma < 8 else 2, 2, table)
            pats = [rand_pattern(rng, text, 1, 24) for _ in range(300)] + [chars[:1] * 3, chars[-1:] * 5]
            for onehot, paired, walk in ((True, True, False), (True, True, True), (False, True, False),
                                         (False, False, False)):
                monkeypatch.setenv("FMX_OCC_ONEHOT", "1" if onehot else "0")
                monkeypatch.setenv("FMX_OCC_PAIRED", "1" if paired else "0")
                monkeypatch.setenv("FMX_OCC_WALK", "1" if walk else "0")
                ix = pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=1)
                want = expected_occ_record(pb, planes, vb, sigma, paired, onehot, walk)
                assert ix.info()["occ_record"] == want, (sigma, onehot, paired, walk)
                ix.close()
                check_parity(pkg, O, blob, pb, planes, vb, 0, pats, 1)
                check_parity(pkg, O, blob, pb, planes, vb, 0, pats, 1 | 2 | 4)


def test_record_fallback_when_hbm_is_short(pkg, O, monkeypatch):
    """fmx_load falls back from multi-line symbol masks with a walk line to
    those without, to the one-line encodings, then to the blob layout, when
    the records do not fit in HBM (FMX_OCC_MAX_MB stands in for a full
    device); answers are unchanged."""
    rng = np.random.default_rng(21)
    chars = rand_chr_list(rng, 21)
    table = table_from_symbols([bytes([c]) for c in chars])
    text = rand_text(rng, chars, 300_000, 300_000)
    blob = gpu_build(pkg, text, 21, 4, 5, 64, 3, 2, table)
    pats = [rand_pattern(rng, text, 1, 14) for _ in range(500)]
    blocks = len(text) // 64 + 1
    for cap_mb, want in ((None, 512 | 2 | 4), ((blocks * 384 >> 20) + 1, 384 | 2), ((blocks * 128 >> 20) + 1, 128),
                         (0, 0)):
        if cap_mb is None:
            monkeypatch.delenv("FMX_OCC_MAX_MB", raising=False)
        else:
            monkeypatch.setenv("FMX_OCC_MAX_MB", str(cap_mb))
        ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block5(pkg.Vector.U64), options=1)
        assert ix.info()["occ_record"] == want, (cap_mb, ix.info()["occ_record"])
        ix.close()
        check_parity(pkg, O, blob, 4, 5, 64, 0, pats, 1, reversed_too=False)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 127, 128, 129, 4096])
def test_block_boundaries(pkg, O, n):
    """n % BLOCK_LEN == 0 appends a zero block + checkpoint row (bwm/mod.rs:136-142)."""
    rng = np.random.default_rng(n)
    table = table_from_symbols([b"A", b"C", b"G", b"T"])
    text = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=n)) if n else b""
    for pb, planes, vb in [(4, 2, 32), (8, 2, 64), (4, 3, 128), (8, 6, 128)]:
        for k, sr in [(1, 1), (3, 2), (4, 3)]:
            blob = gpu_build(pkg, text, 4, pb, planes, vb, k, sr, table)
            assert np.array_equal(blob, O.build(text, 4, O.layout(pb, planes, vb), k, sr, table))
            pats = [b"A", b"AC", b"ACG", b"ACGT", b"T", b"NN", b"GATTACA"] + \
                   ([text[i:i + 5] for i in range(0, max(n - 5, 0), 7)] if n > 5 else [])
            for occ in OCC_MODES:
                check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)


def test_pass_through(pkg, O):
    """PassThrough encoder (pass_through.rs): text and patterns are indices."""
    rng = np.random.default_rng(11)
    for sigma, planes in [(2, 2), (3, 2), (7, 3), (30, 5)]:
        text = bytes(rng.integers(0, sigma, size=3000).astype(np.uint8))
        blob = gpu_build(pkg, text, sigma, 4, planes, 64, 3, 2, None)
        assert np.array_equal(blob, O.build(text, sigma, O.layout(4, planes, 64), 3, 2, None))
        pats = [rand_pattern(rng, text, 1, 15) for _ in range(200)]
        for occ in OCC_MODES:
            check_parity(pkg, O, blob, 4, planes, 64, 1, pats, occ)


def test_high_count_patterns(pkg, O):
    """Skewed occurrence counts: one pattern with ~all rows, many with few —
    exercises the wave-level row balancing of k_locate."""
    text = (b"AC" * 20000) + b"GT" * 50 + (b"A" * 5000)
    table = table_from_symbols([b"A", b"C", b"G", b"T"])
    for pb, planes, vb in [(4, 2, 64), (8, 3, 128)]:
        blob = gpu_build(pkg, text, 4, pb, planes, vb, 3, 3, table)
        pats = [b"A", b"AC", b"CA", b"ACA", b"G", b"GT", b"TA", b"AAAA"] * 20 + [b"C"]
        for occ in OCC_MODES:
            ooff, _ = check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)
        t_idx = encode(table, text)
        assert int(ooff[1] - ooff[0]) == len(occurrences(t_idx, b"\x00"))


def test_repetitive_text_builder(pkg, O):
    """Worst case for prefix doubling: long runs need many doubling rounds."""
    rng = np.random.default_rng(3)
    table = table_from_symbols([b"A", b"C", b"G", b"T"])
    text = b"A" * 30000 + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=500)) + b"ACGT" * 5000
    blob = gpu_build(pkg, text, 4, 4, 2, 64, 3, 2, table)
    assert np.array_equal(blob, O.build(text, 4, O.layout(4, 2, 64), 3, 2, table))
    for occ in OCC_MODES:
        check_parity(pkg, O, blob, 4, 2, 64, 0, [b"A" * 17, b"ACGTA", b"AAAC", b"TA", b"A" * 40], occ)


def test_c1_config(pkg, O):
    """BASELINE configs[0]: 1 Mbp ACGT (T wildcard), u32/Block2<u64>, sr 2,
    k 3, 1,000 x 20 bp patterns — builder bytes and every result."""
    rng = np.random.default_rng(42)
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=1_000_000).astype(np.uint8)
    table = table_from_symbols([b"Aa", b"Cc", b"Gg", b"Tt"])
    blob = gpu_build(pkg, text.tobytes(), 4, 4, 2, 64, 3, 2, table)
    assert blob.size == 2_500_920
    ref = O.build(text.tobytes(), 4, O.layout(4, 2, 64), 3, 2, table)
    assert np.array_equal(blob, ref)
    starts = rng.integers(0, text.size - 20, size=1000)
    pats = [text[s:s + 20].tobytes() for s in starts]
    for occ in OCC_MODES:
        ooff, olocs = check_parity(pkg, O, blob, 4, 2, 64, 0, pats, occ, reversed_too=False)
    # every pattern was cut from the text: its start must be among its locations
    for i, s in enumerate(starts):
        assert int(s) in set(int(x) for x in olocs[ooff[i]:ooff[i + 1]])


def test_errors_gpu(pkg, O):
    table = table_from_symbols([b"A", b"C", b"G", b"T"])
    blob = gpu_build(pkg, b"ACGTACGTAC", 4, 4, 2, 64, 2, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block2(pkg.Vector.U64))
    with pytest.raises(pkg.FmxError) as e:
        ix.count_batch([b"AC", b""])
    assert e.value.code == pkg._native.FMX_E_EMPTY_PATTERN
    assert ix.count(b"AC") == 3  # the index stays usable
    pt_blob = gpu_build(pkg, bytes([0, 1, 2, 3, 0, 1]), 4, 4, 2, 64, 1, 1, None)
    pt = pkg.FmIndex.load(pt_blob, pkg.u32, pkg.blocks.Block2(pkg.Vector.U64), pkg.text_encoders.PassThrough)
    with pytest.raises(pkg.FmxError) as e:
        pt.count(bytes([0, 4]))
    assert e.value.code == pkg._native.FMX_E_SYMBOL
    assert pt.count(bytes([0, 1])) == 2
    with pytest.raises(pkg.FmxError):
        gpu_build(pkg, b"ACGQ", 3, 4, 2, 64, 1, 1, bytes([5] * 256))  # idx 5 >= symbol_count 3


def test_device_async_api(pkg, O):
    """fmx_count_batch_async / fmx_locate_batch_async on HBM-resident buffers
    (torch tensors as plumbing) give the host API's results."""
    import torch
    rng = np.random.default_rng(9)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=200_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    starts = rng.integers(0, text.size - 20, size=5000)
    pats = [text[s:s + 20].tobytes() for s in starts]
    data, offsets = pkg.pack_patterns(pats)
    hoff, hlocs = ix.locate_batch((data, offsets))
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    n = len(pats)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    d_loff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    cap = int(hlocs.size) + 16
    d_locs = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_need = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = ix.locate_workspace_size(n)
    d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (buffers made on torch's stream; the index launches on its own)
    ix.locate_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, d_loff.data_ptr(), d_locs.data_ptr(), cap,
                          d_need.data_ptr(), d_ws.data_ptr(), ws, d_counts=d_cnt.data_ptr())
    ix.sync()
    assert int(d_need.item()) == hlocs.size
    assert np.array_equal(d_loff.cpu().numpy().view(np.uint64), hoff)
    assert np.array_equal(d_locs.cpu().numpy()[:hlocs.size].view(np.uint32), hlocs)
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), np.diff(hoff).astype(np.uint32))
    d_cnt2 = torch.zeros(n, dtype=torch.int32, device=dev)
    ix.count_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, d_cnt2.data_ptr())
    ix.sync()
    assert torch.equal(d_cnt, d_cnt2)
    ix.timing_enable(True)
    ix.locate_batch_async(d_data.data_ptr(), d_off.data_ptr(), n, d_loff.data_ptr(), d_locs.data_ptr(), cap,
                          d_need.data_ptr(), d_ws.data_ptr(), ws)
    ix.sync()
    t = ix.timing_read()
    assert t["locate"]["launches"] == 1 and t["locate"]["total_ms"] > 0 and t["locate"]["units"] == n
    ix.close()


def test_load_device_blob(pkg, O):
    """fmx_build_device + fmx_load_device: the blob never leaves HBM."""
    import torch
    rng = np.random.default_rng(5)
    table = pkg.text_encoders.EncodingTable.from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=100_000).astype(np.uint8)
    b = (pkg.FmIndexBuilder(text.size, 5, table, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
         .set_lookup_table_config(pkg.build_config.LookupTableConfig.KmerSize(3))
         .set_suffix_array_config(pkg.build_config.SuffixArrayConfig.Compressed(2)))
    size = b.blob_size()
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(text).to(dev)
    d_blob = torch.zeros(size, dtype=torch.uint8, device=dev)
    b.build_device(d_text.data_ptr(), d_blob.data_ptr(), size)
    host = d_blob.cpu().numpy()
    ref = O.build(text.tobytes(), 5, O.layout(4, 3, 64), 3, 2, table.table)
    assert np.array_equal(host, ref)
    ix = pkg.FmIndex.load_device(d_blob.data_ptr(), size, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    pats = [text[s:s + 12].tobytes() for s in rng.integers(0, text.size - 12, size=500)]
    orc = O.OracleIndex(ref, O.layout(4, 3, 64, 0))
    data, offsets = pkg.pack_patterns(pats)
    ooff, olocs = orc.locate_batch(data, offsets)
    goff, glocs = ix.locate_batch((data, offsets))
    assert np.array_equal(goff, ooff) and np.array_equal(glocs, olocs)
    ix.close()


def test_deep_lut_info(pkg, O):
    """FMX_OPT_DEEP_LUT is in effect with K > k and answers like the LF path."""
    rng = np.random.default_rng(21)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=50_000, p=[.3, .2, .2, .29, .01]).tobytes()
    blob = gpu_build(pkg, text, 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    assert ix.info()["options"] == pkg._native.FMX_OPT_DEFAULT == pkg._native.FMX_OCC_INTERLEAVED
    ix.close()
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), options=pkg._native.FMX_OPT_DERIVED)
    info = ix.info()
    assert info["options"] == pkg._native.FMX_OPT_DERIVED and info["deep_lut_k"] > 3
    K = info["deep_lut_k"]
    pats = [text[s:s + int(rng.integers(1, 3 * K))] for s in rng.integers(0, len(text) - 3 * K, size=3000)]
    pats += [b"NNNNNNNNNNNNNNNN", b"A" * K, b"Z" * (K + 2)]
    ix.close()
    for occ in (1 | 2, 2, 1 | 2 | 4 | 8):
        check_parity(pkg, O, blob, 4, 3, 64, 0, pats, occ)


@pytest.mark.parametrize("scan", ["1", "7", "64"])
def test_row_context_scan_limits(pkg, O, scan, monkeypatch):
    """FMX_OPT_ROW_CONTEXT with every scan limit (1: single rows only, 64: the
    mask width): contexts shorter than the remaining pattern (sigma = 16 packs
    3 symbols per u32 context... 7), repetitive text (intervals of many rows),
    PassThrough bytes >= sigma (the scan must yield to the LF loop)."""
    monkeypatch.setenv("FMX_SCAN_ROWS", scan)
    rng = np.random.default_rng(int(scan))
    for sigma, pb, planes, vb in [(16, 4, 4, 64), (4, 8, 2, 128), (5, 4, 3, 32)]:
        chars = rand_chr_list(rng, sigma)
        table = table_from_symbols([bytes([c]) for c in chars])
        text = (rand_text(rng, chars, 3000, 6000) + chars[:2] * 300
                + rand_text(rng, chars, 1000, 2000))
        blob = gpu_build(pkg, text, sigma, pb, planes, vb, 3, 3, table)
        pats = [rand_pattern(rng, text, 1, 40) for _ in range(1500)] + [chars[:2] * 5, chars[:2] * 40]
        for occ in (16, 31, 63):
            check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)
        ix = pkg.FmIndex.load(blob, pos_of(pkg, pb), block_of(pkg, planes, vb), options=31)
        info = ix.info()
        assert info["scan_rows"] == int(scan) and info["context_len"] > 0
        ix.close()
    # PassThrough: bytes >= sigma anywhere in the pattern
    text = bytes(rng.integers(0, 4, size=5000).astype(np.uint8))
    blob = gpu_build(pkg, text, 4, 4, 2, 64, 2, 2, None)
    pats = [text[s:s + 20] for s in rng.integers(0, 4900, size=300)]
    pats += [bytes([9]) + p[1:] for p in pats[:50]] + [p[:10] + bytes([7]) + p[11:] for p in pats[50:100]]
    orc = O.OracleIndex(blob, O.layout(4, 2, 64, 1))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block2(pkg.Vector.U64), pkg.text_encoders.PassThrough,
                          options=63)
    for p in pats:
        try:
            want = ("ok", orc.locate(p))
        except O.OracleError as e:
            want = ("err", e.code)
        try:
            got = ("ok", [int(x) for x in ix.locate(p)])
        except pkg.FmxError as e:
            got = ("err", e.code)
        assert got == want, (p, got, want)
    ix.close()


def test_absent_symbols_gpu(pkg, O):
    """Alphabet symbols that never occur in the text (the deep table is indexed
    by the occurring ones; C2's N): patterns holding them anywhere, and for
    PassThrough, bytes >= sigma next to them — same status and locations as
    the oracle under every load option."""
    rng = np.random.default_rng(321)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=20000))
    for pb, planes, vb in [(4, 3, 64), (8, 3, 128)]:
        blob = gpu_build(pkg, text, 5, pb, planes, vb, 3, 2, table)
        pats = [text[s:s + int(rng.integers(1, 30))] for s in rng.integers(0, 19950, size=600)]
        for p in list(pats[:200]):
            j = int(rng.integers(0, len(p)))
            pats.append(p[:j] + b"N" + p[j + 1:])
        pats += [b"N", b"NN", b"N" * 20, b"ACGTN" * 4]
        for occ in OCC_MODES:
            check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ)
    text = bytes(rng.integers(0, 4, size=20000).astype(np.uint8))
    blob = gpu_build(pkg, text, 5, 4, 3, 64, 2, 2, None)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 1))
    pats = [text[s:s + 24] for s in rng.integers(0, 19950, size=40)]
    muts = []
    for p in pats:
        a, b = sorted(int(x) for x in rng.integers(0, len(p), size=2))
        if a < b:
            muts.append(p[:a] + bytes([4]) + p[a + 1:b] + bytes([9]) + p[b + 1:])
            muts.append(p[:a] + bytes([9]) + p[a + 1:b] + bytes([4]) + p[b + 1:])
    for occ in OCC_MODES:
        ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64), pkg.text_encoders.PassThrough,
                              options=occ)
        for p in pats + muts:
            try:
                want = ("ok", orc.locate(p))
            except O.OracleError as e:
                want = ("err", e.code)
            try:
                got = ("ok", [int(x) for x in ix.locate(p)])
            except pkg.FmxError as e:
                got = ("err", e.code)
            assert got == want, (p, occ, got, want)
        ix.close()


def test_locate_queue_many_launches_one_workspace(pkg, O):
    """200 launches of varying batch sizes on one workspace, issued as one
    fmx_locate_jobs_async queue (the look-back epochs of a workspace wrap
    every 63 launches and its tiles are cleared then): every launch's results
    equal the host API's, batches of different sizes interleaved."""
    import torch
    rng = np.random.default_rng(21)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=100_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    dev = torch.device("cuda:0")
    sizes = [3000, 700, 1, 2049]
    bats = []
    for n in sizes:
        starts = rng.integers(0, text.size - 12, size=n)
        pats = [text[s:s + int(rng.integers(1, 13))].tobytes() for s in starts]
        data, offsets = pkg.pack_patterns(pats)
        want = ix.locate_batch((data, offsets))
        cap = int(want[1].size) + 8
        bats.append(dict(n=n, want=want, cap=cap, data=torch.from_numpy(data.copy()).to(dev),
                         off=torch.from_numpy(offsets.view(np.int64).copy()).to(dev),
                         loff=[torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(2)],
                         locs=[torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(2)],
                         need=torch.zeros(1, dtype=torch.int64, device=dev)))
    ws = ix.locate_workspace_size(max(sizes))
    d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
    jobs = []
    for i in range(200):
        b = bats[i % len(bats)]
        k = (i // len(bats)) % 2  # alternate output buffers: launch i's outputs survive launch i + 4
        jobs.append(ix.locate_job(b["data"].data_ptr(), b["off"].data_ptr(), b["n"], b["loff"][k].data_ptr(),
                                  b["locs"][k].data_ptr(), b["cap"], b["need"].data_ptr(), d_ws.data_ptr(), ws))
    q = ix.job_queue(jobs)
    torch.cuda.synchronize()  # (buffers made on torch's stream; the index launches on its own)
    for rep in range(2):
        ix.locate_jobs_async(q)
        ix.sync()
        for b in bats:
            for k in range(2):
                assert np.array_equal(b["loff"][k].cpu().numpy().view(np.uint64), b["want"][0])
                got = b["locs"][k].cpu().numpy()[:b["want"][1].size].view(np.uint32)
                assert np.array_equal(got, b["want"][1])
            assert int(b["need"].item()) == b["want"][1].size
    ix.close()


def test_locate_group_launch(pkg, O):
    """fmx_locate_group_async: up to 128 batches per launch (more are
    split over launches), sizes from 0 to a few thousand, forward and
    reversed, each batch's outputs equal to the host API's; repeated so the
    workspaces' look-back epochs wrap; a shared workspace is rejected."""
    import torch
    rng = np.random.default_rng(33)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=120_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    dev = torch.device("cuda:0")
    sizes = [2500, 0, 1, 700, 256, 257, 3000, 40, 1999, 5, 1024,
             33, 600, 0, 77, 4096, 12, 300, 2, 900, 128,
             64, 1500, 3, 255, 511, 7, 2048, 90, 0, 333, 17, 1200, 4, 640, 9, 2222, 31, 800, 65]
    sizes += [int(x) for x in np.random.default_rng(5).integers(1, 600, size=100)]  # 140 (138 non-empty): two launches
    bats, jobs = [], []
    for bi, n in enumerate(sizes):
        rev = bi % 3 == 2
        starts = rng.integers(0, text.size - 30, size=n)
        pats = [text[s:s + int(rng.integers(1, 31))].tobytes() for s in starts]
        want = ix.locate_batch(pats)
        q = [p[::-1] for p in pats] if rev else pats
        data, offsets = pkg.pack_patterns(q)
        cap = int(want[1].size) + 8
        b = dict(n=n, want=want, data=torch.from_numpy(np.concatenate([data, np.zeros(1, np.uint8)])).to(dev),
                 off=torch.from_numpy(offsets.view(np.int64).copy()).to(dev),
                 loff=torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
                 locs=torch.zeros(cap, dtype=torch.int32, device=dev), need=torch.zeros(1, dtype=torch.int64, device=dev),
                 cnt=torch.zeros(max(n, 1), dtype=torch.int32, device=dev))
        ws = ix.locate_workspace_size(max(n, 1))
        b["ws"] = torch.zeros(ws, dtype=torch.uint8, device=dev)
        jobs.append(ix.locate_job(b["data"].data_ptr(), b["off"].data_ptr(), n, b["loff"].data_ptr(),
                                  b["locs"].data_ptr(), cap, b["need"].data_ptr(), b["ws"].data_ptr(), ws,
                                  d_counts=b["cnt"].data_ptr(), reversed=rev, stage_kb=2 + bi % 3))
        bats.append(b)
    q = ix.job_queue(jobs)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # (buffers made on torch's stream; the launches use another)
    for rep in range(70):
        ix.locate_group_async(q, stream=stream.cuda_stream)
    ix.sync(stream.cuda_stream)
    for b in bats:
        wo, wl = b["want"]
        assert np.array_equal(b["loff"].cpu().numpy().view(np.uint64), wo)
        assert np.array_equal(b["locs"].cpu().numpy()[:wl.size].view(np.uint32), wl)
        assert int(b["need"].item()) == wl.size
        if b["n"]:
            assert np.array_equal(b["cnt"].cpu().numpy()[:b["n"]].view(np.uint32), np.diff(wo).astype(np.uint32))
    dup = ix.job_queue([jobs[0], jobs[0]])
    with pytest.raises(pkg.FmxError):
        ix.locate_group_async(dup)
    ix.close()


def test_large_batch_scan_kernel(pkg, O):
    """A batch of more than 2048 tiles (524,288 patterns): its tile offsets
    come from the separate k_scan kernel instead of k_emit's own sum."""
    rng = np.random.default_rng(44)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=60_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    n = 600_000
    lens = rng.integers(3, 13, size=n)
    starts = rng.integers(0, text.size - 13, size=n)
    idx = starts[:, None] + np.arange(12)[None, :]
    rows = text[idx]
    data = np.concatenate([rows[i, :lens[i]] for i in range(n)]).astype(np.uint8)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 0))
    ooff, olocs = orc.locate_batch(data, offsets, threads=8)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    goff, glocs = ix.locate_batch((data, offsets))
    assert np.array_equal(goff, ooff) and np.array_equal(glocs, olocs)
    ix.close()


@pytest.mark.parametrize("m", [1, 3, 20, 150, 300])
def test_fixed_len_hint(pkg, O, m):
    """FMX_HINT_FIXED_LEN: the kernels address each pattern at i * m without
    reading the offsets first.  Grouped batches (forward and reversed, several
    sizes; m = 300 overflows the 56 KB LDS stage and reads from HBM) and
    k_count give the oracle's results; offsets that disagree with the hint
    (a wrong length, a nonzero first offset) are reported as FMX_E_ARG."""
    import torch
    rng = np.random.default_rng(100 + m)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=60_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    orc = O.OracleIndex(blob, O.layout(4, 3, 64, 0))
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    dev = torch.device("cuda:0")
    stage_kb = min(56, -(-256 * m // 1024))
    bats, jobs = [], []
    for bi, n in enumerate([700, 1, 256, 2049]):
        rev = bi % 2 == 1
        starts = rng.integers(0, text.size - m, size=n)
        pats = [text[s:s + m].tobytes() for s in starts]
        data, offsets = pkg.pack_patterns(pats)
        want = orc.locate_batch(data, offsets)
        q = [p[::-1] for p in pats] if rev else pats
        data, offsets = pkg.pack_patterns(q)
        cap = int(want[1].size) + 8
        # a wrong (too large) hint below reads n * (m + 1) bytes: fmx.h makes
        # that the caller's buffer size, so the buffer is padded to it
        b = dict(n=n, want=want, data=torch.from_numpy(np.concatenate([data, np.zeros(n + 16, np.uint8)])).to(dev),
                 off=torch.from_numpy(offsets.view(np.int64).copy()).to(dev),
                 loff=torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
                 locs=torch.zeros(cap, dtype=torch.int32, device=dev),
                 need=torch.zeros(1, dtype=torch.int64, device=dev),
                 cnt=torch.zeros(n, dtype=torch.int32, device=dev), cnt2=torch.zeros(n, dtype=torch.int32, device=dev))
        ws = ix.locate_workspace_size(n)
        b["ws"] = torch.zeros(ws, dtype=torch.uint8, device=dev)
        jobs.append(ix.locate_job(b["data"].data_ptr(), b["off"].data_ptr(), n, b["loff"].data_ptr(),
                                  b["locs"].data_ptr(), cap, b["need"].data_ptr(), b["ws"].data_ptr(), ws,
                                  d_counts=b["cnt"].data_ptr(), reversed=rev, stage_kb=stage_kb, fixed_len=m))
        torch.cuda.synchronize()  # (buffers made on torch's stream; the index launches on its own)
        ix.count_batch_async(b["data"].data_ptr(), b["off"].data_ptr(), n, b["cnt2"].data_ptr(),
                             reversed=rev, stage_kb=stage_kb, fixed_len=m)
        bats.append(b)
    ix.sync()
    ix.locate_group_async(ix.job_queue(jobs))
    ix.sync()
    for b in bats:
        wo, wl = b["want"]
        assert np.array_equal(b["loff"].cpu().numpy().view(np.uint64), wo)
        assert np.array_equal(b["locs"].cpu().numpy()[:wl.size].view(np.uint32), wl)
        assert np.array_equal(b["cnt"].cpu().numpy().view(np.uint32), np.diff(wo).astype(np.uint32))
        assert np.array_equal(b["cnt2"].cpu().numpy().view(np.uint32), np.diff(wo).astype(np.uint32))
    # the host API sets the hint itself for equal-length patterns
    data, offsets = pkg.pack_patterns([text[s:s + m].tobytes() for s in starts])
    goff, glocs = ix.locate_batch((data, offsets))
    ooff, olocs = orc.locate_batch(data, offsets)
    assert np.array_equal(goff, ooff) and np.array_equal(glocs, olocs)
    # a hint the offsets contradict
    b = bats[0]
    bad = ix.locate_job(b["data"].data_ptr(), b["off"].data_ptr(), b["n"], b["loff"].data_ptr(),
                        b["locs"].data_ptr(), int(b["locs"].numel()), b["need"].data_ptr(), b["ws"].data_ptr(),
                        int(b["ws"].numel()), stage_kb=stage_kb, fixed_len=m + 1)
    ix.locate_group_async(ix.job_queue([bad]))
    with pytest.raises(pkg.FmxError):
        ix.sync()
    shifted = torch.cat([b["off"][:1] + 1, b["off"][1:]])  # offsets[0] != 0
    ix.count_batch_async(b["data"].data_ptr(), shifted.data_ptr(), b["n"], b["cnt2"].data_ptr(),
                         stage_kb=stage_kb, fixed_len=m)
    with pytest.raises(pkg.FmxError):
        ix.sync()
    ix.sync()  # the status was cleared by the failing sync
    ix.close()


def test_status_is_per_stream(pkg, O):
    """Device-latched errors belong to the stream whose launch raised them
    (ADVICE r1): a bad batch (an empty pattern) on stream B and a good one on
    stream A — fmx_sync(A) is OK, fmx_sync(B) reports FMX_E_EMPTY_PATTERN
    once, and a later sync of B is OK again."""
    import torch
    rng = np.random.default_rng(17)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=50_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    dev = torch.device("cuda:0")
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    good = [text[s:s + 12].tobytes() for s in rng.integers(0, text.size - 12, size=3000)]
    keep = []
    bad = good[:100] + [b""] + good[100:200]
    for pats, st in ((good, sa), (bad, sb)):
        data, offsets = pkg.pack_patterns(pats)
        n = len(pats)
        d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
        o = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        c = torch.zeros(n, dtype=torch.int32, device=dev)
        st.synchronize()
        ix.count_batch_async(d.data_ptr(), o.data_ptr(), n, c.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
        keep.append((d, o, c))
    ix.sync(sa.cuda_stream)  # no error on A
    with pytest.raises(pkg.FmxError) as e:
        ix.sync(sb.cuda_stream)
    assert e.value.code == pkg._native.FMX_E_EMPTY_PATTERN
    ix.sync(sb.cuda_stream)  # reported once, then cleared
    ix.sync()
    ix.close()


def _hip_runtime():
    """The HIP runtime this process already uses (torch's), for raw streams:
    torch.cuda.Stream() hands out a pool of 32, but this test needs distinct
    handles."""
    import ctypes

    import torch
    torch.cuda.init()
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    hip = ctypes.CDLL(path)
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    return hip


def test_status_slots_recycled(pkg, O):
    """An index holds 1024 status words; streams beyond that recycle the least
    recently used word whose stream is idle: 2,300 distinct
    streams, all alive, each run a count batch; every result is right and
    every sync is clean (a recycled word is zeroed for its new owner).  A
    stream that latched an error and never synced either still owns its word
    (reported once) or lost it to recycling (bits dropped);
    fmx_stream_release reports what a stream latched and frees its word."""
    import ctypes

    import torch
    hip = _hip_runtime()
    rng = np.random.default_rng(31)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=30_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    dev = torch.device("cuda:0")
    pats = [text[s:s + 10].tobytes() for s in rng.integers(0, text.size - 10, size=500)]
    want = ix.count_batch(pats)
    data, offsets = pkg.pack_patterns(pats)
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    o = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
    bdata, boffsets = pkg.pack_patterns(pats[:5] + [b""] + pats[5:10])
    bd = torch.from_numpy(np.concatenate([bdata, np.zeros(16, np.uint8)])).to(dev)
    bo = torch.from_numpy(boffsets.view(np.int64).copy()).to(dev)
    bc = torch.zeros(11, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def new_stream():
        s = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
        return s.value

    streams, outs = [], []
    try:
        # a stream latches an error and is never synced
        lost = new_stream()
        streams.append(lost)
        ix.count_batch_async(bd.data_ptr(), bo.data_ptr(), 11, bc.data_ptr(), stream=lost)
        torch.cuda.synchronize()
        outs = [torch.zeros(len(pats), dtype=torch.int32, device=dev) for _ in range(2300)]
        torch.cuda.synchronize()  # (made on torch's stream; the launches use raw streams)
        for i in range(2300):
            s = new_stream()
            streams.append(s)
            ix.count_batch_async(d.data_ptr(), o.data_ptr(), len(pats), outs[i].data_ptr(), stream=s)
            if i % 97 == 0:
                ix.sync(s)
        torch.cuda.synchronize()
        for s in streams[-300:]:
            ix.sync(s)  # clean: a recycled word was zeroed for its new owner
        for c in outs[::50]:
            assert np.array_equal(c.cpu().numpy().view(np.uint32), want)
        try:  # its word was recycled (bits dropped) or is still its own (reported once)
            ix.sync(lost)
        except pkg.FmxError as e:
            assert e.code == pkg._native.FMX_E_EMPTY_PATTERN
        # fmx_stream_release: reports the latched error once, frees the word
        r = new_stream()
        streams.append(r)
        ix.count_batch_async(bd.data_ptr(), bo.data_ptr(), 11, bc.data_ptr(), stream=r)
        with pytest.raises(pkg.FmxError) as e:
            ix.release_stream(r)
        assert e.value.code == pkg._native.FMX_E_EMPTY_PATTERN
        ix.sync(r)
        c = torch.zeros(len(pats), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ix.count_batch_async(d.data_ptr(), o.data_ptr(), len(pats), c.data_ptr(), stream=r)
        ix.release_stream(r)
        assert np.array_equal(c.cpu().numpy().view(np.uint32), want)
        ix.sync()
    finally:
        torch.cuda.synchronize()
        for s in streams:
            hip.hipStreamDestroy(s)
        ix.close()


def test_locate_split_timers(pkg, O):
    """Timing a grouped locate yields the launch and its two kernels
    (locate.search, locate.emit): same launch count, search + emit = launch."""
    import torch
    rng = np.random.default_rng(5)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=200_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    dev = torch.device("cuda:0")
    n, m = 20_000, 16
    starts = rng.integers(0, text.size - m, size=n)
    data = torch.from_numpy(np.stack([text[s:s + m] for s in starts]).reshape(-1).copy()).to(dev)
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * m
    loff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    locs = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    need = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(ix.locate_workspace_size(n), dtype=torch.uint8, device=dev)
    q = ix.job_queue([ix.locate_job(data.data_ptr(), off.data_ptr(), n, loff.data_ptr(), locs.data_ptr(), 4 * n,
                                    need.data_ptr(), ws.data_ptr(), ws.numel(), fixed_len=m)])
    torch.cuda.synchronize()  # (the buffers were made on torch's stream; the index launches on its own)
    ix.timing_enable(True)
    for _ in range(6):
        ix.locate_group_async(q)
    t = ix.timing_read()
    ix.timing_enable(False)
    assert t["locate"]["launches"] == t["locate.search"]["launches"] == t["locate.emit"]["launches"] == 6
    total = t["locate"]["total_ms"]
    assert abs(t["locate.search"]["total_ms"] + t["locate.emit"]["total_ms"] - total) <= 0.02 * total + 1e-3
    assert t["locate.search"]["units"] == 6 * n
    ix.sync()
    ix.close()


def test_concurrent_host_threads(pkg, O):
    """One index driven from several host threads at once (fmx.h: an index is
    thread-safe): 4 threads each run the host-buffer API (count + locate,
    their own pattern sets) and a private-stream async locate with timing on,
    20 rounds each; every result equals the single-threaded answer."""
    import threading

    import torch
    rng = np.random.default_rng(23)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=200_000).astype(np.uint8)
    blob = gpu_build(pkg, text.tobytes(), 5, 4, 3, 64, 3, 2, table)
    ix = pkg.FmIndex.load(blob, pkg.u32, pkg.blocks.Block3(pkg.Vector.U64))
    ix.timing_enable(True)
    dev = torch.device("cuda:0")
    sets = []
    for t in range(4):
        pats = [text[s:s + int(rng.integers(4, 21))].tobytes() for s in rng.integers(0, text.size - 20, 3000 + 500 * t)]
        data, offsets = pkg.pack_patterns(pats)
        want = ix.locate_batch((data, offsets))
        sets.append((pats, data, offsets, want, ix.count_batch((data, offsets))))
    errors = []

    def worker(t):
        try:
            pats, data, offsets, (wo, wl), wc = sets[t]
            st = torch.cuda.Stream(device=dev)
            n = len(pats)
            d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
            o = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
            loff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            cap = int(wl.size) + 8
            locs = torch.zeros(cap, dtype=torch.int32, device=dev)
            need = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = ix.locate_workspace_size(n)
            wsb = torch.zeros(ws, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            for _ in range(20):
                go, gl = ix.locate_batch((data, offsets))
                assert np.array_equal(go, wo) and np.array_equal(gl, wl)
                assert np.array_equal(ix.count_batch((data, offsets)), wc)
                ix.locate_batch_async(d.data_ptr(), o.data_ptr(), n, loff.data_ptr(), locs.data_ptr(), cap,
                                      need.data_ptr(), wsb.data_ptr(), ws, stream=st.cuda_stream)
                ix.sync(st.cuda_stream)
                assert np.array_equal(loff.cpu().numpy().view(np.uint64), wo)
                assert np.array_equal(locs.cpu().numpy()[:wl.size].view(np.uint32), wl)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert ix.timing_read()  # the timers saw the threads' launches
    ix.close()


@pytest.mark.parametrize("sigma,budget,pb", [(4, 2 << 20, 4), (5, 32 << 20, 8)])
def test_max_memory_large_k(pkg, O, sigma, budget, pb):
    """LookupTableConfig::MaxMemory (lookup_table_config.rs:23-51) with k >= 8:
    the k-mer count table (1.5 MB / 13 MB) is far past the kernels' LDS copy
    and is read from HBM; patterns shorter and longer than k, absent k-mers,
    wildcard bytes — builder bytes and every result equal the oracle's."""
    rng = np.random.default_rng(sigma * 1000 + pb)
    chars = b"ACGT" if sigma == 4 else b"ACGTN"
    table = table_from_symbols([bytes([c]) for c in chars])
    position = pos_of(pkg, pb)
    k = pkg.build_config.LookupTableConfig.MaxMemory(budget).kmer_size(position, sigma)
    assert k >= 8 and (sigma + 1) ** k * pb <= budget < (sigma + 1) ** (k + 1) * pb
    text = bytes(rng.choice(np.frombuffer(chars, np.uint8), size=300_000))
    planes, vb = (2, 64) if pb == 4 else (3, 128)
    blob = gpu_build(pkg, text, sigma, pb, planes, vb, k, 2, table)
    assert np.array_equal(blob, O.build(text, sigma, O.layout(pb, planes, vb), k, 2, table))
    pats = [rand_pattern(rng, text, 1, 30) for _ in range(3000)]
    pats += [bytes(rng.choice(np.frombuffer(chars, np.uint8), size=int(rng.integers(8, 16)))) for _ in range(300)]
    pats += [b"Z" * 9, b"A" * 12, chars * 3]
    for occ in (0, 1, 63):
        check_parity(pkg, O, blob, pb, planes, vb, 0, pats, occ, reversed_too=(occ == 1))


def test_builder_sa64_small(pkg, O, monkeypatch):
    """The 64-bit suffix-array path (bucketed prefix doubling, used for
    n + 1 >= 2^32; forced here with FMX_BUILD_SA64=1) writes the oracle's
    blob byte for byte: random texts, long runs (many doubling rounds),
    n % BL == 0, a one-symbol text, several layouts."""
    monkeypatch.setenv("FMX_BUILD_SA64", "1")
    rng = np.random.default_rng(64)
    table = table_from_symbols([b"A", b"C", b"G", b"T", b"N"])
    texts = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=20000)),
             b"A" * 5000 + bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=300)) + b"AC" * 3000,
             b"ACGT" * 64, b"G" * 777, b"N"]
    for text in texts:
        for pb, planes, vb, k, sr in [(4, 3, 64, 3, 2), (8, 3, 128, 4, 3), (8, 3, 32, 1, 1)]:
            blob = gpu_build(pkg, text, 5, pb, planes, vb, k, sr, table)
            ref = O.build(text, 5, O.layout(pb, planes, vb), k, sr, table)
            assert np.array_equal(blob, ref), (len(text), pb, planes, vb)
