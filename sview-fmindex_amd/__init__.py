"""sview-fmindex_amd — MI355X-native batched FM-index count/locate.

Host-side mirror of baku4/sview-fmindex's public surface for its query hot
path, over the engine's C ABI (``include/fmx.h``, ``lib/libfmx.so``):

=============================  ===========================================================
this module                    reference (sview-fmindex/src/...)
=============================  ===========================================================
``FmIndex.load``               ``FmIndex::load``                 load_from_blob.rs:28-85
``FmIndex.count``              ``FmIndex::count``                locate/with_slice.rs:5-8
``FmIndex.locate``             ``FmIndex::locate``               locate/with_slice.rs:10-13
``FmIndex.locate_to_buffer``   ``FmIndex::locate_to_buffer``     locate/with_slice.rs:15-18
``FmIndex.*_rev_iter``         ``FmIndex::*_rev_iter``           locate/with_rev_iter.rs:5-19
``FmIndex.blob``               ``FmIndex::blob``                 reference_to_source_blob.rs:9-11
``FmIndex.count_batch`` /      (new) one kernel launch for a whole pattern batch
``FmIndex.locate_batch``
``FmIndex.match`` /            (new) longest-suffix match: greedy backward seeding
``FmIndex.match_batch``
``FmIndex.seeds`` /            (new) greedy seed chains: the match restarted on ever shorter prefixes
``FmIndex.seeds_batch``
``FmIndex.approx`` /           (new) k-mismatch search: every variant within max_mm substitutions
``FmIndex.approx_batch``
``FmIndexBuilder``            ``FmIndexBuilder``                builder/mod.rs:59-264 (built on the GPU)
``blocks.Block2..Block6``      ``blocks::Block2..Block6<V>``     components/bwm/blocks/
``text_encoders.*``            ``EncodingTable`` / ``PassThrough`` components/text_encoder/
``build_config.*``             ``LookupTableConfig`` / ``SuffixArrayConfig`` builder/build_config/
``LoadError`` / ``BuildError``  the reference's error enums       load_from_blob.rs:16-24, builder/mod.rs:37-57
=============================  ===========================================================

Generic parameters the reference carries in the type (``P``, ``B``, ``E``) are
passed as arguments here.  Every query runs the gfx950 kernels; there is no
CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as _n
from . import distributed  # noqa: F401  (multi-GPU helpers)

__all__ = ["FmIndex", "FmIndexBuilder", "Position", "u32", "u64", "Vector", "blocks",
           "text_encoders", "build_config", "LoadError", "BuildError", "FmxError",
           "aligned_buffer", "pack_patterns", "complement_map", "OPT_VERIFY_TEXT"]

# load option (OR it into `options`): keep the text in HBM for verify_async / map_batch only; no search reads
# it and the index stays the one the other options make (FMX_OPT_VERIFY_TEXT, fmx.h)
OPT_VERIFY_TEXT = _n.FMX_OPT_VERIFY_TEXT


# ------------------------------------------------------------------ errors

class FmxError(RuntimeError):
    """A failure of the engine that the reference would report as a panic or
    that has no reference counterpart (device errors)."""

    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{_n.status_str(code)} (fmx status {code}){': ' + what if what else ''}")


class LoadError(Exception):
    """``LoadError`` (load_from_blob.rs:16-24)."""


class InvalidFormat(LoadError):
    def __init__(self):
        super().__init__("Invalid FM-index format. The data does not appear to be a valid FM-index blob.")


class MismatchedBlobSize(LoadError):
    def __init__(self, expected: int, actual: int):
        self.expected, self.actual = expected, actual
        super().__init__(f"Mismatched blob size: headers indicate a total size of {expected} bytes, "
                         f"but the provided blob is {actual} bytes.")


LoadError.InvalidFormat = InvalidFormat
LoadError.MismatchedBlobSize = MismatchedBlobSize


class BuildError(Exception):
    """``BuildError`` (builder/mod.rs:37-57)."""


class SymbolCountOver(BuildError):
    def __init__(self, maximum: int, got: int):
        super().__init__(f"The symbol count ({got}) exceeds the maximum for the chosen block type ({maximum}).")


class UnmatchedTextLength(BuildError):
    def __init__(self, expected: int, got: int):
        super().__init__(f"Mismatched text length: expected {expected} bytes, but got {got} bytes.")


class InvalidBlobSize(BuildError):
    def __init__(self, expected: int, got: int):
        super().__init__(f"Incorrect blob size: expected {expected} bytes, but got {got} bytes.")


class NotAlignedBlob(BuildError):
    def __init__(self, required: int, offset: int):
        super().__init__(f"Improper blob alignment: required alignment is {required} bytes, "
                         f"but the blob has an offset of {offset} bytes.")


class InvalidConfig(BuildError):
    pass


for _c in (SymbolCountOver, UnmatchedTextLength, InvalidBlobSize, NotAlignedBlob, InvalidConfig):
    setattr(BuildError, _c.__name__, _c)


def _check(code: int, what: str = ""):
    if code != _n.FMX_OK:
        raise FmxError(code, what)


# ------------------------------------------------------------ type params

class Position:
    """``Position`` (text_length.rs:10-129): u32 or u64."""

    def __init__(self, nbytes: int):
        self.nbytes = nbytes
        self.dtype = np.dtype(np.uint32 if nbytes == 4 else np.uint64)

    def __repr__(self):
        return f"u{self.nbytes * 8}"


u32 = Position(4)
u64 = Position(8)


class Vector:
    """``Vector`` (blocks/vector.rs:11-79): u32 / u64 / u128."""

    def __init__(self, bits: int):
        self.bits = bits
        self.BLOCK_LEN = bits
        self.ALIGN_SIZE = 16 if bits == 128 else 8

    def __repr__(self):
        return f"u{self.bits}"


Vector.U32, Vector.U64, Vector.U128 = Vector(32), Vector(64), Vector(128)


class _Block:
    PLANES = 0

    def __init__(self, vector: Vector = Vector.U64):
        if isinstance(vector, int):
            vector = Vector(vector)
        self.vector = vector

    @property
    def planes(self):
        return self.PLANES

    @property
    def BLOCK_LEN(self):
        return self.vector.bits

    @property
    def MAX_SYMBOL(self):
        return 1 << self.PLANES

    @property
    def ALIGN_SIZE(self):
        return self.vector.ALIGN_SIZE

    def __repr__(self):
        return f"Block{self.PLANES}<{self.vector!r}>"


class blocks:
    """``blocks::Block2..Block6<V>`` (components/bwm/blocks/)."""

    class Block2(_Block):
        PLANES = 2

    class Block3(_Block):
        PLANES = 3

    class Block4(_Block):
        PLANES = 4

    class Block5(_Block):
        PLANES = 5

    class Block6(_Block):
        PLANES = 6


class text_encoders:
    """``text_encoders`` (components/text_encoder/text_encoders/)."""

    class EncodingTable:
        """``EncodingTable([u8; 256])`` (encoding_table.rs:7-39)."""
        ENCODER = _n.FMX_ENC_TABLE

        def __init__(self, table: bytes):
            if len(table) != 256:
                raise ValueError("EncodingTable needs 256 bytes")
            self.table = bytes(table)

        @classmethod
        def from_symbols(cls, symbols: Sequence[bytes]):
            """Last symbol is the wildcard (encoding_table.rs:15-26)."""
            count = len(symbols)
            t = bytearray([count - 1] * 256)
            for idx, sym in enumerate(symbols):
                for x in bytes(sym):
                    t[x] = idx
            return cls(bytes(t))

        @classmethod
        def from_symbols_with_wildcard(cls, symbols: Sequence[bytes]):
            """One extra wildcard symbol (encoding_table.rs:27-35)."""
            count = len(symbols) + 1
            t = bytearray([count - 1] * 256)
            for idx, sym in enumerate(symbols):
                for x in bytes(sym):
                    t[x] = idx
            return cls(bytes(t))

        def symbol_count(self) -> int:
            return max(self.table) + 1

        def idx_of(self, sym: int) -> int:
            return self.table[sym]

    class PassThrough:
        """``PassThrough`` (pass_through.rs:6-12): bytes are already symbol indices."""
        ENCODER = _n.FMX_ENC_PASS
        table = None

        def idx_of(self, sym: int) -> int:
            return sym


class build_config:
    """``build_config`` (builder/build_config/)."""

    class LookupTableConfig:
        def __init__(self, kind: str, value: int = 0):
            self.kind, self.value = kind, value

        @classmethod
        def None_(cls):
            return cls("None")

        @classmethod
        def KmerSize(cls, k: int):
            return cls("KmerSize", k)

        @classmethod
        def MaxMemory(cls, nbytes: int):
            return cls("MaxMemory", nbytes)

        def kmer_size(self, position: Position, symbol_count: int) -> int:
            """lookup_table_config.rs:22-51."""
            if self.kind == "None":
                return 1
            if self.kind == "KmerSize":
                if self.value < 2:
                    raise InvalidConfig("K-mer size must be at least 2")
                return self.value
            k = 2
            while (symbol_count + 1) ** k * position.nbytes <= self.value:
                k += 1
            return k - 1

    class SuffixArrayConfig:
        def __init__(self, kind: str, value: int = 1):
            self.kind, self.value = kind, value

        @classmethod
        def Uncompressed(cls):
            return cls("Uncompressed", 1)

        @classmethod
        def Compressed(cls, ratio: int):
            return cls("Compressed", ratio)

        def sampling_ratio(self) -> int:
            """suffix_array_config.rs:17-32."""
            if self.kind == "Uncompressed":
                return 1
            if self.value < 2:
                raise InvalidConfig("Sampling ratio for compressed suffix array must be at least 2")
            return self.value


build_config.LookupTableConfig.default = staticmethod(build_config.LookupTableConfig.None_)
build_config.SuffixArrayConfig.default = staticmethod(build_config.SuffixArrayConfig.Uncompressed)


# ----------------------------------------------------------------- helpers

def aligned_buffer(nbytes: int, align: int = 16) -> np.ndarray:
    """A zeroed uint8 host buffer whose data pointer is `align`-aligned."""
    raw = np.zeros(nbytes + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def pack_patterns(patterns: Iterable[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """Ragged patterns -> (bytes uint8[total], offsets uint64[n+1])."""
    pats = [bytes(p) for p in patterns]
    lens = np.fromiter((len(p) for p in pats), dtype=np.uint64, count=len(pats))
    offsets = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(pats), dtype=np.uint8) if pats else np.zeros(0, np.uint8)
    return data, offsets


def _layout(position: Position, block: _Block, encoder) -> _n.fmx_layout:
    return _n.fmx_layout(position.nbytes, block.planes, block.vector.bits, encoder.ENCODER)


def _options(occ: str, deep_lut: bool, full_sa: bool = True, text: bool = True, context: bool = True,
             lut_rows: bool = True) -> int:
    mode = _n.FMX_OCC_INTERLEAVED if occ == "interleaved" else _n.FMX_OCC_BLOB
    return (mode | (_n.FMX_OPT_DEEP_LUT if deep_lut else 0) | (_n.FMX_OPT_FULL_SA if full_sa else 0)
            | (_n.FMX_OPT_TEXT if text else 0) | (_n.FMX_OPT_ROW_CONTEXT if context else 0)
            | (_n.FMX_OPT_LUT_ROWS if lut_rows else 0))


def _flags(reversed: bool, long_patterns: bool, stage_kb: int = 0, fixed_len: int = 0) -> int:
    """Query flags: FMX_PATTERN_REVERSED, FMX_HINT_LONG_PATTERNS,
    FMX_HINT_STAGE_KB(stage_kb) (LDS KB per 256-pattern tile; 0 = no hint) and
    FMX_HINT_FIXED_LEN(fixed_len) (every pattern fixed_len bytes, offsets[i] ==
    i * fixed_len; 0 = no hint)."""
    if not 0 <= int(fixed_len) <= 0xFFFF:
        raise ValueError("fixed_len must be in 0..65535")
    return ((_n.FMX_PATTERN_REVERSED if reversed else 0) | (_n.FMX_HINT_LONG_PATTERNS if long_patterns else 0)
            | ((int(stage_kb) & 0xFF) << 8) | (int(fixed_len) << 16))


def _strand_flags(strands: str) -> int:
    """strands = "forward" | "reverse" | "both": no flag, FMX_PATTERN_REVCOMP or
    FMX_BOTH_STRANDS (the last two need FmIndex.set_complement)."""
    try:
        return {"forward": 0, "reverse": _n.FMX_PATTERN_REVCOMP, "both": _n.FMX_BOTH_STRANDS}[strands]
    except KeyError:
        raise ValueError('strands must be "forward", "reverse" or "both"') from None


def complement_map(pairs: Iterable[Tuple[bytes, bytes]]) -> bytes:
    """A 256-byte complement map that swaps the two bytes of each pair and
    leaves every other byte as it is: complement_map([(b"A", b"T"), (b"C",
    b"G")]) for upper-case DNA."""
    m = bytearray(range(256))
    for a, b in pairs:
        (x,), (y,) = bytes(a), bytes(b)
        m[x], m[y] = y, x
    return bytes(m)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _vp(x: int):
    """An optional device pointer (or stream) of the async calls: 0 = NULL."""
    return C.c_void_p(x) if x else None


def _host_query(name: str, h, dt, patterns, reversed: bool, params: Optional[tuple] = None,
                max_occ: Optional[int] = None, outs=lambda n: (), per: int = 1, locate: bool = True,
                cap: int = 1 << 16, strands: str = "forward"):
    """One host-buffer query `name(h, bytes, offsets, n, flags, *params,
    max_occ, *outs(n), loc_offsets, locations, cap, &needed)` (params None: a
    call without them and without max_occ): the patterns packed, max_occ None
    as no bound, and — with `locate` — the locations of n * per slots, their
    buffer grown to `needed` and the call repeated once on FMX_E_CAPACITY.
    Returns (n, outputs, loc_offsets uint64[n * per + 1], locations[:needed]),
    the last two None without `locate`; under strands="both" the returned n
    and every output count the 2n virtual patterns (read i's strand s: 2 i +
    s)."""
    data, offsets = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
    reads = offsets.size - 1
    n = 2 * reads if strands == "both" else reads
    out = outs(n)
    flags = (_n.FMX_PATTERN_REVERSED if reversed else 0) | _strand_flags(strands)
    mid = () if params is None else params + ((1 << 64) - 1 if max_occ is None else int(max_occ),)
    head = (h, _ptr(data) if data.size else None, _ptr(offsets), reads, flags) + mid + tuple(_ptr(o) for o in out)
    fn = getattr(_n.lib(), name)
    needed = C.c_uint64()
    if not locate:
        _check(fn(*head, None, None, 0, C.byref(needed)), name)
        return n, out, None, None
    loc_off = np.zeros(n * max(per, 0) + 1, dtype=np.uint64)
    locs = np.zeros(max(cap, 1), dtype=dt)
    st = fn(*head, _ptr(loc_off), _ptr(locs), cap, C.byref(needed))
    if st == _n.FMX_E_CAPACITY:  # (the first guess was short: once more with room for every location)
        cap = needed.value
        locs = np.zeros(max(cap, 1), dtype=dt)
        st = fn(*head, _ptr(loc_off), _ptr(locs), cap, C.byref(needed))
    _check(st, name)
    return n, out, loc_off, locs[:needed.value]


def _load(name: str, call, position: Position, block: Optional[_Block], text_encoder, blob=None, table=None):
    """What every load shares: the default block, an encoder class made an
    instance, a host `blob` realigned to the block's vectors, the native
    ``call(layout, arr, h, exp, act)``, the reference's two load errors, and
    the table of an `EncodingTable` that has none yet recovered from the blob's
    header (`table(offset)` reads its 256 bytes where the blob is not in host
    memory).  Returns (handle, block, encoder, the blob as loaded)."""
    block = block or blocks.Block2(Vector.U64)
    if isinstance(text_encoder, type):
        text_encoder = text_encoder.__new__(text_encoder)
    arr = None
    if blob is not None:
        arr = blob if isinstance(blob, np.ndarray) else np.frombuffer(bytes(blob), dtype=np.uint8)
        if arr.ctypes.data % block.ALIGN_SIZE:
            a2 = aligned_buffer(arr.size, 16)
            a2[:] = arr
            arr = a2

        def table(offset):
            return bytes(arr[offset:][:256])

    h = C.c_void_p()
    exp, act = C.c_uint64(), C.c_uint64()
    st = call(_layout(position, block, text_encoder), arr, C.byref(h), C.byref(exp), C.byref(act))
    if st == _n.FMX_E_FORMAT:
        raise InvalidFormat()
    if st == _n.FMX_E_SIZE:
        raise MismatchedBlobSize(exp.value, act.value)
    _check(st, name)
    if table and isinstance(text_encoder, text_encoders.EncodingTable) and not hasattr(text_encoder, "table"):
        text_encoder.table = table(8 if block.ALIGN_SIZE == 8 else 16)
    return h, block, text_encoder, arr


# ----------------------------------------------------------------- FmIndex

class FmIndex:
    """``FmIndex<'a, P, B, E>`` (lib.rs:14-28), resident in HBM of one GPU."""

    def __init__(self, handle, position: Position, block: _Block, encoder, blob):
        self._h = handle
        self.position = position
        self.block = block
        self.text_encoder = encoder
        self._blob = blob  # keeps the borrowed host blob alive (fmx_blob)
        self._dt = position.dtype

    # -- load ---------------------------------------------------------
    @classmethod
    def load(cls, blob, position: Position = u32, block: Optional[_Block] = None,
             text_encoder=text_encoders.EncodingTable, device: int = 0,
             occ: str = "interleaved", deep_lut: bool = False, full_sa: bool = False, text: bool = False,
             context: bool = False, lut_rows: bool = False, options: Optional[int] = None) -> "FmIndex":
        """``FmIndex::load`` (load_from_blob.rs:28-85): validate, then copy the
        blob to HBM once.  By default the index is the reference's own: the
        blob, its occ planes and checkpoints re-laid out as one record per
        block (FMX_OPT_DEFAULT).  The flags add derived device structures
        (results are identical with any of them; they cost HBM — ~55x the
        blob at C2 with all of them — and load time; bench.py "derived"):
        `occ` — "blob" reads the blob's arrays as they are, "interleaved"
        re-lays checkpoint + planes into one HBM line per block; `deep_lut` —
        the device K-mer interval table (FMX_OPT_DEEP_LUT); `full_sa` — the
        full suffix array (FMX_OPT_FULL_SA); `text` — the recovered text for
        single-row tail verification (FMX_OPT_TEXT); `context` — row records
        {SA, preceding symbols} so that small intervals finish with one scan
        (FMX_OPT_ROW_CONTEXT); `lut_rows` — single-row deep-table entries
        that hold the row's location (FMX_OPT_LUT_ROWS).  `options` overrides all
        (FMX_OPT_DERIVED: every derived structure)."""
        mode = options if options is not None else _options(occ, deep_lut, full_sa, text, context, lut_rows)
        h, block, text_encoder, arr = _load(
            "fmx_load", lambda layout, arr, *out: _n.lib().fmx_load(_ptr(arr), arr.size, layout, device, mode, *out),
            position, block, text_encoder, blob=blob)
        return cls(h, position, block, text_encoder, arr)

    @classmethod
    def load_device(cls, d_blob: int, blob_len: int, position: Position = u32,
                    block: Optional[_Block] = None, text_encoder=text_encoders.EncodingTable,
                    device: int = 0, occ: str = "interleaved", deep_lut: bool = False, full_sa: bool = False,
                    text: bool = False, context: bool = False, lut_rows: bool = False,
                    options: Optional[int] = None) -> "FmIndex":
        """Load a blob already resident in HBM (borrowed, must outlive the index)."""
        mode = options if options is not None else _options(occ, deep_lut, full_sa, text, context, lut_rows)
        h, block, text_encoder, _ = _load(
            "fmx_load_device",
            lambda layout, _, *out: _n.lib().fmx_load_device(C.c_void_p(d_blob), blob_len, layout, device, mode, *out),
            position, block, text_encoder)
        return cls(h, position, block, text_encoder, None)

    @classmethod
    def load_file(cls, path, position: Position = u32, block: Optional[_Block] = None,
                  text_encoder=text_encoders.EncodingTable, device: int = 0, occ: str = "interleaved",
                  deep_lut: bool = False, full_sa: bool = False, text: bool = False, context: bool = False,
                  lut_rows: bool = False, options: Optional[int] = None, chunk_bytes: int = 0,
                  direct: bool = False) -> "FmIndex":
        """Blob file -> HBM (fmx_load_file): what the bench's mmap loader
        (bench/src/locate/sview_mmap.rs:17-45) followed by ``FmIndex::load``
        does, as a streamed ingest — the header is validated from the file,
        then the body is read in pinned chunks overlapped with their DMA.
        `direct`: the body is read with O_DIRECT (FMX_LOAD_DIRECT), bypassing
        the page cache — a cold load (raises if the file system refuses it)."""
        mode = options if options is not None else _options(occ, deep_lut, full_sa, text, context, lut_rows)
        if direct:
            mode |= _n.FMX_LOAD_DIRECT

        def table(offset):
            with open(path, "rb") as f:
                f.seek(offset)
                return f.read(256)

        h, block, text_encoder, _ = _load(
            f"fmx_load_file({path})",
            lambda layout, _, *out: _n.lib().fmx_load_file(os.fsencode(path), layout, device, mode, int(chunk_bytes),
                                                           *out),
            position, block, text_encoder, table=table)
        return cls(h, position, block, text_encoder, None)

    def close(self):
        if self._h:
            _n.lib().fmx_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def blob(self) -> Optional[memoryview]:
        """``FmIndex::blob`` (reference_to_source_blob.rs:9-11)."""
        return None if self._blob is None else memoryview(self._blob)

    def info(self) -> dict:
        i = _n.fmx_index_info()
        _check(_n.lib().fmx_info(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in i._fields_}

    # -- the complement map of strands="reverse" / "both" ------------------
    def set_complement(self, map: Optional[bytes]) -> None:
        """fmx_set_complement: `map` is 256 bytes, byte -> complement byte (see
        complement_map), or None to remove it.  Not to be called while strand
        queries of this index are in flight."""
        if map is not None:
            map = bytes(map)
            if len(map) != 256:
                raise ValueError("a complement map is 256 bytes")
        _check(_n.lib().fmx_set_complement(self._h, map), "fmx_set_complement")

    @property
    def complement(self) -> Optional[bytes]:
        """The map that was set, or None."""
        buf = C.create_string_buffer(256)
        st = _n.lib().fmx_get_complement(self._h, buf)
        if st == _n.FMX_E_ARG:
            return None
        _check(st, "fmx_get_complement")
        return buf.raw

    # -- single-pattern API (the reference's own) -----------------------
    def count(self, pattern: bytes) -> int:
        """``FmIndex::count`` (with_slice.rs:5-8)."""
        return int(self.count_batch([pattern])[0])

    def locate(self, pattern: bytes) -> List[int]:
        """``FmIndex::locate`` (with_slice.rs:10-13): suffix-array-row order."""
        _, locs = self.locate_batch([pattern])
        return [int(x) for x in locs]

    def locate_to_buffer(self, pattern: bytes, buffer: list) -> None:
        """``FmIndex::locate_to_buffer`` (with_slice.rs:15-18): appends."""
        buffer.extend(self.locate(pattern))

    def count_rev_iter(self, pattern_rev_iter: Iterable[int]) -> int:
        """``FmIndex::count_rev_iter`` (with_rev_iter.rs:5-9)."""
        rev = bytes(pattern_rev_iter)
        return int(self.count_batch([rev], reversed=True)[0])

    def locate_rev_iter(self, pattern_rev_iter: Iterable[int]) -> List[int]:
        """``FmIndex::locate_rev_iter`` (with_rev_iter.rs:10-14)."""
        rev = bytes(pattern_rev_iter)
        _, locs = self.locate_batch([rev], reversed=True)
        return [int(x) for x in locs]

    def locate_rev_iter_to_buffer(self, pattern_rev_iter: Iterable[int], buffer: list) -> None:
        buffer.extend(self.locate_rev_iter(pattern_rev_iter))

    # -- batched API -----------------------------------------------------
    def count_batch(self, patterns, reversed: bool = False) -> np.ndarray:
        """Counts of many patterns in one launch (P-typed numpy array)."""
        data, offsets = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        n = offsets.size - 1
        out = np.zeros(max(n, 1), dtype=self._dt)
        flags = _n.FMX_PATTERN_REVERSED if reversed else 0
        _check(_n.lib().fmx_count_batch(self._h, _ptr(data) if data.size else None, _ptr(offsets), n,
                                        flags, _ptr(out)), "fmx_count_batch")
        return out[:n]

    def locate_batch(self, patterns, reversed: bool = False,
                     cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Locations of many patterns: (offsets uint64[n+1], locations P[total]);
        pattern i's locations are locations[offsets[i]:offsets[i+1]] in
        suffix-array-row order."""
        return _host_query("fmx_locate_batch", self._h, self._dt, patterns, reversed,
                           cap=(1 << 16) if cap is None else cap)[2:]

    # -- longest-suffix match (greedy backward seeding) ---------------------
    def match(self, pattern: bytes, strands: str = "forward"):
        """(length, lo, hi): the longest suffix of `pattern` that occurs in the
        text and its suffix-array interval (hi - lo occurrences; (0, 0, 0)
        when not even the last symbol occurs).  strands="reverse": of the
        pattern's reverse complement; "both": a (forward, reverse) pair."""
        lens, rng = self.match_batch([pattern], locate=False, strands=strands)
        res = [(int(lens[v]), int(rng[v, 0]), int(rng[v, 1])) for v in range(lens.size)]
        return tuple(res) if strands == "both" else res[0]

    def match_batch(self, patterns, reversed: bool = False, locate: bool = True, min_len: int = 1,
                    max_occ: Optional[int] = None, strands: str = "forward"):
        """Longest-suffix match of many patterns (fmx_match_batch): (lens
        uint32[n], ranges P[n, 2]) and, with `locate`, (..., loc_offsets
        uint64[n+1], locations P[total]).  lens[i] is the length of the longest
        suffix of pattern i that occurs in the text and ranges[i] = (lo, hi) its
        interval, always the true values; locations (suffix-array-row order)
        are emitted only for patterns with lens[i] >= max(min_len, 1) and
        hi - lo <= max_occ (None: no bound).  `strands` (here and in
        seeds_batch / approx_batch; needs set_complement): "reverse" answers
        for each pattern's reverse complement rc(p)[j] = map[p[m-1-j]] instead,
        "both" for the 2n patterns p_0, rc(p_0), p_1, rc(p_1), ... — every
        array then has 2n patterns' entries, flat, and positions within a
        reverse strand are in rc(p)'s own coordinates."""
        outs = lambda n: (np.zeros(max(n, 1), dtype=np.uint32), np.zeros((max(n, 1), 2), dtype=self._dt))  # noqa: E731
        n, (lens, rng), loff, locs = _host_query("fmx_match_batch", self._h, self._dt, patterns, reversed,
                                                 (int(min_len),), max_occ, outs, locate=locate, strands=strands)
        return (lens[:n], rng[:n]) + ((loff, locs) if locate else ())

    # -- greedy seed chains (the match restarted until the pattern is used up) --
    def seeds(self, pattern: bytes, max_seeds: int = 8, min_len: int = 1, skip: int = 0,
              max_occ: Optional[int] = None, strands: str = "forward"):
        """The pattern's seeds, right to left: [(end, len, lo, hi)], seed j
        covering pattern[end - len:end] with suffix-array interval [lo, hi).
        (max_occ only selects which seeds seeds_batch locates.)  strands=
        "both": a (forward, reverse) pair of such lists."""
        ns, _, spans, rng = self.seeds_batch([pattern], max_seeds, min_len, skip, max_occ, locate=False,
                                             strands=strands)
        res = [[(int(spans[v, j, 0]), int(spans[v, j, 1]), int(rng[v, j, 0]), int(rng[v, j, 1]))
                for j in range(int(ns[v]))] for v in range(ns.size)]
        return tuple(res) if strands == "both" else res[0]

    def seeds_batch(self, patterns, max_seeds: int = 8, min_len: int = 1, skip: int = 0,
                    max_occ: Optional[int] = None, reversed: bool = False, locate: bool = True,
                    strands: str = "forward"):
        """Greedy seed chains of many patterns (fmx_seeds_batch): (nseeds
        uint32[n], rest uint32[n], spans uint32[n, max_seeds, 2], ranges P[n,
        max_seeds, 2]) and, with `locate`, (..., loc_offsets uint64[n *
        max_seeds + 1], locations P[total]).  With e = len(p): the longest
        suffix of p[:e] that occurs in the text, of length L with interval (lo,
        hi), is a seed when L >= max(min_len, 1) — spans[i, j] = (e, L),
        ranges[i, j] = (lo, hi) — then e -= min(e, max(L + skip, 1)), until e =
        0 or max_seeds are stored; rest[i] = the e left (0: all parsed); unused
        slots are zero.  Slot i * max_seeds + j holds the seed's locations
        (suffix-array-row order) when hi - lo <= max_occ (None: no bound)."""
        ms = int(max_seeds)

        def outs(n):
            rows = max(n, 1) * max(ms, 1)
            return (np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32),
                    np.zeros((rows, 2), dtype=np.uint32), np.zeros((rows, 2), dtype=self._dt))

        n, (ns, rest, spans, rng), loff, locs = _host_query("fmx_seeds_batch", self._h, self._dt, patterns, reversed,
                                                            (ms, int(min_len), int(skip)), max_occ, outs, ms, locate,
                                                            strands=strands)
        return ((ns[:n], rest[:n], spans[:n * ms].reshape(n, ms, 2), rng[:n * ms].reshape(n, ms, 2))
                + ((loff, locs) if locate else ()))

    # -- k-mismatch search (substitutions only, a bounded backtracking walk on the device) --
    def approx(self, pattern: bytes, max_mm: int = 1, max_hits: int = 8, best: bool = False,
               strands: str = "forward"):
        """The pattern's variants within max_mm substitutions that occur in
        the text, in the contract's order: [(d, [(pos, sym), ...], lo, hi)],
        the d substitutions by decreasing position (sym a symbol index), [lo,
        hi) the variant's suffix-array interval; at most max_hits of them.
        strands="both": a (forward, reverse) pair of such lists."""
        nh, _, mm, subs, rng = self.approx_batch([pattern], max_mm, max_hits, best, locate=False, strands=strands)
        res = [[(int(mm[v, j]), [(int(subs[v, j, t, 0]), int(subs[v, j, t, 1])) for t in range(int(mm[v, j]))],
                 int(rng[v, j, 0]), int(rng[v, j, 1])) for j in range(int(nh[v]))] for v in range(nh.size)]
        return tuple(res) if strands == "both" else res[0]

    def approx_batch(self, patterns, max_mm: int = 1, max_hits: int = 8, best: bool = False,
                     max_occ: Optional[int] = None, reversed: bool = False, locate: bool = True,
                     strands: str = "forward"):
        """k-mismatch search of many patterns (fmx_approx_batch): (nhits
        uint32[n], more uint32[n], mm uint32[n, max_hits], subs uint32[n,
        max_hits, 3, 2], ranges P[n, max_hits, 2]) and, with `locate`, (...,
        loc_offsets uint64[n * max_hits + 1], locations P[total]).  A variant
        differs from the pattern in d <= max_mm positions (substitutions only)
        and occurs in the text; they come by d ascending, then — scanning the
        positions from the last to the first — a substituted symbol before the
        pattern's own, a smaller substituted symbol first.  `best` keeps the
        smallest d that has any.  nhits[i] of them are stored (more[i]: there
        are others): mm[i, j] = d, subs[i, j, t] = (position, symbol index) of
        substitution t < d by decreasing position, ranges[i, j] = (lo, hi);
        unused entries are zero.  Slot i * max_hits + j holds the variant's
        locations (suffix-array-row order) when hi - lo <= max_occ (None: no
        bound)."""
        mh = int(max_hits)

        def outs(n):
            rows = max(n, 1) * max(mh, 1)
            return (np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32),
                    np.zeros(rows, dtype=np.uint32), np.zeros((rows, 6), dtype=np.uint32),
                    np.zeros((rows, 2), dtype=self._dt))

        params = (int(max_mm), mh, _n.FMX_APPROX_BEST if best else 0)
        n, (nh, more, mm, subs, rng), loff, locs = _host_query("fmx_approx_batch", self._h, self._dt, patterns,
                                                               reversed, params, max_occ, outs, mh, locate,
                                                               strands=strands)
        return ((nh[:n], more[:n], mm[:n * mh].reshape(n, mh), subs[:n * mh].reshape(n, mh, 3, 2),
                 rng[:n * mh].reshape(n, mh, 2)) + ((loff, locs) if locate else ()))

    # -- placing reads: seeds -> locations -> diagonal vote, all on the device --
    def place(self, pattern: bytes, max_seeds: int = 8, min_len: int = 1, skip: int = 0, max_occ: int = 16,
              band: int = 0, min_cover: int = 1, max_cands: int = 4, strands: str = "forward"):
        """The read's candidate placements, best first: [(pos, cover, mask)] —
        the read would start at text position pos (negative: it overhangs the
        text's start), the seeds in `mask` (bit j: seed j of `seeds`) agree on
        it and cover `cover` of its symbols.  strands="both": a (forward,
        reverse) pair of such lists, the reverse one placing rc(pattern)."""
        nc, _, pos, cover, mask = self.place_batch([pattern], max_seeds, min_len, skip, max_occ, band, min_cover,
                                                   max_cands, strands=strands)
        res = [[(int(pos[v, k]), int(cover[v, k]), int(mask[v, k])) for k in range(int(nc[v]))]
               for v in range(nc.size)]
        return tuple(res) if strands == "both" else res[0]

    def place_batch(self, patterns, max_seeds: int = 8, min_len: int = 1, skip: int = 0, max_occ: int = 16,
                    band: int = 0, min_cover: int = 1, max_cands: int = 4, reversed: bool = False,
                    strands: str = "forward"):
        """Candidate placements of many reads (fmx_place_batch): (ncands
        uint32[n], flags uint32[n], pos int64[n, max_cands], cover uint32[n,
        max_cands], mask uint32[n, max_cands]); 2n rows under strands="both".
        The seeds of seeds_batch (max_seeds, min_len, skip; those with at most
        max_occ occurrences are located; max_seeds * max_occ <= 1024) vote:
        every occurrence x of seed j, covering p[e-L:e], says the read starts
        at d = x - (e - L); occurrences whose d lie within `band` of their
        neighbour's form a cluster with pos = its smallest d, mask = its seeds
        and cover = their summed lengths; the clusters with cover >= min_cover
        come by cover descending, then pos ascending, the first max_cands of
        them stored (flags & 2: there were more) and the unused entries zero.
        Only the reads go to the device and only the candidates come back."""
        data, offsets = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        reads, K = offsets.size - 1, int(max_cands)
        n = 2 * reads if strands == "both" else reads
        rows = max(n, 1) * max(K, 1)
        nc, fl = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        pos = np.zeros(rows, dtype=np.int64)
        cover, mask = np.zeros(rows, dtype=np.uint32), np.zeros(rows, dtype=np.uint32)
        flags = (_n.FMX_PATTERN_REVERSED if reversed else 0) | _strand_flags(strands)
        _check(_n.lib().fmx_place_batch(self._h, _ptr(data) if data.size else None, _ptr(offsets), reads, flags,
                                        int(max_seeds), int(min_len), int(skip), int(max_occ), int(band),
                                        int(min_cover), K, _ptr(nc), _ptr(fl), _ptr(pos), _ptr(cover), _ptr(mask)),
               "fmx_place_batch")
        return (nc[:n], fl[:n], pos[:n * K].reshape(n, K), cover[:n * K].reshape(n, K), mask[:n * K].reshape(n, K))

    # -- mapping reads: place, then align each candidate against the text (needs the text: OPT_VERIFY_TEXT) --
    def map(self, pattern: bytes, max_seeds: int = 8, min_len: int = 1, skip: int = 0, max_occ: int = 16,
            band: int = 0, min_cover: int = 1, max_cands: int = 4, align_band: int = 8,
            max_dist: Optional[int] = None, strands: str = "forward"):
        """The read's verified placements, in place()'s order: [(pos, cover,
        mask, dist, tstart, tend)] — the read aligns to text[tstart:tend] at
        `dist` unit-cost edits; dist is None (tstart = tend = 0) for a candidate
        with no alignment within align_band diagonals of pos and max_dist
        edits.  strands="both": a (forward, reverse) pair of such lists."""
        nc, _, pos, cover, mask, dist, ts, te = self.map_batch([pattern], max_seeds, min_len, skip, max_occ, band,
                                                               min_cover, max_cands, align_band, max_dist,
                                                               strands=strands)
        res = [[(int(pos[v, k]), int(cover[v, k]), int(mask[v, k]),
                 None if dist[v, k] == _n.FMX_VERIFY_NONE else int(dist[v, k]), int(ts[v, k]), int(te[v, k]))
                for k in range(int(nc[v]))] for v in range(nc.size)]
        return tuple(res) if strands == "both" else res[0]

    def map_batch(self, patterns, max_seeds: int = 8, min_len: int = 1, skip: int = 0, max_occ: int = 16,
                  band: int = 0, min_cover: int = 1, max_cands: int = 4, align_band: int = 8,
                  max_dist: Optional[int] = None, reversed: bool = False, strands: str = "forward"):
        """place_batch, then every candidate aligned against the text on the
        device (fmx_map_batch): place_batch's five arrays, then dist
        uint32[n, max_cands], tstart, tend int64[n, max_cands].  Candidate k of
        read v aligns to text[tstart:tend] at dist edits (substitutions,
        insertions, deletions, 1 each), over the diagonals within align_band
        (0..31) of pos: the fewest edits, the earliest end among those, the
        shortest alignment to that end.  dist = 0xFFFFFFFF (tstart = tend = 0):
        no alignment within the band, or more than max_dist edits (None: any
        number), or a read longer than 65,535; unused entries are zero.  The
        index must hold the text: load it with options | OPT_VERIFY_TEXT."""
        data, offsets = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        reads, K = offsets.size - 1, int(max_cands)
        n = 2 * reads if strands == "both" else reads
        rows = max(n, 1) * max(K, 1)
        nc, fl = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        pos, ts, te = (np.zeros(rows, dtype=np.int64) for _ in range(3))
        cover, mask, dist = (np.zeros(rows, dtype=np.uint32) for _ in range(3))
        flags = (_n.FMX_PATTERN_REVERSED if reversed else 0) | _strand_flags(strands)
        _check(_n.lib().fmx_map_batch(self._h, _ptr(data) if data.size else None, _ptr(offsets), reads, flags,
                                      int(max_seeds), int(min_len), int(skip), int(max_occ), int(band), int(min_cover),
                                      K, int(align_band), _n.FMX_VERIFY_NONE - 1 if max_dist is None else int(max_dist),
                                      _ptr(nc), _ptr(fl), _ptr(pos), _ptr(cover), _ptr(mask), _ptr(dist), _ptr(ts),
                                      _ptr(te)), "fmx_map_batch")
        return (nc[:n], fl[:n]) + tuple(a[:n * K].reshape(n, K) for a in (pos, cover, mask, dist, ts, te))

    # -- device-resident API (pointers are ints; stream is a hipStream_t) --
    def count_batch_async(self, d_bytes: int, d_offsets: int, n: int, d_counts: int,
                          stream: int = 0, reversed: bool = False, long_patterns: bool = False, stage_kb: int = 0,
                          fixed_len: int = 0) -> None:
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len)
        _check(_n.lib().fmx_count_batch_async(self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n, flags,
                                              C.c_void_p(d_counts), C.c_void_p(stream) if stream else None))

    def locate_workspace_size(self, n: int) -> int:
        b = C.c_uint64()
        _check(_n.lib().fmx_locate_workspace_size(self._h, n, C.byref(b)))
        return b.value

    def locate_batch_async(self, d_bytes: int, d_offsets: int, n: int, d_loc_offsets: int,
                           d_locs: int, cap: int, d_needed: int, d_ws: int, ws_bytes: int,
                           d_counts: int = 0, stream: int = 0, reversed: bool = False,
                           long_patterns: bool = False, stage_kb: int = 0, fixed_len: int = 0) -> None:
        """`long_patterns`: FMX_HINT_LONG_PATTERNS (patterns average > 64 bytes);
        `fixed_len`: FMX_HINT_FIXED_LEN (checked on the device: FMX_E_ARG at sync)."""
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len)
        _check(_n.lib().fmx_locate_batch_async(
            self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n, flags,
            C.c_void_p(d_counts) if d_counts else None, C.c_void_p(d_loc_offsets), C.c_void_p(d_locs), cap,
            C.c_void_p(d_needed) if d_needed else None, C.c_void_p(d_ws), ws_bytes,
            C.c_void_p(stream) if stream else None))

    def match_batch_async(self, d_bytes: int, d_offsets: int, n: int, d_lens: int, d_ranges: int,
                          d_loc_offsets: int = 0, d_locs: int = 0, cap: int = 0, d_needed: int = 0, d_ws: int = 0,
                          ws_bytes: int = 0, min_len: int = 1, max_occ: Optional[int] = None, stream: int = 0,
                          reversed: bool = False, long_patterns: bool = False, stage_kb: int = 0,
                          fixed_len: int = 0, strands: str = "forward") -> None:
        """(strands="both", here and in the next two: n reads, every size below
        with 2 n for n.)
        fmx_match_batch_async: d_lens uint32[n], d_ranges P[2 n]; with
        d_loc_offsets (uint64[n+1]) also the locations of the reporting
        patterns, into d_locs (cap entries) with the total in d_needed, over a
        workspace of locate_workspace_size(n) bytes; d_loc_offsets = 0:
        lengths and intervals only, no workspace."""
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len) | _strand_flags(strands)
        _check(_n.lib().fmx_match_batch_async(
            self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n, flags, int(min_len),
            (1 << 64) - 1 if max_occ is None else int(max_occ), C.c_void_p(d_lens), C.c_void_p(d_ranges),
            _vp(d_loc_offsets), _vp(d_locs), cap, _vp(d_needed), _vp(d_ws), ws_bytes, _vp(stream)))

    def seeds_batch_async(self, d_bytes: int, d_offsets: int, n: int, d_nseeds: int, d_rest: int, d_spans: int,
                          d_ranges: int, d_loc_offsets: int = 0, d_locs: int = 0, cap: int = 0, d_needed: int = 0,
                          d_ws: int = 0, ws_bytes: int = 0, max_seeds: int = 8, min_len: int = 1, skip: int = 0,
                          max_occ: Optional[int] = None, stream: int = 0, reversed: bool = False,
                          long_patterns: bool = False, stage_kb: int = 0, fixed_len: int = 0,
                          strands: str = "forward") -> None:
        """fmx_seeds_batch_async: d_nseeds, d_rest uint32[n], d_spans uint32[2 n
        max_seeds], d_ranges P[2 n max_seeds]; with d_loc_offsets (uint64[n
        max_seeds + 1]) also the locations of the reporting seeds, into d_locs
        (cap entries) with the total in d_needed, over a workspace of
        locate_workspace_size(n * max_seeds) bytes; d_loc_offsets = 0: spans
        and intervals only, no workspace."""
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len) | _strand_flags(strands)
        _check(_n.lib().fmx_seeds_batch_async(
            self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n, flags, int(max_seeds), int(min_len), int(skip),
            (1 << 64) - 1 if max_occ is None else int(max_occ), _vp(d_nseeds), _vp(d_rest), _vp(d_spans), _vp(d_ranges),
            _vp(d_loc_offsets), _vp(d_locs), cap, _vp(d_needed), _vp(d_ws), ws_bytes, _vp(stream)))

    def approx_batch_async(self, d_bytes: int, d_offsets: int, n: int, d_nhits: int, d_more: int, d_mm: int,
                           d_subs: int, d_ranges: int, d_loc_offsets: int = 0, d_locs: int = 0, cap: int = 0,
                           d_needed: int = 0, d_ws: int = 0, ws_bytes: int = 0, max_mm: int = 1, max_hits: int = 8,
                           best: bool = False, max_occ: Optional[int] = None, stream: int = 0, reversed: bool = False,
                           long_patterns: bool = False, stage_kb: int = 0, fixed_len: int = 0,
                           strands: str = "forward") -> None:
        """fmx_approx_batch_async: d_nhits, d_more uint32[n], d_mm uint32[n
        max_hits], d_subs uint32[6 n max_hits], d_ranges P[2 n max_hits]; with
        d_loc_offsets (uint64[n max_hits + 1]) also the locations of the
        reporting hits, into d_locs (cap entries) with the total in d_needed,
        over a workspace of locate_workspace_size(n * max_hits) bytes;
        d_loc_offsets = 0: intervals only, no workspace."""
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len) | _strand_flags(strands)
        _check(_n.lib().fmx_approx_batch_async(
            self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n, flags, int(max_mm), int(max_hits),
            _n.FMX_APPROX_BEST if best else 0, (1 << 64) - 1 if max_occ is None else int(max_occ), _vp(d_nhits),
            _vp(d_more), _vp(d_mm), _vp(d_subs), _vp(d_ranges), _vp(d_loc_offsets), _vp(d_locs), cap, _vp(d_needed),
            _vp(d_ws), ws_bytes, _vp(stream)))

    def vote_async(self, n_chains: int, max_seeds: int, d_nseeds: int, d_spans: int, d_loc_offsets: int, d_locs: int,
                   cap: int, d_ncands: int, d_flags: int, d_pos: int, d_cover: int, d_mask: int, band: int = 0,
                   min_cover: int = 1, max_cands: int = 4, stream: int = 0) -> None:
        """fmx_vote_async over what seeds_batch_async (with locations, `cap`
        its capacity) left for n_chains patterns — 2n under strands="both" —
        at max_seeds slots each: d_ncands, d_flags uint32[n_chains], d_pos
        int64[n_chains max_cands], d_cover, d_mask uint32[n_chains max_cands]
        (place_batch describes them).  A chain with more than 1,024
        occurrences, or whose locations reach past cap: no candidates, flags =
        1.  No workspace; on the same stream as the seeds launch no
        synchronisation is needed in between."""
        _check(_n.lib().fmx_vote_async(
            self._h, n_chains, int(max_seeds), _vp(d_nseeds), _vp(d_spans), _vp(d_loc_offsets), _vp(d_locs), cap,
            int(band), int(min_cover), int(max_cands), _vp(d_ncands), _vp(d_flags), _vp(d_pos), _vp(d_cover),
            _vp(d_mask), _vp(stream)))

    def verify_async(self, d_bytes: int, d_offsets: int, n: int, d_ncands: int, d_pos: int, d_dist: int,
                     d_tstart: int, d_tend: int, max_cands: int = 4, band: int = 8, max_dist: Optional[int] = None,
                     stream: int = 0, reversed: bool = False, long_patterns: bool = False, stage_kb: int = 0,
                     fixed_len: int = 0, strands: str = "forward") -> None:
        """fmx_verify_async: the reads as seeds_batch_async takes them (the
        staging hints are ignored) and what vote_async left for their chains —
        2n under strands="both" — at max_cands: d_ncands uint32[n], d_pos
        int64[n max_cands]; d_dist uint32[n max_cands], d_tstart, d_tend
        int64[n max_cands] (map_batch describes them).  No workspace; on the
        same stream as the vote no synchronisation is needed in between."""
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len) | _strand_flags(strands)
        _check(_n.lib().fmx_verify_async(
            self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n, flags, int(max_cands), _vp(d_ncands), _vp(d_pos),
            int(band), _n.FMX_VERIFY_NONE - 1 if max_dist is None else int(max_dist), _vp(d_dist), _vp(d_tstart),
            _vp(d_tend), _vp(stream)))

    @staticmethod
    def locate_job(d_bytes: int, d_offsets: int, n: int, d_loc_offsets: int, d_locs: int, cap: int,
                   d_needed: int, d_ws: int, ws_bytes: int, d_counts: int = 0, stream: int = 0,
                   reversed: bool = False, long_patterns: bool = False, stage_kb: int = 0,
                   fixed_len: int = 0) -> "_n.fmx_locate_job":
        """One entry of a locate queue (fmx_locate_job): the arguments of
        locate_batch_async."""
        flags = _flags(reversed, long_patterns, stage_kb, fixed_len)
        return _n.fmx_locate_job(d_bytes, d_offsets, n, flags, 0, d_counts or None, d_loc_offsets, d_locs, cap,
                                 d_needed, d_ws, ws_bytes, stream or None)

    @staticmethod
    def job_queue(jobs) -> "C.Array":
        """A ctypes array of jobs, built once and submitted many times."""
        return (_n.fmx_locate_job * len(jobs))(*jobs)

    def locate_jobs_async(self, queue) -> None:
        """Issue a queue of locate batches in one native call
        (fmx_locate_jobs_async): no per-batch Python overhead."""
        _check(_n.lib().fmx_locate_jobs_async(self._h, queue, len(queue)))

    def locate_group_async(self, queue, stream: int = 0) -> None:
        """Run a queue of locate batches together, up to 256 per kernel launch,
        on `stream` (fmx_locate_group_async); distinct workspaces and outputs."""
        _check(_n.lib().fmx_locate_group_async(self._h, queue, len(queue), C.c_void_p(stream) if stream else None))

    def sync(self, stream: int = 0) -> None:
        _check(_n.lib().fmx_sync(self._h, C.c_void_p(stream) if stream else None))

    def release_stream(self, stream: int) -> None:
        """Done with `stream`: wait for it, raise what it latched (as sync),
        free its status word (fmx_stream_release)."""
        _check(_n.lib().fmx_stream_release(self._h, C.c_void_p(stream) if stream else None))

    def timing_enable(self, on: bool = True, every: int = 1) -> None:
        """Bracket every `every`-th launch with HIP events (fmx_timing_enable)."""
        _check(_n.lib().fmx_timing_enable(self._h, max(1, int(every)) if on else 0))

    def timing_read(self) -> dict:
        arr = (_n.fmx_kernel_timing * 16)()
        cnt = C.c_int()
        _check(_n.lib().fmx_timing_read(self._h, arr, 16, C.byref(cnt)))
        return {arr[i].name.decode(): {"launches": arr[i].launches, "total_ms": arr[i].total_ms,
                                       "units": arr[i].units} for i in range(min(cnt.value, 16))}


# ------------------------------------------------------- MultiDeviceIndex

class MultiDeviceIndex:
    """One index over several GPUs of this process (fmx_multi_*): a replica
    per entry of `devices` (the blob copied host -> devices[0] once, then
    device to device), batches cut into contiguous shards answered
    concurrently and concatenated — the same answers as `FmIndex` on one
    device, for a single-process caller with no process group."""

    def __init__(self, blob, devices: Sequence[int], position: Position = u32, block: Optional[_Block] = None,
                 text_encoder=text_encoders.EncodingTable, options: int = _n.FMX_OPT_DEFAULT):
        devs = (C.c_int * len(devices))(*devices)
        h = _load("fmx_multi_load",
                  lambda layout, arr, *out: _n.lib().fmx_multi_load(_ptr(arr), arr.size, layout, devs, len(devices),
                                                                    options, *out),
                  position, block, text_encoder, blob=blob)[0]
        self._h = h
        self._dt = position.dtype
        self.devices = list(devices)

    @property
    def replicas(self) -> int:
        return _n.lib().fmx_multi_replicas(self._h)

    def close(self):
        if self._h:
            _n.lib().fmx_multi_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count_batch(self, patterns, reversed: bool = False) -> np.ndarray:
        data, offsets = patterns if isinstance(patterns, tuple) else pack_patterns(patterns)
        n = offsets.size - 1
        out = np.zeros(max(n, 1), dtype=self._dt)
        flags = _n.FMX_PATTERN_REVERSED if reversed else 0
        _check(_n.lib().fmx_multi_count_batch(self._h, _ptr(data) if data.size else None, _ptr(offsets), n, flags,
                                              _ptr(out)), "fmx_multi_count_batch")
        return out[:n]

    def locate_batch(self, patterns, reversed: bool = False,
                     cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        return _host_query("fmx_multi_locate_batch", self._h, self._dt, patterns, reversed,
                           cap=(1 << 16) if cap is None else cap)[2:]


# ---------------------------------------------------------- FmIndexBuilder

class FmIndexBuilder:
    """``FmIndexBuilder<P, B, E>`` (builder/mod.rs:17-264); ``build`` runs on the GPU."""

    def __init__(self, text_len: int, symbol_count: int, text_encoder, position: Position = u32,
                 block: Optional[_Block] = None, lookup_table_config=None, suffix_array_config=None):
        self.block = block or blocks.Block2(Vector.U64)
        if symbol_count > self.block.MAX_SYMBOL:
            raise SymbolCountOver(self.block.MAX_SYMBOL, symbol_count)
        self.text_len = text_len
        self.symbol_count = symbol_count
        self.text_encoder = text_encoder
        self.position = position
        self.lookup_table_config = lookup_table_config or build_config.LookupTableConfig.None_()
        self.suffix_array_config = suffix_array_config or build_config.SuffixArrayConfig.Uncompressed()
        self.kmer_size = self.lookup_table_config.kmer_size(position, symbol_count)
        self.sampling_ratio = self.suffix_array_config.sampling_ratio()

    @classmethod
    def new(cls, text_len, symbol_count, text_encoder, position=u32, block=None):
        return cls(text_len, symbol_count, text_encoder, position, block)

    def set_lookup_table_config(self, config) -> "FmIndexBuilder":
        return FmIndexBuilder(self.text_len, self.symbol_count, self.text_encoder, self.position, self.block,
                              config, self.suffix_array_config)

    def set_suffix_array_config(self, config) -> "FmIndexBuilder":
        return FmIndexBuilder(self.text_len, self.symbol_count, self.text_encoder, self.position, self.block,
                              self.lookup_table_config, config)

    def _layout(self):
        return _layout(self.position, self.block, self.text_encoder)

    def blob_size(self) -> int:
        out = C.c_uint64()
        st = _n.lib().fmx_build_blob_size(self.text_len, self.symbol_count, self._layout(), self.kmer_size,
                                          self.sampling_ratio, C.byref(out))
        if st == _n.FMX_E_CONFIG:
            raise InvalidConfig("unsupported configuration")
        _check(st)
        return out.value

    def build(self, text, blob: np.ndarray, device: int = 0) -> None:
        """``FmIndexBuilder::build`` (builder/mod.rs:187-264) on `device`."""
        t = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
        if t.size != self.text_len:
            raise UnmatchedTextLength(self.text_len, t.size)
        if blob.ctypes.data % self.block.ALIGN_SIZE:
            raise NotAlignedBlob(self.block.ALIGN_SIZE, blob.ctypes.data % self.block.ALIGN_SIZE)
        size = self.blob_size()
        if blob.size != size:
            raise InvalidBlobSize(size, blob.size)
        table = self.text_encoder.table
        tb = None if table is None else C.create_string_buffer(table, 256)
        st = _n.lib().fmx_build(_ptr(t) if t.size else None, t.size, tb, self.symbol_count, self._layout(),
                                self.kmer_size, self.sampling_ratio, _ptr(blob), blob.size, device)
        if st == _n.FMX_E_SYMBOL:
            raise FmxError(st, "text symbol index >= symbol_count")
        _check(st, "fmx_build")

    def build_device(self, d_text: int, d_blob: int, blob_len: int, device: int = 0) -> None:
        """Build from a text already in HBM into a device blob."""
        table = self.text_encoder.table
        tb = None if table is None else C.create_string_buffer(table, 256)
        _check(_n.lib().fmx_build_device(C.c_void_p(d_text), self.text_len, tb, self.symbol_count,
                                         self._layout(), self.kmer_size, self.sampling_ratio,
                                         C.c_void_p(d_blob), blob_len, device), "fmx_build_device")
