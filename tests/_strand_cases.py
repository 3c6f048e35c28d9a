"""Both strands (FMX_PATTERN_REVCOMP, FMX_BOTH_STRANDS on fmx_match_batch,
fmx_seeds_batch and fmx_approx_batch): the cases, expected values and runs the
emulator tests (test_strands_simt.py, test_strands_guard_simt.py) and the GPU
tests (test_gpu_strands.py, test_gpu_strands_guard.py) share.

The contract (include/fmx.h): with rc(p)[j] = map[p[m-1-j]], a strand call
returns what the flag-less call returns for the EXPANDED batch — rc(p_0), ...
under FMX_PATTERN_REVCOMP, p_0, rc(p_0), p_1, rc(p_1), ... under
FMX_BOTH_STRANDS.  So the expected values are the existing references run on
the expanded list, which is built here in Python (expand): _match_cases.Case.
expected, _seed_cases.expected_arrays and the brute force of _approx_cases.  In
addition (never instead) the strand call is compared with the engine's own
flag-less call on the expanded list.

Maps: a random involution over the text's alphabet (an odd character and every
byte outside the alphabet, ABSENT among them, map to themselves), and a
3-cycle a -> b -> c -> a, which no involution is: it shows the map applied
exactly once.

Reads: text substrings alternating with reads whose rc is a text substring (so
strand 1 truly matches), then the substituted and absent-byte classes of
_match_cases.Case.core().  assert_classes checks on the reference alone that
both strands hold whole matches and partial ones.

stage_bytes_of / staged_tiles restate, from the offsets alone, which tiles a
launch stages under its hints; run_device and the flag-less runners assert a
caller's expectation of that (tiles=) for the reads of tests/_long_cases.py.
"""
import numpy as np

import _approx_cases as AC
import _seed_cases as SC
from _guard_cases import FILL_OUT, Arena
from _match_cases import ABSENT
from _util import SIMT_LAYOUTS as LAYOUTS  # noqa: F401

QUERIES = ("match", "seeds", "approx")
PER = 3  # max_seeds / max_hits: a 256-slot tile straddles the 128-read tile edge
BOTH_SIZES = (1, 127, 128, 129, 300)
RC_SIZES = (1, 255, 256, 257)
FIXED_M = 24
KW = {"match": dict(min_len=1, max_occ=None),
      "seeds": dict(max_seeds=PER, min_len=1, skip=0, max_occ=None),
      "approx": dict(max_mm=1, max_hits=PER, best=False, max_occ=None)}


def kw_for(query, **over):
    kw = dict(KW[query])
    kw.update(over)
    return kw


def per_of(query, kw):
    return {"match": 1, "seeds": kw.get("max_seeds"), "approx": kw.get("max_hits")}[query]


# -------------------------------------------------------------------- the maps

def involution(case):
    """A random pairing of case.chars; the odd one out and every other byte map to themselves."""
    rng = np.random.default_rng(case.seed + 4242)
    chars = [int(c) for c in rng.permutation(np.frombuffer(case.chars, np.uint8))]
    m = bytearray(range(256))
    for a, b in zip(chars[0::2], chars[1::2]):
        m[a], m[b] = b, a
    assert m[ABSENT] == ABSENT and all(m[m[b]] == b for b in range(256))
    return bytes(m)


def cycle_map(case):
    """a -> b -> c -> a over the first three characters: not an involution."""
    a, b, c = case.chars[:3]
    m = bytearray(range(256))
    m[a], m[b], m[c] = b, c, a
    return bytes(m)


def rc(p, cmap):
    return bytes(cmap[b] for b in reversed(p))


def unrc(q, cmap):
    """The read p with rc(p) = q (cmap a permutation)."""
    inv = bytearray(256)
    for b in range(256):
        inv[cmap[b]] = b
    return bytes(inv[b] for b in reversed(q))


def expand(reads, cmap, strands):
    if strands == "reverse":
        return [rc(p, cmap) for p in reads]
    assert strands == "both"
    return [q for p in reads for q in (p, rc(p, cmap))]


# ------------------------------------------------------------------- the reads

_READS = {}


def reads_for(case, cmap, n, fixed=False):
    """n reads: text substrings and reads whose rc is one in turn (12..40
    symbols, 24..40 over a two-letter alphabet, where a random 12-mer is likely
    to occur; FIXED_M each when `fixed`), then — ragged batches — the classes
    of Case.core() with a substituted or an absent byte."""
    key = (id(case), cmap, n, fixed)
    got = _READS.get(key)
    if got is not None:
        return got
    rng = np.random.default_rng(case.seed + 31 * n + fixed)
    t = case.text
    lo = 12 if len(case.chars) >= 3 else 24

    def sub():
        m = FIXED_M if fixed else int(rng.integers(lo, 41))
        s = int(rng.integers(0, len(t) - m))
        return t[s:s + m]
    # (substituted, absent bytes, the empty pattern)
    core = [] if fixed else [p for p in case.core() if not p or p not in t]
    n_alt = n if n == 1 else min(n, max(96, n - len(core)))
    out = [sub() if i % 2 == 0 else unrc(sub(), cmap) for i in range(n_alt)]
    if n == 1:
        out = [unrc(sub(), cmap)]
    for i in range(n - len(out)):
        if core:
            out.append(core[i % len(core)])
        else:  # fixed length: a substring or the rc of one with one substitution
            q = bytearray(out[i])
            j = int(rng.integers(0, len(q)))
            q[j] = case.other(rng, q[j])
            out.append(bytes(q))
    _READS[key] = out
    return out


def assert_classes(case, orc, reads, cmap):
    """On the reference alone (batches of at least 128 reads): each strand has
    at least 30 whole matches of 12 symbols or more and 30 partial ones."""
    if len(reads) < 128:
        return
    for s in (0, 1):
        pats = [rc(p, cmap) if s else p for p in reads]
        L = np.array([case.expected(orc, p)[0] for p in pats])
        m = np.array([len(p) for p in pats])
        whole, part = int(((L == m) & (m >= 12)).sum()), int(((L > 0) & (L < m)).sum())
        assert whole >= 30 and part >= 30, f"strand {s}: {whole} whole matches, {part} partial ones"


# -------------------------------------------------------- the expected values

def match_expected_arrays(case, orc, pats, min_len, max_occ):
    """lens, ranges, loc_offsets, locations from Case.expected (as check_match reads it)."""
    exp = [case.expected(orc, p) for p in pats]
    lens = np.array([e[0] for e in exp], np.int64)
    rng = np.array([[e[1], e[2]] for e in exp], np.int64).reshape(len(pats), 2)
    need = max(min_len, 1)
    rep = [e[0] >= need and (max_occ is None or e[2] - e[1] <= max_occ) for e in exp]
    cnt = np.array([e[2] - e[1] if r else 0 for e, r in zip(exp, rep)], np.uint64)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
    locs = [x for e, r in zip(exp, rep) if r for x in e[3]]
    return lens, rng, off, np.array(locs, dtype=np.uint64)


def expected(query, case, orc, vpats, kw):
    """The flag-less call's outputs for the (expanded) list vpats: the query's
    own arrays, then loc_offsets and locations."""
    if query == "match":
        return match_expected_arrays(case, orc, vpats, kw["min_len"], kw["max_occ"])
    if query == "seeds":
        return SC.expected_arrays(case, orc, vpats, kw["max_seeds"], kw["min_len"], kw["skip"], kw["max_occ"])
    return AC.expected_arrays(case, orc, vpats, kw["max_mm"], kw["max_hits"], kw["best"], kw["max_occ"])


def host_call(ix, query, pats, kw, strands="forward", reversed=False, locate=True):
    q = [p[::-1] for p in pats] if reversed else pats
    return getattr(ix, query + "_batch")(q, reversed=reversed, locate=locate, strands=strands, **kw)


def compare(what, got, exp, locate=True):
    """Every output array against the expected one: shape and every element."""
    n_own = len(exp) - 2
    assert len(got) == n_own + (2 if locate else 0), what
    for j in range(n_own + (2 if locate else 0)):
        g, e = np.asarray(got[j]), np.asarray(exp[j])
        assert g.shape == e.shape, (what, j, g.shape, e.shape)
        bad = np.argwhere(g.astype(np.int64) != e.astype(np.int64))
        assert bad.size == 0, (f"{what}: output {j} differs at {len(bad)} places, first {bad[:4].tolist()}: "
                               f"{[int(g[tuple(b)]) for b in bad[:4]]} expected {[int(e[tuple(b)]) for b in bad[:4]]}")


def check(ix, orc, case, query, reads, cmap, strands, reversed=False, locate=True, **over):
    """The strand call of `reads` (host buffers) against the reference on the
    expanded list, then against the engine's own flag-less call on it."""
    kw = kw_for(query, **over)
    what = f"{query} strands={strands} n={len(reads)} rev={reversed} locate={locate} {over}"
    assert_classes(case, orc, reads, cmap)
    vpats = expand(reads, cmap, strands)
    exp = expected(query, case, orc, vpats, kw)
    got = host_call(ix, query, reads, kw, strands, reversed, locate)
    compare(what, got, exp, locate)
    own = host_call(ix, query, vpats, kw, "forward", reversed, locate)
    for j, (g, o) in enumerate(zip(got, own)):
        assert g.dtype == o.dtype and np.array_equal(g, o), f"{what}: output {j} differs from the flag-less call"
    return exp, got


# ------------------------------------------------------- the device-buffer run

# per query: (buffer, bytes per unit, counted in slots) in the order of the async call's arguments
OUTS = {"match": (("lens", 4, False), ("ranges", None, False)),
        "seeds": (("nseeds", 4, False), ("rest", 4, False), ("spans", 8, True), ("ranges", None, True)),
        "approx": (("nhits", 4, False), ("more", 4, False), ("mm", 4, True), ("subs", 24, True),
                   ("ranges", None, True))}


def stage_kb_both(reads, strands):
    """FMX_HINT_STAGE_KB that stages every tile: both copies of a 128-read tile, or one of a 256-read tile."""
    tile, copies = (128, 2) if strands == "both" else (256, 1)
    most = max(copies * sum(len(p) for p in reads[t:t + tile]) for t in range(0, len(reads), tile))
    return min(max(-(-most // 1024), 1), 56)


def stage_bytes_of(strands="forward", stage_kb=0, fixed_len=0, long_patterns=False):
    """The stage of a slot-query launch by the rules of include/fmx.h: the
    FMX_HINT_STAGE_KB hint (at most 56 KB), else 56 KB with
    FMX_HINT_LONG_PATTERNS, else 16 KB; a strand launch with FMX_HINT_FIXED_LEN
    asks for no more than its tile spans (256 m bytes, rounded up to 16)."""
    sb = min(stage_kb, 56) * 1024 if stage_kb else 56 * 1024 if long_patterns else 16 * 1024
    if strands != "forward" and fixed_len:
        sb = min(sb, -(-256 * fixed_len // 16) * 16)
    return sb


def staged_tiles(reads, strands="forward", stage_kb=0, fixed_len=0, long_patterns=False):
    """Per tile (256 reads, 128 under "both"), from the offsets alone: whether
    its span (both copies under "both") fits the launch's stage."""
    tile, copies = (128, 2) if strands == "both" else (256, 1)
    sb = stage_bytes_of(strands, stage_kb, fixed_len, long_patterns)
    return [copies * sum(len(p) for p in reads[t:t + tile]) <= sb for t in range(0, len(reads), tile)]


def run_device(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, reversed=False, locate=True,
               cap_name="total", skew=1, stage_kb=None, fixed_len=0, long_patterns=False, tiles=None, **over):
    """The _async call with every buffer carved at its exact (2n-shaped) size
    and weakest alignment out of one guard-filled allocation (_guard_cases.
    Arena): the pattern bytes at `skew`, flush against the end guard, 4-B
    arrays 4 B past a 16-B boundary, P-wide ones P bytes, the workspace 16 B
    past a 256-B boundary.  After the launch: every guard byte intact, the
    inputs unchanged, every output the expected value, *d_needed exact and
    d_locs[min(cap, total):cap] still the prefill.  stage_kb: None = the hint
    that stages every tile; 1 = no full tile fits (the raw path).  tiles: the
    caller's list of which tiles are staged (True) and which raw, asserted
    against staged_tiles() in place of that check of an explicit stage_kb (0 =
    no hint); long_patterns: FMX_HINT_LONG_PATTERNS."""
    kw = kw_for(query, **over)
    n = len(reads)
    vpats = expand(reads, cmap, strands)
    nv, per = len(vpats), per_of(query, kw)
    S = nv * per
    exp = expected(query, case, orc, vpats, kw)
    total = int(exp[-2][-1])
    cap = {"total": total, "total-1": total - 1, "zero-null": 0}[cap_name] if locate else 0
    if cap < 0:
        return
    hinted = stage_kb is not None
    if not hinted:
        stage_kb = stage_kb_both(reads, strands)
    if tiles is not None:
        got = staged_tiles(reads, strands, stage_kb, fixed_len, long_patterns)
        assert got == list(tiles), f"tiles staged by their offsets: {got}, expected {list(tiles)}"
    elif hinted and n >= (128 if strands == "both" else 256):
        tile, copies = (128, 2) if strands == "both" else (256, 1)
        assert copies * sum(len(p) for p in reads[:tile]) > 1024 * stage_kb, "the first tile fits: not the raw path"
    what = (f"{query} strands={strands} n={n} cap={cap_name}({cap}) skew={skew} rev={reversed} locate={locate} "
            f"stage_kb={stage_kb} fixed_len={fixed_len} {over}")
    P = np.uint32 if pb == 4 else np.uint64
    data, offsets = pkg.pack_patterns([p[::-1] for p in reads] if reversed else reads)
    arena = Arena(mem_cls)
    c = arena.carve
    if locate:
        wsb = ix.locate_workspace_size(S)
        c("ws", wsb, 16, 16, boundary=256)
    c("offsets", 8 * (n + 1), 8, 8, data=offsets)
    if locate:
        c("loc_offsets", 8 * (S + 1), 8, 8)
        c("needed", 8, 8, 8)
        if cap:
            c("locs", pb * cap, pb, pb, tail=pb * max(total - cap, 0))
    for name, unit, slots in OUTS[query]:
        unit, al = (2 * pb, pb) if unit is None else (unit, 4)
        c(name, unit * (S if slots else nv), al, al)
    c("bytes", data.size, 1, skew if data.size else 0, data=data)
    arena.commit()
    off, nb = arena.bufs["bytes"]
    assert off + nb == arena.size - 4096, "the last pattern byte is not the byte before the end guard"
    p = arena.ptr
    args = [p("bytes"), p("offsets"), n] + [p(name) for name, _, _ in OUTS[query]]
    if locate:
        args += [p("loc_offsets"), p("locs"), cap, p("needed"), p("ws"), wsb]
    getattr(ix, query + "_batch_async")(*args, reversed=reversed, stage_kb=stage_kb, fixed_len=fixed_len,
                                        long_patterns=long_patterns, strands=strands, **kw)
    ix.sync()
    arena.image()
    arena.check_guards_and_inputs(what)
    v = arena.view
    for j, (name, unit, _) in enumerate(OUTS[query]):
        g = v(name, P if unit is None else np.uint32).astype(np.int64)
        assert np.array_equal(g, np.asarray(exp[j]).astype(np.int64).reshape(-1)), f"{what}: d_{name}"
    if not locate:
        return
    assert np.array_equal(v("loc_offsets", np.uint64), exp[-2]), f"{what}: d_loc_offsets"
    assert int(v("needed", np.uint64)[0]) == total, f"{what}: *d_needed"
    if cap:
        k = min(cap, total)
        assert np.array_equal(v("locs", P)[:k].astype(np.uint64), exp[-1][:k]), f"{what}: d_locs[:min(cap, total)]"
        assert (v("locs", np.uint8)[k * pb:] == FILL_OUT).all(), f"{what}: d_locs written past min(cap, total)"


# ------------------------------------------------------------ the guard-band runs

SKEWS = (0, 1, 7, 15)
CAPS = ("total", "total-1", "zero-null")
GUARD_LAYOUTS = [(4, 3, 64), (8, 5, 128)]
GUARD_SHAPES = (("both", 1), ("both", 129), ("both", 300), ("reverse", 1), ("reverse", 257))
FILTERS = {"match": dict(min_len=2, max_occ=3), "seeds": dict(min_len=2, skip=1, max_occ=3),
           "approx": dict(max_occ=3)}


def guard_runs(pkg, O, mem_cls, query, pb, planes, vb, skew):
    """The guard-band runs of one query on one layout at one skew of the pattern bytes."""
    case = SC.case_for(planes)
    cmap = involution(case)
    ix, orc = SC.open_index(pkg, O, case, pb, planes, vb, 1)
    ix.set_complement(cmap)
    for j, (strands, n) in enumerate(GUARD_SHAPES):
        reads = reads_for(case, cmap, n)
        run = lambda **kw: run_device(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, skew=skew,  # noqa
                                      **FILTERS[query], **kw)
        for ci, cap in enumerate(CAPS):
            run(cap_name=cap, reversed=(j + ci + skew) % 2 == 1)
        run(locate=False, reversed=(j + skew) % 2 == 0)
        if n > 128:  # the reads read from HBM (no full tile fits a 1 KB stage), both directions
            for rev in (False, True):
                run(reversed=rev, stage_kb=1)
    ix.close()
