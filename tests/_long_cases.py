"""Reads of mapper length (100 to 300 symbols, and 65,535 / 65,536) through
fmx_match_batch, fmx_seeds_batch, fmx_approx_batch and the strand flags: the
texts, reads, class floors and runs that the emulator tests
(test_long_simt.py) and the GPU tests (test_gpu_long.py) share.

Nothing here is a reference of its own.  Every answer is compared with the
existing ones — _match_cases.Case.expected, _seed_cases.expected_arrays, the
brute force of _approx_cases, on the list _strand_cases.expand builds for a
strand call, which is also compared with the engine's flag-less call on that
list — and every device call goes through the existing guard-band runners
(_strand_cases.run_device, _seed_guard_cases.run_seeds, _approx_guard_cases.
run_approx, _guard_cases.run_match), given the reads and the hints.

Texts: the random text of _seed_cases.case_for (forced to 2,000 symbols where
it is shorter than 1,000), and RepeatCase: a random unit of 400 symbols copied
8 times, every symbol of every copy substituted with probability 0.003, so a
long read occurs in several rows and has several variants within one
substitution.

Reads (reads_for): one pool per (text, complement map, n, length), built from
what the text is and never from an answer.  F kinds are cut from the text, R
kinds are reads whose reverse complement is; each unsubstituted (150 symbols
or more in a ragged batch; on the repeat text two of three cut where the text
holds no substitution of its own) and with 1, 2 and 3 substitutions at random
positions (two or three: at least 13 symbols apart and from the ends, so that
every piece between them is a seed of min_len = 12); two-substring chimeras; a
read with ABSENT in the middle and one with ABSENT as its last byte; a read
alternating ABSENT and a text symbol (300 symbols in a ragged batch: 150
one-symbol seeds); the empty read in mid-batch (ragged batches).  The kinds are
dealt round-robin, so every tile holds every kind.  A batch of fewer than 256
reads is for FMX_BOTH_STRANDS only: its floors hold over the two strands
together, not over either alone.

assert_classes holds the floors, on the reference alone, before any engine
call."""
import numpy as np

import _approx_cases as AC
import _seed_cases as SC
import _strand_cases as S
from _approx_guard_cases import run_approx
from _guard_cases import run_match
from _match_cases import ABSENT, Case
from _seed_guard_cases import run_seeds
from _util import encode, rand_text

LENGTHS = (150, 224, 225, 300)
RAGGED = (100, 300)
MATCH = dict(min_len=12, max_occ=8)
SEEDS = dict(max_seeds=8, skip=1, min_len=12, max_occ=8)
SEEDS32 = dict(max_seeds=32, skip=0, min_len=1, max_occ=8)
APPROX = dict(max_mm=1, max_hits=3, best=False, max_occ=8)
APPROX_BEST = dict(APPROX, best=True)
APPROX_MM2 = dict(max_mm=2, max_hits=3, best=True, max_occ=8)
# (query, parameters): what a sweep runs on every batch
CONFIGS = (("match", MATCH), ("seeds", SEEDS), ("seeds", SEEDS32), ("approx", APPROX), ("approx", APPROX_BEST))


# -------------------------------------------------------------------- the texts

class RepeatCase(Case):
    """A random unit of `unit` symbols copied `copies` times; in each copy every
    symbol is substituted, independently, with probability p_sub by another
    symbol of the alphabet.  The alphabet, the wildcard symbol (absent from the
    text, as ABSENT is), k and sr follow the rules of Case."""

    def __init__(self, seed, nchars, unit=400, copies=8, p_sub=0.003, k=None, sr=None):
        super().__init__(seed, nchars, k=k, sr=sr)
        rng = np.random.default_rng(seed + 13)
        t = bytearray(rand_text(rng, self.chars, unit, unit) * copies)
        self.substituted = np.flatnonzero(rng.random(len(t)) < p_sub)
        for j in self.substituted:
            t[j] = self.other(rng, t[j])
        self.text = bytes(t)
        self.enc = encode(self.table, self.text)
        assert len(self.text) == unit * copies and set(self.text) == set(self.chars) and ABSENT not in self.text
        assert max(self.enc) == self.sigma - 2, "the wildcard symbol occurs in the text"

    def clean_window(self, rng, m):
        """A substring of m symbols that holds none of the text's own
        substitutions: a whole piece of the unit, so it occurs wherever another
        copy is as clean (chosen by how the text was built, not by an answer)."""
        while True:
            s = int(rng.integers(0, len(self.text) - m + 1))
            if not ((self.substituted >= s) & (self.substituted < s + m)).any():
                return self.text[s:s + m]


_REPEATS = {}


def random_case(planes):
    """case_for(planes), forced to 2,000 symbols where its text is shorter than 1,000."""
    case = SC.case_for(planes)
    return case if len(case.text) >= 1000 else SC.case_for(planes, n_text=2000)


def repeat_case(planes):
    if planes not in _REPEATS:
        _REPEATS[planes] = RepeatCase(planes * 11 + 3, min((1 << planes) - 1, 20))
    return _REPEATS[planes]


def two_letter_case():
    """W = 4 and 4^5 entries: a k-mer table of exactly 4,096 B with u32 positions."""
    return SC.case_for(2, two_letters=True, k=5, sr=2)


TEXTS = {"random": random_case, "repeat": repeat_case}


# -------------------------------------------------------------------- the reads

_READS = {}
KINDS = ("F0", "R0", "F1", "R1", "F2", "R2", "F3", "R3", "chimera")


def quotas(n):
    """How many reads of each kind a batch of n >= 128 holds.  From 256 reads on
    each family (F, R) alone holds 48 unsubstituted, more than 30 once-
    substituted and 30 twice- or thrice-substituted reads; below, the two
    families together do (30 + 30, 32 and 32: a FMX_BOTH_STRANDS batch).  The
    special reads take 4 (3 in a fixed-length batch), chimeras the rest."""
    if n >= 256:
        q = dict(F0=48, R0=48, F1=33, R1=33, F2=19, R2=19, F3=19, R3=19)
    else:
        q = dict(F0=30, R0=30, F1=16, R1=16, F2=8, R2=8, F3=8, R3=8)
    return q


def reads_for(case, cmap, n, m=None):
    """n >= 128 reads of m symbols each, or (m = None) of 100 to 300."""
    key = (id(case), cmap, n, m)
    got = _READS.get(key)
    if got is not None:
        return got
    assert n >= 128
    rng = np.random.default_rng(case.seed + 97 * n + (m or 0))
    t = case.text

    def length(lo=RAGGED[0]):
        return m if m else int(rng.integers(lo, RAGGED[1] + 1))

    def sub(mm):
        s = int(rng.integers(0, len(t) - mm + 1))
        return t[s:s + mm]

    def plant(p, nsub):
        q, mm = bytearray(p), len(p)
        if nsub == 1:
            where = [int(rng.integers(0, mm))]
        else:  # nsub positions at least 14 apart, the first and the last 13 or more from the ends
            slack = mm - 14 * (nsub - 1) - 27
            assert slack >= 0
            cuts = np.sort(rng.integers(0, slack + 1, size=nsub))
            where = [13 + int(c) + 14 * j for j, c in enumerate(cuts)]
        for j in where:
            q[j] = case.other(rng, q[j])
        return bytes(q)

    def make(kind):
        if kind == "chimera":
            mm = length()
            a = int(rng.integers(20, mm - 19))
            p = sub(a) + sub(mm - a)
            return p if rng.integers(0, 2) else S.unrc(p, cmap)
        nsub = int(kind[1])
        if nsub == 0:  # on the repeat text two of three from a stretch without a substitution of the text's own
            made[kind] = made.get(kind, 0) + 1
            clean = hasattr(case, "clean_window") and made[kind] % 3 != 0
            p = case.clean_window(rng, length(150)) if clean else sub(length(150))
        else:
            p = plant(sub(length()), nsub)
        return p if kind[0] == "F" else S.unrc(p, cmap)

    q, made = quotas(n), {}
    special = 3 if m else 4
    q["chimera"] = n - special - sum(q.values())
    assert q["chimera"] >= 1
    left, out = dict(q), []
    while any(left.values()):  # round-robin over the kinds that have reads left
        for kind in KINDS:
            if left[kind]:
                left[kind] -= 1
                out.append(make(kind))
    mm = m or RAGGED[1]
    mid = bytearray(sub(mm))
    mid[mm // 2] = ABSENT
    last = sub(mm - 1) + bytes([ABSENT])
    alt = bytearray(sub(mm))  # ABSENT and a text symbol in turn, the last byte a text symbol
    alt[mm - 2::-2] = bytes([ABSENT]) * len(alt[mm - 2::-2])
    out.insert(len(out) // 3, bytes(mid))
    out.insert(2 * len(out) // 3, last)
    out.append(bytes(alt))
    if not m:
        out.insert(len(out) // 2, b"")  # the empty read in mid-batch
    assert len(out) == n and (not m or all(len(p) == m for p in out))
    _READS[key] = out
    return out


def alt_read(reads):
    """Where the alternating read is: the last of the batch."""
    return len(reads) - 1


def expand(reads, cmap, strands):
    return list(reads) if strands == "forward" else S.expand(reads, cmap, strands)


# ------------------------------------------------------------------- the floors

_CLASSES = set()


def assert_classes(case, orc, reads, cmap, strands):
    """The floors, on the reference alone, over the list the call answers (the
    reads, their reverse complements, or both in turn):
      * 30 patterns match whole with 150 symbols or more, 30 have k < L < m;
      * seeds with skip = 1, min_len = 12, max_seeds = 8: 30 patterns have 3
        seeds or more and 30 exactly one; the alternating read of 300 symbols
        has 32 seeds and rest > 0 at max_seeds = 32;
      * each strand of the reads holds 30 whole matches and 30 partial ones
        (_strand_cases.assert_classes);
      * the repeat text, max_mm = 1: 30 patterns occur unsubstituted in two
        rows or more, 30 have 2 to 8 distinct variants, 30 have none and 30
        have d = 1 as their best stratum."""
    key = (id(case), id(reads), strands)
    if key in _CLASSES:
        return
    assert len(reads) >= 128
    vp = expand(reads, cmap, strands)
    exp = [case.expected(orc, p) for p in vp]
    m = np.array([len(p) for p in vp])
    L = np.array([e[0] for e in exp])
    whole, part = int(((L == m) & (m >= 150)).sum()), int(((L > case.k) & (L < m)).sum())
    assert whole >= 30 and part >= 30, f"{whole} whole matches of 150 symbols or more, {part} with k < L < m"
    ns = np.array([len(SC.chain(case, orc, p, 8, 12, 1)[0]) for p in vp])
    assert (ns >= 3).sum() >= 30 and (ns == 1).sum() >= 30, \
        f"{int((ns >= 3).sum())} patterns with 3 seeds or more, {int((ns == 1).sum())} with exactly one"
    alt = reads[alt_read(reads)]
    if len(alt) == 300 and strands != "reverse":
        assert alt[::2] == bytes([ABSENT]) * 150
        seeds, rest = SC.chain(case, orc, alt, 32, 1, 0)
        assert len(seeds) == 32 and rest > 0, (len(seeds), rest)
    S.assert_classes(case, orc, reads, cmap)
    if isinstance(case, RepeatCase):
        var = [AC.variants(case, orc, p, 1) for p in vp]
        nv = np.array([len(v) for v in var])
        twice = sum(1 for v in var if v and v[0][0] == 0 and v[0][3] - v[0][2] >= 2)
        d1 = sum(1 for v in var if v and v[0][0] == 1)
        few, none = int(((nv >= 2) & (nv <= 8)).sum()), int((nv == 0).sum())
        assert min(twice, few, none, d1) >= 30, \
            f"{twice} occur twice or more, {few} have 2-8 variants, {none} none, {d1} d = 1 as the best stratum"
    _CLASSES.add(key)


# -------------------------------------------------------------- the host calls

_EXPECTED = {}


def expected(query, case, orc, reads, cmap, strands, kw):
    """(the list the call answers, the reference's arrays for it): computed
    once per batch and configuration, shared by every test of the run and
    read-only."""
    key = (id(case), id(reads), strands, query, tuple(sorted(kw.items())))
    got = _EXPECTED.get(key)
    if got is None:
        vp = expand(reads, cmap, strands)
        exp = tuple(np.asarray(a) for a in S.expected(query, case, orc, vp, kw))
        for a in exp:
            a.setflags(write=False)
        got = _EXPECTED[key] = (vp, exp)
    return got


def check(ix, orc, case, query, reads, cmap, strands, reversed=False, locate=True, **kw):
    """One host call (it sets its own hints) against the reference on the list
    it answers; a strand call, as _strand_cases.check has it, also against the
    engine's flag-less call on that list.  Returns (expected, got)."""
    assert_classes(case, orc, reads, cmap, strands)
    kw = S.kw_for(query, **kw)
    what = f"{query} strands={strands} n={len(reads)} rev={reversed} locate={locate} {kw}"
    vp, exp = expected(query, case, orc, reads, cmap, strands, kw)
    got = S.host_call(ix, query, reads, kw, strands, reversed, locate)
    S.compare(what, got, exp, locate)
    if strands != "forward":
        own = S.host_call(ix, query, vp, kw, "forward", reversed, locate)
        for j, (g, o) in enumerate(zip(got, own)):
            assert g.dtype == o.dtype and np.array_equal(g, o), f"{what}: output {j} differs from the flag-less call"
    return exp, got


def open_index(pkg, O, case, cmap, pb, planes, vb, occ):
    ix, orc = SC.open_index(pkg, O, case, pb, planes, vb, occ)
    ix.set_complement(cmap)
    return ix, orc


# (strands, n) of the ragged sweep
SWEEP_SHAPES = (("forward", 300), ("reverse", 300), ("both", 129), ("both", 300))


def sweep(pkg, O, text, pb, planes, vb, occ, passes, shapes=SWEEP_SHAPES, configs=CONFIGS):
    """Case 1: the ragged batches from host calls, every configuration under
    every (reversed, locate) pair of `passes`."""
    case = TEXTS[text](planes)
    cmap = S.involution(case)
    ix, orc = open_index(pkg, O, case, cmap, pb, planes, vb, occ)
    for strands, n in shapes:
        reads = reads_for(case, cmap, n)
        for query, kw in configs:
            for rev, loc in passes:
                check(ix, orc, case, query, reads, cmap, strands, reversed=rev, locate=loc, **kw)
    ix.close()


# ------------------------------------------------------------ the device calls

def run(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, kw, reversed=False, locate=True, skew=1,
        stage_kb=0, fixed_len=0, long_patterns=False, tiles=None):
    """One device call through the query's guard-band runner: d_bytes at
    `skew`, the hints as given (stage_kb = 0: none), `tiles` the staged (True)
    and raw tiles the caller expects, asserted there from the offsets."""
    hints = dict(stage_kb=stage_kb, fixed_len=fixed_len, long_patterns=long_patterns, tiles=tiles)
    if strands != "forward":
        return S.run_device(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, reversed=reversed,
                            locate=locate, skew=skew, **hints, **kw)
    n, a = len(reads), (pkg, ix, mem_cls, case, orc, pb, len(reads), "total", skew, reversed)
    if query == "match":
        return run_match(*a, locate=locate, pats=reads, params=(kw["min_len"], kw["max_occ"]), **hints)
    if query == "seeds":
        return run_seeds(*a, locate=locate, pats=reads,
                         params=(kw["max_seeds"], kw["min_len"], kw["skip"], kw["max_occ"]), **hints)
    return run_approx(*a, locate=locate, best=kw["best"], pats=reads,
                      params=(kw["max_mm"], kw["max_hits"], kw["max_occ"]), **hints)


def tile_count(n, strands):
    return -(-n // (128 if strands == "both" else 256))


# Case 2, the stage edge: (strands, n) of the fixed-length batches — a full tile (two) and a short last one
EDGE_SHAPES = (("forward", 257 + 44), ("reverse", 257 + 44), ("both", 129 + 22))
EDGE_LAYOUTS = ((4, 3, 64), (8, 4, 64))


def stage_edge(pkg, O, mem_cls, pb, planes, vb, query, kw, strands, n, m, text="random", observe=None):
    """Device calls of n reads of m symbols with FMX_HINT_STAGE_KB(56) and
    FMX_HINT_FIXED_LEN(m), d_bytes at an odd address: at m = 224 a full tile
    (256 reads, or both copies of 128) is exactly 57,344 B and staged, at 225
    it is raw and only the short last tile is staged — both facts asserted from
    the offsets; then the host calls of the same batch, which must answer the
    same.  observe(go, tiles, spans, stage, kt_bytes=None): how the caller
    watches the launch go() makes (the emulator's log of dynamic LDS: the
    request, and the bytes each workgroup wrote of it)."""
    case = TEXTS[text](planes)
    cmap = S.involution(case)
    reads = reads_for(case, cmap, n, m)
    per, copies = (128, 2) if strands == "both" else (256, 1)
    full = copies * per * m <= 57344
    tiles = [full] * (n // per) + [True]
    assert n % per and tiles == S.staged_tiles(reads, strands, 56, m)
    # 56 KB; a strand launch of fixed-length reads asks for no more than its tile spans (256 m, rounded to 16)
    stage_of_hint = 57344 if strands == "forward" else min(57344, -(-256 * m // 16) * 16)
    ix, orc = open_index(pkg, O, case, cmap, pb, planes, vb, 1)
    assert_classes(case, orc, reads, cmap, strands)
    for rev, loc in ((False, True), (True, False)):

        def go(rev=rev, loc=loc):
            run(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, kw, reversed=rev, locate=loc,
                skew=1 if rev else 7, stage_kb=56, fixed_len=m, tiles=tiles)
        if observe is not None and not loc:
            spans, stage = [copies * m * len(reads[t:t + per]) for t in range(0, n, per)], stage_of_hint
            observe(go, tiles, spans, stage)
            # the host call's own hints (stage_hint) must come to the same stage: 56 KB at either length
            observe(lambda: S.host_call(ix, query, reads, S.kw_for(query, **kw), strands, rev, False), tiles, spans,
                    stage)
        else:
            go()
        check(ix, orc, case, query, reads, cmap, strands, reversed=rev, locate=loc, **kw)
    ix.close()


def hint_forms(pkg, O, mem_cls, pb, planes, vb, query, kw, strands, n, text="random", observe=None):
    """Case 3: the ragged batch, ordered so that its first tiles hold its
    shortest reads, from device calls under four hints: none (a 16 KB stage:
    every full tile raw), FMX_HINT_LONG_PATTERNS alone (56 KB),
    FMX_HINT_STAGE_KB of the largest tile, rounded up (56 KB at the most), and
    one between the smallest and the largest full tile (some full tiles staged,
    some raw).  Which tile is staged is worked out here from the spans and
    asserted again from the offsets by the runner."""
    case = TEXTS[text](planes)
    cmap = S.involution(case)
    reads = sorted(reads_for(case, cmap, n), key=len)  # (by what the reads are: their length)
    per, copies = (128, 2) if strands == "both" else (256, 1)
    spans = [copies * sum(len(p) for p in reads[t:t + per]) for t in range(0, n, per)]
    fulls = spans[:n // per]
    assert len(fulls) >= 2 and min(fulls) > 16384
    between = -(-min(fulls) // 1024)
    assert min(fulls) <= 1024 * between < min(max(fulls), 57344)
    ix, orc = open_index(pkg, O, case, cmap, pb, planes, vb, 1)
    forms = ((dict(), 16384), (dict(long_patterns=True), 57344),
             (dict(stage_kb=-(-max(spans) // 1024)), min(-(-max(spans) // 1024), 56) * 1024),
             (dict(stage_kb=between), 1024 * between))
    for j, (hint, stage) in enumerate(forms):
        tiles = [s <= stage for s in spans]
        if j == 0:
            assert not any(tiles[:len(fulls)])
        if j == 3:
            assert True in tiles[:len(fulls)] and False in tiles[:len(fulls)]
        rev, loc = bool(j & 1), j < 2

        def go(hint=hint, tiles=tiles, rev=rev, loc=loc, j=j):
            run(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, kw, reversed=rev, locate=loc,
                skew=1 + 2 * j, tiles=tiles, **hint)
        if observe is not None and not loc:
            observe(go, tiles, spans, stage)
        else:
            go()
    ix.close()


def kmer_table_bytes(orc, pb):
    """From the blob header as the oracle parsed it: entries times the position width."""
    return int(orc.ix.kmer_len) * pb


def largest_lds(pkg, O, mem_cls, pb, query, kw, strands, n, observe=None):
    """Case 4: the two-letter text with k = 5 (4^5 k-mer entries: 4,096 B with
    u32 positions, in LDS; 8,192 B with u64, in HBM), reads of 224 symbols
    staged at 56 KB: the launch asks for 57,344 + 4,096 B of dynamic LDS, must
    succeed and answer as the reference does."""
    case = two_letter_case()
    cmap = S.involution(case)
    reads = reads_for(case, cmap, n, 224)
    ix, orc = open_index(pkg, O, case, cmap, pb, 2, 64, 1)
    assert case.k == 5 and kmer_table_bytes(orc, pb) == (4096 if pb == 4 else 8192)
    per, copies = (128, 2) if strands == "both" else (256, 1)
    tiles = [True] * tile_count(n, strands)
    for rev, loc in ((False, False), (True, True)):

        def go(rev=rev, loc=loc):
            run(pkg, ix, mem_cls, case, orc, pb, query, reads, cmap, strands, kw, reversed=rev, locate=loc,
                skew=3, stage_kb=56, fixed_len=224, tiles=tiles)
        if observe is not None and not loc:
            observe(go, tiles, [copies * 224 * len(reads[t:t + per]) for t in range(0, n, per)], 57344,
                    kt_bytes=4096 if pb == 4 else 0)
        else:
            go()
    check(ix, orc, case, query, reads, cmap, strands, **kw)
    ix.close()


# ---------------------------------------------------- the fixed-length hint's limit

def hint_limit(pkg, O, pb=4, planes=3, vb=64):
    """Case 5: host calls of 3 reads of 65,535 symbols (the largest
    FMX_HINT_FIXED_LEN, which the host call sets) and of 65,536 (which it cannot
    hold): random symbols whose last 30 are a text substring.  count and locate
    against the oracle, match and seeds (max_seeds = 4) against Case.expected."""
    case = random_case(planes)
    ix, orc = SC.open_index(pkg, O, case, pb, planes, vb, 1)
    rng = np.random.default_rng(65535)
    t = case.text
    for m in (65535, 65536):
        pats = []
        for _ in range(3):
            s = int(rng.integers(0, len(t) - 30))
            pats.append(bytes(rng.choice(np.frombuffer(case.chars, np.uint8), size=m - 30)) + t[s:s + 30])
        assert all(len(p) == m for p in pats)
        data, offsets = pkg.pack_patterns(pats)
        ooff, olocs = orc.locate_batch(data, offsets)
        cnt = ix.count_batch(pats)
        assert np.array_equal(cnt, np.diff(ooff).astype(cnt.dtype)), f"m={m}: counts"
        off, locs = ix.locate_batch(pats)
        assert np.array_equal(off, ooff) and np.array_equal(locs, olocs), f"m={m}: locations"
        for rev in (False, True):
            exp = S.expected("match", case, orc, pats, dict(min_len=1, max_occ=None))
            assert (exp[0] >= 30).all() and (exp[0] < m).all()
            S.compare(f"match m={m} rev={rev}", S.host_call(ix, "match", pats, dict(min_len=1, max_occ=None),
                                                            reversed=rev), exp)
            kw = dict(max_seeds=4, min_len=1, skip=0, max_occ=None)
            exp = S.expected("seeds", case, orc, pats, kw)
            assert (exp[0] == 4).all() and (exp[1] > 0).all()
            S.compare(f"seeds m={m} rev={rev}", S.host_call(ix, "seeds", pats, kw, reversed=rev), exp)
    ix.close()
