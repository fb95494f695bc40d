"""The same strings, far out on the tape: every call on tapes whose totals cross 2^30, 2^31 and 2^32 bytes.

The shape is sparse. Each side of a call is ONE device byte buffer of 2^32 + 2^21 + 16 bytes filled with `z`; a batch of a few hundred
strings is written into a small region of it and the library is given offsets that START at the region: offsets = base + cumsum(lengths).
The tape total the kernels see is offsets[count] -- above the threshold -- while nothing of size is generated, copied or scored. The
letters are `acgt`, so a read from any wrong address (the fill, or another base's strings: every (regime, base) has its own seed)
changes the answer. Every comparison is exact, against the references of the other test modules, computed once per batch (`known`).

Bases (S = the batch's bytes): 0 (the control), 2^30 - S/2, 2^31 - S/2, 2^32 - S/2 (the threshold falls inside the batch: `inside` a
string -- for lines at least 64 bytes from both of its ends -- or on the `boundary` between two strings), 2^32 + 2^20 (everything
above), and a u32 tape whose last offset is exactly 2^32 - 1.

Regimes -- the engine chooses its kernels by the batch's lengths, so each regime is meant for some of the kernel files:
  * `words`   0 .. 16 bytes, 400 pairs      prepass.hip (k_direct_short), cross.hip, topk.hip and within.hip (the fused searches),
                                            alignshort.hip, and the one-block items of osa / lcs / jaro.hip
    (`many_words`: 2^16 + 64 pairs, the batch size from which short.hip's chunked kernel takes word batches)
  * `tokens`  20 .. 96 bytes, 300 pairs     tiled.hip and bitparallel.hip (bp_item.hpp: 1 .. 3 blocks), wavefront.hip (general costs, and the
                                            class kernels of NW / SW), alignshort.hip (k_align_cross_wide, their cross-product), align.hip
  * `lines`   200 .. 1200 bytes, 60 pairs   bitparallel.hip / tiled.hip (7 .. 38 blocks), banded.hip (k = 0, 7, 32: one word; 100: two words
                                            and the doubling schedule), align.hip's stored Pv / Mv walk, infix.hip, the searches' general path
  * `long`    2100 .. 6000 bytes, 8 pairs   bitparallel.hip's multi-pass kernel (more than 64 blocks), nwprofile.hip and wavefront.hip
    (`long_shorter`: the shorter side cut to 2048 for OSA and LCS; `long_both`: both sides, for Jaro and partial_ratio: their 64-block
    items; `long_near`: the longer side cut to 2048 + 16, partial_ratio's needle of 64 blocks under more than one whole window)
  * `spaced_words`, `spaced_tokens`, `spaced_lines`: the same batches with every `t` a space, so a string is 1 .. 300 tokens of `acg`
                                            between single and repeated spaces: tokens.hip (PreparedTape.token_sorted, token_sort_ratio,
                                            token_set_counts) -- a line holds at most 1200 bytes, under the calls' cap of 4096
The score searches (extract.hip, extract_within.hip over the slices of two_tape.hip's ExtractSweep) run windows of 12 x 20 words and 4 x 6
lines; partial.hip the words, the tokens, `infix` (the tokens' a side cut to 64 symbols in the lines: hundreds of windows a pair),
`long_both` (equal lengths: both directions) and the pair of `long_near` at the threshold. Its reference scores every whole window of
the haystack against the needle, 2048 big-integer steps each: 0.07 s a pair at equal lengths, 0.2 s with 17 windows, seconds with
the hundreds of `long_shorter` -- which is why partial_ratio has regimes of its own for needles of 64 blocks.
The code-point engine runs the same regimes with the letters mapped to four of `a é Ж 中 😀` (lengths in symbols, layout in bytes) on
the first 2^30 + 2^21 + 16 bytes of the same buffers, at the control and the 2^30 base: bp_item.hpp's SymWindow32 and prepass.hip's
staging; staged string by string the symbols lie where the bytes did, at indices at or above 2^30 of a symbol buffer of over 4 GiB.

Forms: raw device tapes with u64 offsets at every base and u32 offsets (an int32 tensor: values at or above 2^31 are the point) at the
control, the 2^30 and the 2^31 base; prepared tapes over the same in both widths; one prepared tape per side that spans the 2^32 and the
above-2^32 region, called through sub-views; (far a, far b), (far a, small b in a buffer of its own) and the reverse; results on the
host everywhere and on the device once per family (alignments and infix matches come back on the host by their interface).
Not every family takes every form, by the interface and not by choice: cross-products, top-k and within have raw exports for u64
offsets only, so their u32 tapes run prepared (`raw32=False`); align, infix, OSA, LCS and Jaro prepare the device tapes they are given
in the Python wrapper before they call, so for them a raw form would be the prepared one again and only those run (`raw=False`) -- as
do partial_ratio and the token calls, which derive their tapes from prepared ones; extract and extract_within have raw exports for u64
offsets only, like top-k; the code-point engine runs at two bases, and raw with one far tape only (device memory, below).

Device memory, by arithmetic from api.hip and, for the searches, two_tape.hip (no test may need more than 24 GiB):
  * the two buffers: 2 x (2^32 + 2^21 + 16) B = 8.004 GiB, allocated once per module and freed at its teardown;
  * byte calls add the regions' small copies, offsets, results and the searches' matrices (24 x 400 x 4 B): under 0.1 GiB -> 8.1 GiB;
  * the score searches carve ExtractSweep::need() -- 16 B of first over-long strings, one OsaSizes, 16 B of LaneItem and up to 3 counts
    of 8 B per pair of a slice, 12 x 20 pairs here -- and k x 16 B of lists per query: some 10 KiB; token_sorted stages the view's span
    (at most 60 lines of 1200 B: 72 KiB) and owns a derived tape no larger; partial_ratio's scratch (partial_scratch_bytes) is 8 B per
    pair and 16 + 12 B per item of at most 4096 column steps: under 1 MiB for the 60 `infix` pairs. None of it is seen next to 8 GiB;
  * a prepared UTF-8 tape owns (total + 4) x 4 B of symbols = 4.008 GiB at total = 2^30 + S/2, 8 B per string of offsets, and while it
    is prepared utf8_scratch_words(total) x 4 B = 36 words per 8 KiB tile = 0.018 GiB: two far prepared tapes 8.02 GiB -> 16.1 GiB
    (partial_ratio and the token calls of the code-point engine run on these prepared tapes alone, freed form by form; the searches
    also raw, as the next line has it);
  * a raw UTF-8 call stages in the scope's scratch: per tape (bytes + 4) x 4 B twice (the flat and the string-by-string staging are both
    provided for) + the scratch words; `ensure` allocates need x 1.25 + 1 MiB. One far tape against a small one: 8.03 GiB x 1.25 =
    10.04 GiB -> 18.1 GiB with the buffers, on a scope of the test's own that is closed afterwards, after the prepared tapes are freed.
    BOTH tapes far would be 16.07 GiB x 1.25 = 20.1 GiB -> 28.1 GiB: that form (raw UTF-8, far a and far b) is left out; far a with far
    b runs prepared."""
import functools

import numpy as np
import pytest

import test_partial_ratio as partial_tests
import test_token_ratios as token_tests
from test_align import script_errors
from test_extract import LARGER_IS_BETTER, SCORERS, assert_rows, expected_rows, reference_scores
from test_extract_within import assert_csr, batch_cutoffs, expected_within
from test_gpu_parity import ALGORITHMS
from test_lcs import reference_lcs
from test_osa import mutated
from test_search_edges import counts_of, extract_rows, within_csr
from test_tape_edges import expanded, expected, remember, run_cross, run_pairs, same
from test_topk import check_rows, expected_topk
from test_within import check_csr, expected_csr

gpu = pytest.mark.gpu

FILL = ord("z")
FAR_BYTES = (1 << 32) + (1 << 21) + 16      # one side's buffer
FAR_BYTES_UTF8 = (1 << 30) + (1 << 21) + 16   # what the code-point engine sees of it
LETTERS = "acgt"
GLYPHS = "aéЖ中\U0001f600"
THRESHOLDS = {"2^30": 1 << 30, "2^31": 1 << 31, "2^32": 1 << 32}
ABOVE = (1 << 32) + (1 << 20)
BASES = ("control", "2^30", "2^31", "2^32", "above")      # placed together: no two of their regions overlap
U32_BASES = ("control", "2^30", "2^31")
UTF8_BASES = ("control", "2^30")
ARRANGEMENTS = ("inside", "boundary")
REGIMES = {"words": (400, 0, 16), "tokens": (300, 20, 96), "lines": (60, 200, 1200), "long": (8, 2100, 6000)}   # pairs, shortest, longest
SPACED = ("spaced_words", "spaced_tokens", "spaced_lines")   # the token calls' batches: every `t` of the strings is a space
NEAR = 16   # symbols the haystack of `long_near` holds more than its needle
DERIVED = ("long_shorter", "long_both", "long_near", "infix") + SPACED
MANY_WORDS = (1 << 16) + 64   # pairs of the `many_words` batch: k_short_tiled takes word batches of 2^16 pairs and more
BOUNDS = (0, 7, 32, 100)
COSTS = (0, 1, 2, 1)
CUT = 2048
MODELS = ("mod 2^32", "sign-extended from 32 bits", "mod 2^31", "start clamped to 2^30", "total - start clamped to 2^30 as the end")


# ---- the generators -----------------------------------------------------------------------------------------------------------------
def seed_of(regime, base):
    return 77000 + 16 * (list(REGIMES) + ["many_words"]).index(regime) + (BASES + ("u32max",)).index(base)


@functools.lru_cache(maxsize=None)
def batch(regime, base):
    """(a, b): the strings of a (regime, base) over `acgt`; b[k] is a mutated copy of a[k] (substitutions, insertions, deletions, swaps
    of neighbours) for two pairs of three and independent for the third. Every (regime, base) has its own seed."""
    if regime == "long_shorter":   # OSA, LCS: the shorter string holds at most 2048 symbols
        a, b = batch("long", base)
        return ([x[:CUT] if len(x) <= len(y) else x for x, y in zip(a, b)], [y[:CUT] if len(y) < len(x) else y for x, y in zip(a, b)])
    if regime == "long_both":      # Jaro: neither holds more
        a, b = batch("long", base)
        return [x[:CUT] for x in a], [y[:CUT] for y in b]
    if regime == "long_near":      # partial_ratio: a needle of 2048 symbols, 17 whole windows of the haystack between the 2047 cut ones at either end
        a, b = batch("long_shorter", base)
        return [x[:CUT + NEAR] for x in a], [y[:CUT + NEAR] for y in b]
    if regime == "infix":          # patterns: tokens' a side cut to 64 symbols; texts: the lines' b side
        return [x[:64] for x in batch("tokens", base)[0][:REGIMES["lines"][0]]], batch("lines", base)[1]
    if regime in SPACED:           # tokens of `acg` between single and repeated spaces; the fill `z` is no space
        return tuple([x.replace("t", " ") for x in side] for side in batch(regime[len("spaced_"):], base))
    if regime == "many_words":
        return many_words(base)
    count, shortest, longest = REGIMES[regime]
    rng = np.random.default_rng(seed_of(regime, base))
    draw = lambda: LETTERS[int(rng.integers(0, 4))]
    word = lambda: "".join(LETTERS[int(k)] for k in rng.integers(0, 4, int(rng.integers(shortest, longest + 1))))
    a, b = [], []
    for k in range(count):
        x = word()
        if k % 3 < 2:
            y = "".join(mutated(rng, x, int(rng.integers(1, max(3, len(x) // 12) + 1)), draw))[:longest]
            y += "".join(draw() for _ in range(shortest - len(y)))
        else:
            y = word()
        a.append(x); b.append(y)
    return a, b


def many_words(base):
    """2^16 + 64 pairs of 0 .. 16 letters, cut from one long random string: b[k] is a[k] with one letter changed, a[k] without its
    first letter and with one changed, or a word of its own, in turn."""
    rng = np.random.default_rng(seed_of("many_words", base))
    sizes = rng.integers(0, 17, (2, MANY_WORDS))
    ends = np.concatenate([[0], np.cumsum(sizes.ravel())])
    text = "".join(LETTERS[k] for k in rng.integers(0, 4, int(ends[-1])))
    words = [text[s:e] for s, e in zip(ends, ends[1:])]
    a, b = words[:MANY_WORDS], words[MANY_WORDS:]
    spots = rng.integers(0, 16, MANY_WORDS)
    for k in range(MANY_WORDS):
        if k % 3 < 2:
            x = a[k][k % 3:]
            at = int(spots[k]) % max(len(x), 1)
            b[k] = x[:at] + LETTERS[(LETTERS.index(x[at]) + 1) % 4] + x[at + 1:] if x else x
    return a, b


def glyph_map(regime, base):
    """Four of the five glyphs (one to four bytes each), another four for every batch."""
    source = regime[len("spaced_"):] if regime in SPACED else regime.split("_")[0]   # (the infix batch draws on two regimes: it runs on bytes alone)
    drop = seed_of(source, base) % 5
    return str.maketrans(LETTERS, GLYPHS[:drop] + GLYPHS[drop + 1:])   # (a spaced batch has no `t` left: its spaces stay spaces)


def items(regime, base, utf8):
    """The batch as the tapes hold it: lists of bytes."""
    a, b = batch(regime, base)
    if utf8:
        table = glyph_map(regime, base)
        a, b = [x.translate(table) for x in a], [y.translate(table) for y in b]
    return [x.encode() for x in a], [y.encode() for y in b]


def as_called(strings, utf8):
    """What the references take: bytes for the byte engine, str for the code-point engine."""
    return [s.decode() for s in strings] if utf8 else list(strings)


class Region:
    """One side of a (regime, base, arrangement): `strings` (bytes) laid end to end from byte `start` of the buffer. `at`: the string
    the threshold falls in (inside) or begins (boundary); the middle one where there is no threshold."""

    def __init__(self, strings, base, arrangement):
        self.strings, self.base = strings, base
        self.lengths = np.array([len(s) for s in strings], dtype=np.int64)
        self.deep = int(self.lengths.min()) >= 200   # lines and longer: the threshold at least 64 bytes from the string's ends
        self.ends = np.concatenate([[0], np.cumsum(self.lengths)])
        self.bytes = int(self.ends[-1])
        half = self.bytes // 2
        if base in THRESHOLDS:
            far_off = np.int64(1) << 62
            if arrangement == "inside":
                need = 130 if self.deep else 2
                middles = self.ends[:-1] + self.lengths // 2
                self.at = int(np.argmin(np.where(self.lengths >= need, np.abs(middles - half), far_off)))
                self.start = THRESHOLDS[base] - int(middles[self.at])
            else:   # between two strings that both hold something
                both = (self.lengths[:-1] > 0) & (self.lengths[1:] > 0)
                self.at = 1 + int(np.argmin(np.where(both, np.abs(self.ends[1:-1] - half), far_off)))
                self.start = THRESHOLDS[base] - int(self.ends[self.at])
        else:
            self.at = len(strings) // 2
            self.start = {"control": 0, "above": ABOVE, "u32max": (1 << 32) - 1 - self.bytes}[base]
        self.offsets = self.start + self.ends      # int64: every value is below 2^63
        self.payload = b"".join(strings)

    def window(self, count):
        """`count` consecutive strings around `at` (a search's queries, a cross-product's sides): (first, count)."""
        count = min(count, len(self.strings))
        return max(0, min(self.at - count // 2, len(self.strings) - count)), count


@functools.lru_cache(maxsize=None)
def layout(regime, arrangement, utf8=False, bases=BASES):
    """{base: (region a, region b)}: what lies in the two buffers while a (regime, arrangement) is tested."""
    out = {}
    for base in bases:
        a, b = items(regime, base, utf8)
        out[base] = (Region(a, base, arrangement), Region(b, base, arrangement))
    return out


class SparseTape:
    """A buffer of `size` fill bytes with a few live regions, as a dict: the CPU model of one side's device buffer."""

    def __init__(self, size, regions):
        self.size, self.regions = size, sorted((r.start, r.payload) for r in regions)

    def overlaps(self):
        return any(s0 + len(p0) > s1 for (s0, p0), (s1, _) in zip(self.regions, self.regions[1:])) or \
            any(s < 0 or s + len(p) > self.size for s, p in self.regions)

    def read(self, start, end):
        """Bytes [start, end): the fill wherever nothing is live, below 0 and beyond the buffer too (a wrong read, never a fault here)."""
        out = bytearray([FILL]) * max(end - start, 0)
        for s, p in self.regions:
            lo, hi = max(start, s), min(end, s + len(p))
            if lo < hi:
                out[lo - start:hi - start] = p[lo - s:hi - s]
        return bytes(out)


def misaddressed(model, start, end, total):
    """Where a kernel with the bug `model` reads the string [start, end) of a tape of `total` bytes."""
    length = end - start
    if model == "mod 2^32":
        start %= 1 << 32
    elif model == "sign-extended from 32 bits":
        start %= 1 << 32
        start -= (1 << 32) if start >= (1 << 31) else 0
    elif model == "mod 2^31":
        start %= 1 << 31
    elif model == "start clamped to 2^30":
        start = min(start, 1 << 30)
    else:
        length = min(total - start, 1 << 30)
    return start, start + length


# ---- the references, computed once per batch ----------------------------------------------------------------------------------------
_known = {}


def known(key, compute):
    if key not in _known:
        _known[key] = compute()
    return _known[key]


def levenshtein_of(sw, orc, a, b, utf8=False, costs=None):
    """int64 distances of the pairs (a[k], b[k]) of two lists of bytes, by the oracle."""
    def compute():
        sa, sb = sw.Strs(a), sw.Strs(b)
        d = orc.levenshtein_costs_pairs(sa, sb, *costs) if costs else orc.levenshtein_pairs(sa, sb, utf8=utf8, algo="wf" if utf8 else "hyyro")
        return np.asarray(d, dtype=np.int64)
    return known(("lev", utf8, costs, tuple(a), tuple(b)), compute)


def matrix_of(sw, orc, queries, candidates):
    return levenshtein_of(sw, orc, *expanded(queries, candidates)).reshape(len(queries), len(candidates))


# ---- the CPU test: the layout can catch what it is for -------------------------------------------------------------------------------
def string_extents(region):
    return [(int(s), int(e)) for s, e in zip(region.offsets, region.offsets[1:])]


def ratio_row(query, candidates):
    """The reference extract result of one query under `ratio`, k = 3: (indices, score patterns)."""
    lcs = reference_lcs([query] * len(candidates), candidates).reshape(1, len(candidates))
    unused = np.zeros_like(lcs)
    lengths = np.array([len(query)], dtype=np.int64), np.array([len(c) for c in candidates], dtype=np.int64)
    return expected_rows(reference_scores("ratio", (unused, lcs, unused, unused, unused) + lengths), True, 3)


def test_layout_can_catch_misaddressing(sw, orc):
    """The generators alone, on a sparse model of the buffers: every threshold falls where its arrangement says, every batch is
    distinct, the u32 forms stay below 2^32, no live region overlaps another -- and for every misaddressing model, reading a batch
    through it changes the oracle's Levenshtein distance of some pair, wherever the model changes any address at all; on the words
    also a row of the reference `extract` result under `ratio` (one query against the six candidates around it) and a row of the
    partial-ratio reference, and on the spaced words a token normal form."""
    from stringwars_amd import _native as N
    # the searches have raw exports for u64 offsets only: their u32 tapes run prepared (`raw32=False`)
    assert all("u32" not in kinds for _, stem, _, kinds in N.TWO_TAPE if stem in ("extract", "extract_within", "topk", "within"))
    payloads, caught, caught_search, caught_partial, caught_tokens = [], set(), set(), set(), set()
    for utf8 in (False, True):
        size = FAR_BYTES_UTF8 if utf8 else FAR_BYTES
        for regime in tuple(REGIMES) + (("spaced_words",) if utf8 else DERIVED + ("many_words",)):
            for arrangement in ARRANGEMENTS:
                lay = layout(regime, arrangement, utf8, UTF8_BASES if utf8 else BASES)
                tapes = [SparseTape(size, [lay[base][side] for base in lay]) for side in (0, 1)]
                assert not tapes[0].overlaps() and not tapes[1].overlaps(), (regime, arrangement, utf8)
                for base, regions in lay.items():
                    for side, r in enumerate(regions):
                        assert FILL not in r.payload and r.offsets[-1] <= size
                        assert regime == "many_words" or [tapes[side].read(s, e) for s, e in string_extents(r)] == r.strings
                        if arrangement == "inside" and regime in REGIMES:
                            payloads.append(r.payload)
                        if base in U32_BASES:
                            assert r.offsets[-1] <= (1 << 32) - 1
                        if base not in THRESHOLDS:
                            continue
                        T, first, last = THRESHOLDS[base], int(r.offsets[r.at]), int(r.offsets[r.at + 1])
                        assert r.offsets[0] < T < r.offsets[-1], (regime, base, arrangement)
                        if arrangement == "inside":
                            assert first < T < last, (regime, base, side)
                            assert not r.deep or first + 64 <= T <= last - 64, (regime, base, side)
                        else:
                            assert first == T and r.lengths[r.at - 1] and r.lengths[r.at], (regime, base, side)
                    assert regime not in ("lines", "long") or (regions[0].deep and regions[1].deep)
                if utf8 or regime not in tuple(REGIMES) + ("spaced_words",):
                    continue
                for base, regions in lay.items():
                    a, b = items(regime, base, False)
                    want = levenshtein_of(sw, orc, a, b) if regime in REGIMES else None
                    true = [string_extents(r) for r in regions]
                    for model in MODELS:
                        moved = [[misaddressed(model, s, e, int(r.offsets[-1])) for s, e in x] for r, x in zip(regions, true)]
                        changed = [k for k in range(len(a)) if moved[0][k] != true[0][k] or moved[1][k] != true[1][k]]
                        # (the pairs whose misread strings are shortest first: the oracle is quadratic, and one changed distance is enough)
                        changed.sort(key=lambda k: sum(m[k][1] - m[k][0] for m in moved))
                        if not changed:
                            continue
                        misread = [lambda k, side=side: tapes[side].read(*moved[side][k]) for side in (0, 1)]
                        where = (regime, base, arrangement, model)
                        if regime in REGIMES:
                            assert any(orc.levenshtein(misread[0](k), misread[1](k), algo="hyyro") != want[k] for k in changed), where
                            caught.add((model, base))
                        if regime == "words":   # what sections i and j compare: one changed row each is enough, the cheapest pairs first
                            around = lambda k: range(max(0, k - 2), min(len(b), k + 4))
                            assert any(not all((x == y).all() for x, y in zip(ratio_row(misread[0](k), [misread[1](j) for j in around(k)]),
                                                                               ratio_row(a[k], [b[j] for j in around(k)]))) for k in changed), where
                            caught_search.add((model, base))
                            assert any((partial_tests.expected([misread[0](k)], [misread[1](k)]) != partial_tests.expected([a[k]], [b[k]])).any()
                                       for k in changed), where
                            caught_partial.add((model, base))
                        if regime == "spaced_words":   # section k
                            assert any(token_tests.normal_form(misread[side](k), unique) != token_tests.normal_form((a, b)[side][k], unique)
                                       for k in changed for side in (0, 1) for unique in (False, True)), where
                            caught_tokens.add((model, base))
    # every model moves something at every base it can: the first four from the threshold they are named for on, the fifth everywhere
    for model, first in zip(MODELS, ("2^32", "2^31", "2^31", "2^30", "control")):
        for kind in (caught, caught_search, caught_partial, caught_tokens):
            assert {base for m, base in kind if m == model} == set(BASES[BASES.index(first):]), (model, kind)
    for regime in tuple(REGIMES) + ("many_words",):   # the u32 tape that ends at 2^32 - 1, placed alone (it lies where the 2^32 base's strings do)
        for r in layout(regime, "inside", False, ("u32max",))["u32max"]:
            assert r.offsets[-1] == (1 << 32) - 1 and r.offsets[0] > (1 << 31) and r.start + r.bytes <= FAR_BYTES
            if regime in REGIMES:
                payloads.append(r.payload)
    many = layout("many_words", "inside")
    assert len({many[base][side].payload for base in many for side in (0, 1)}) == 2 * len(BASES) and len(many["2^32"][0].strings) == MANY_WORDS
    assert len(payloads) == len(REGIMES) * 2 * (len(BASES) + len(UTF8_BASES) + 1) and len(set(payloads)) == len(payloads)


# ---- the buffers and the tapes ------------------------------------------------------------------------------------------------------
class Far:
    """The two device buffers, and the tapes over them."""

    def __init__(self, sw):
        import torch
        self.sw, self.torch = sw, torch
        self.data = [torch.full((FAR_BYTES,), FILL, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
        self.live, self.small = [], {}
        torch.cuda.synchronize()

    def close(self):
        self.clear()
        self.data = None
        self.torch.cuda.empty_cache()

    def on_device(self, array):
        return self.torch.from_numpy(np.array(array, copy=True)).cuda()   # (a copy: the strings' own bytes are read-only)

    def place(self, lay):
        """Writes a layout's regions into the buffers (what lay there before goes back to the fill), and each region into a small
        buffer of its own as well: the other side of a (far, small) call."""
        self.clear()
        for base, regions in lay.items():
            for side, r in enumerate(regions):
                payload = np.frombuffer(r.payload + b"z" * 16, dtype=np.uint8)
                if r.bytes:
                    self.data[side][r.start:r.start + r.bytes] = self.on_device(payload[:r.bytes])
                    self.live.append((side, r.start, r.bytes))
                self.small[(base, side)] = self.on_device(payload)
        self.torch.cuda.synchronize()

    def clear(self):
        for side, start, size in self.live:
            self.data[side][start:start + size] = FILL
        self.live, self.small = [], {}
        self.torch.cuda.synchronize()

    def offsets(self, values, width):
        values = np.asarray(values, dtype=np.int64)
        if width == 32:   # an int32 tensor holds the bits of the uint32 offsets: those at or above 2^31 come out negative
            assert 0 <= values.min() and values.max() <= (1 << 32) - 1
            return self.on_device(values.astype(np.uint64).astype(np.uint32).view(np.int32))
        return self.on_device(values)

    def tape(self, lay, base, side, width=64, first=0, count=None, small=False):
        """Strings [first, first + count) of a region as a raw device tape: over the far buffer, or (small) over the region's own."""
        r = lay[base][side]
        count = len(r.strings) - first if count is None else count
        values = r.offsets[first:first + count + 1] - (r.start if small else 0)
        return self.sw.DeviceTape.from_torch(self.small[(base, side)] if small else self.data[side], self.offsets(values, width))

    def spanning(self, lay, side, scope, width=64, utf8=False):
        """One prepared tape over the 2^32 and the above-2^32 region, the fill between them as one string that no view holds: the
        reference's call shape -- a whole dataset prepared once, sub-viewed per call. Returns the tape and {base: (first, count)}."""
        lower, upper = lay["2^32"][side], lay["above"][side]
        values = np.concatenate([lower.offsets, upper.offsets])
        tape = self.sw.DeviceTape.from_torch(self.data[side], self.offsets(values, width))
        return self.sw.PreparedTape(scope, tape, utf8=utf8), {"2^32": (0, len(lower.strings)), "above": (len(lower.strings) + 1, len(upper.strings))}


@pytest.fixture(scope="module")
def far(sw):
    buffers = Far(sw)
    yield buffers
    buffers.close()


@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


def forms(far, scope, lay, select=lambda r: (0, len(r.strings)), raw=True, raw32=True, utf8=False, u32=U32_BASES):
    """(what, tape a, tape b, first a, count a, first b, count b) of a placed layout: which strings of either side the call sees, as
    `select(region)` says. Raw device tapes with u64 offsets at every base and u32 offsets at `u32`; far a with small b and the reverse
    at every base but the control; prepared tapes over the same far tapes in both widths; sub-views of a prepared tape that spans the
    2^32 and the above-2^32 region. `raw`: the call takes raw device tapes; `raw32`: also with u32 offsets."""
    sw = far.sw
    picks = {base: (select(lay[base][0]), select(lay[base][1])) for base in lay}
    for base in lay:
        (fa, ca), (fb, cb) = picks[base]
        where = (fa, ca, fb, cb)
        for width in (32,) if base == "u32max" else (64, 32) if base in u32 else (64,):
            ta, tb = far.tape(lay, base, 0, width, fa, ca), far.tape(lay, base, 1, width, fb, cb)
            if raw and (width == 64 or raw32):
                yield ("raw u%d" % width, base), ta, tb, *where
            yield ("prepared u%d" % width, base), sw.PreparedTape(scope, ta, utf8=utf8), sw.PreparedTape(scope, tb, utf8=utf8), *where
        if base not in ("control", "u32max"):
            sa, sb = far.tape(lay, base, 0, 64, fa, ca, small=True), far.tape(lay, base, 1, 64, fb, cb, small=True)
            ta, tb = far.tape(lay, base, 0, 64, fa, ca), far.tape(lay, base, 1, 64, fb, cb)   # (u64: the loop above may have ended on u32, and the two sides of a call share one width)
            if raw:
                yield ("raw far a, small b", base), ta, sb, *where
                yield ("raw small a, far b", base), sa, tb, *where
            else:
                yield ("prepared far a, small b", base), sw.PreparedTape(scope, ta, utf8=utf8), sw.PreparedTape(scope, sb, utf8=utf8), *where
                yield ("prepared small a, far b", base), sw.PreparedTape(scope, sa, utf8=utf8), sw.PreparedTape(scope, tb, utf8=utf8), *where
    if "2^32" in lay and "above" in lay:
        (pa, va), (pb, vb) = far.spanning(lay, 0, scope, 64, utf8), far.spanning(lay, 1, scope, 64, utf8)
        for base in ("2^32", "above"):
            (fa, ca), (fb, cb) = picks[base]
            yield ("sub-view of a spanning prepared tape", base), pa[va[base][0] + fa:va[base][0] + fa + ca], \
                pb[vb[base][0] + fb:vb[base][0] + fb + cb], fa, ca, fb, cb


def placements(far, regime, utf8=False):
    """The layouts of a regime, each placed in turn: the five bases with the threshold inside a string, the three thresholds again on
    a boundary between two strings, and the u32 tape that ends at 2^32 - 1 (it lies where the 2^32 base's strings do)."""
    if utf8:
        plan = [("inside", UTF8_BASES), ("boundary", ("2^30",))]
    else:
        plan = [("inside", BASES), ("boundary", tuple(THRESHOLDS)), ("inside", ("u32max",))]
    for arrangement, bases in plan:
        lay = layout(regime, arrangement, utf8, bases)
        far.place(lay)
        yield arrangement, lay
    far.clear()


def sides(lay, base, where, utf8=False):
    """The strings a form's call sees, as the references take them."""
    fa, ca, fb, cb = where
    return as_called(lay[base][0].strings[fa:fa + ca], utf8), as_called(lay[base][1].strings[fb:fb + cb], utf8)


def device_result(scope, tensor, dtype):
    scope.synchronize()
    return tensor.cpu().numpy().view(dtype)


# ---- a. Levenshtein distances, pairwise ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_levenshtein_pairs(sw, orc, scope, far, algorithm):
    """Every algorithm on all four regimes, every form; once with the distances left on the device."""
    import torch
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm=algorithm)
    on_device = False
    for regime in REGIMES:
        for arrangement, lay in placements(far, regime):
            for what, ta, tb, *where in forms(far, scope, lay):
                a, b = sides(lay, what[1], where)
                want = levenshtein_of(sw, orc, a, b)
                got = engine.pairs(ta, tb, scope)
                assert (got == want).all(), (algorithm, regime, arrangement, what, np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
                if what == ("raw u64", "2^32"):
                    out = torch.full((len(a),), -7, dtype=torch.int32, device="cuda")
                    engine.pairs(ta, tb, scope, out=out)
                    assert (device_result(scope, out, np.uint32) == want).all(), (algorithm, regime, arrangement, "device out")
                    on_device = True
    assert on_device


@gpu
def test_levenshtein_bounds_and_general_costs(sw, orc, scope, far, lev):
    """Bounds of 0, 7, 32 (one band word) and 100 (two words, the doubling schedule) on the lines; costs (0, 1, 2, 1) on the tokens."""
    costly = sw.LevenshteinDistances(*COSTS, capabilities=scope)
    for arrangement, lay in placements(far, "lines"):
        for what, ta, tb, *where in forms(far, scope, lay):
            a, b = sides(lay, what[1], where)
            want = levenshtein_of(sw, orc, a, b)
            for bound in BOUNDS:
                got = lev.pairs(ta, tb, scope, bound=bound)
                assert (got == np.minimum(want, bound + 1)).all(), ("lines", arrangement, what, bound, np.nonzero(got != np.minimum(want, bound + 1))[0][:5])
    for arrangement, lay in placements(far, "tokens"):
        for what, ta, tb, *where in forms(far, scope, lay):
            a, b = sides(lay, what[1], where)
            want = levenshtein_of(sw, orc, a, b, costs=COSTS)
            got = costly.pairs(ta, tb, scope)
            assert (got == want).all(), ("tokens", arrangement, what, np.nonzero(got != want)[0][:5])


@gpu
def test_word_batches_on_the_chunked_kernel(sw, orc, scope, far, lev):
    """2^16 + 64 pairs of words: prepared, they run on short.hip (k_short_tiled takes batches of 2^16 pairs and more), whose chunks
    hold their strings' starts relative to the chunk's first byte -- here with the threshold inside a chunk. Raw tapes and the
    sub-views of the spanning tape take the routes the scope's beliefs and the tape's longest string give them."""
    chunked = set()
    for arrangement, lay in placements(far, "many_words"):
        for what, ta, tb, *where in forms(far, scope, lay):
            a, b = sides(lay, what[1], where)
            want = levenshtein_of(sw, orc, a, b)
            scope.set_profiling(True)
            got = lev.pairs(ta, tb, scope)
            name = scope.last_timing()["dominant_name"]
            scope.set_profiling(False)
            assert (got == want).all(), (arrangement, what, name, np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
            if what[0].startswith("prepared u"):
                assert name == "short_tiled", (arrangement, what, name)
                chunked.add(what)
            got = lev.pairs(ta, tb, scope, bound=1)
            assert (got == np.minimum(want, 2)).all(), (arrangement, what, "bound 1", np.nonzero(got != np.minimum(want, 2))[0][:5])
    assert {base for _, base in chunked} == set(BASES + ("u32max",))


# ---- b. the code-point engine -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_levenshtein_utf8(sw, orc, far, regime):
    """The letters as four of `a é Ж 中 😀` on the first 2^30 + 2^21 + 16 bytes of the buffers, at the control and the 2^30 base:
    prepared (decoded once: far a with far b, both widths, and against a small tape), then -- the prepared tapes freed -- raw, staged
    in the call, one far tape against a small one (both far would need 28 GiB: the module's docstring). Unbounded, and bounded at 32.
    A scope of the test's own: what it stages raw stays in the scope's scratch, over 10 GiB, until the scope is closed."""
    import torch
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope)
    on_device = set()

    def into_device_memory(ta, tb, want, what, form):
        out = torch.full((len(want),), -7, dtype=torch.int32, device="cuda")
        engine.pairs(ta, tb, scope, out=out)
        assert (device_result(scope, out, np.uint32) == want).all(), (regime, what, "device out")
        on_device.add(form)

    try:
        for arrangement, lay in placements(far, regime, utf8=True):
            assert all(r.offsets[-1] <= FAR_BYTES_UTF8 for regions in lay.values() for r in regions)
            for what, ta, tb, *where in forms(far, scope, lay, raw=False, utf8=True, u32=UTF8_BASES):
                a, b = sides(lay, what[1], where, utf8=True)
                want = levenshtein_of(sw, orc, [x.encode() for x in a], [y.encode() for y in b], utf8=True)
                for bound in (None, 32):
                    got = engine.pairs(ta, tb, scope, bound=bound)
                    wanted = want if bound is None else np.minimum(want, bound + 1)
                    assert (got == wanted).all(), (regime, arrangement, what, bound, np.nonzero(got != wanted)[0][:5])
                if what == ("prepared u64", "2^30"):
                    into_device_memory(ta, tb, want, what, "prepared")
                ta.free(); tb.free()
            for base in lay:
                ra, rb = lay[base]
                a, b = sides(lay, base, (0, len(ra.strings), 0, len(rb.strings)), utf8=True)
                want = levenshtein_of(sw, orc, [x.encode() for x in a], [y.encode() for y in b], utf8=True)
                for small_side in (1, 0):
                    ta, tb = far.tape(lay, base, 0, small=small_side == 0), far.tape(lay, base, 1, small=small_side == 1)
                    for bound in (None, 32):
                        got = engine.pairs(ta, tb, scope, bound=bound)
                        wanted = want if bound is None else np.minimum(want, bound + 1)
                        assert (got == wanted).all(), (regime, arrangement, "raw, small side %d" % small_side, base, bound, np.nonzero(got != wanted)[0][:5])
                    if base == "2^30":
                        into_device_memory(ta, tb, want, ("raw, small side %d" % small_side, base), "raw")
        assert on_device == {"prepared", "raw"}
    finally:
        del engine
        scope.close()


# ---- c. Needleman-Wunsch and Smith-Waterman -------------------------------------------------------------------------------------------
def alignment_scores(orc, a, b, matrix, gaps, local):
    def compute():
        return np.array([orc.nw_score(x, y, matrix, gaps[0], gaps[1], local=local) for x, y in zip(a, b)], dtype=np.int64)
    return known(("scores", matrix.tobytes(), gaps, local, tuple(a), tuple(b)), compute)


@gpu
@pytest.mark.parametrize("gaps", [(-4, -4), (-11, -1)], ids=["linear", "affine"])
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
@pytest.mark.parametrize("model", ["classes", "few classes", "matrix"])
def test_alignment_scores(sw, orc, scope, far, model, local, gaps):
    """`classes`: a class table on the words (alignshort.hip) and the tokens (wavefront.hip's class kernels; their cross-product, in
    test_cross_products, is alignshort.hip's again). `few classes`: a substitution matrix that folds into a class table, on the long
    pairs (nwprofile.hip). `matrix`: one of 256 classes on the long pairs (wavefront.hip, several passes)."""
    Engine = sw.SmithWatermanScores if local else sw.NeedlemanWunschScores
    if model == "classes":
        byte_to_class, costs = sw.unary_class_costs(2, -1)
        matrix = np.array([[costs[i % 32, j % 32] for j in range(256)] for i in range(256)], dtype=np.int8)
        engine = Engine(byte_to_class, costs, open=gaps[0], extend=gaps[1], capabilities=scope)
    else:
        matrix = np.random.default_rng(5).integers(-8, 9, (256, 256)).astype(np.int8)
        matrix = sw.substitution_matrix(42, b"acgt") if model == "few classes" else np.maximum(matrix, matrix.T)
        engine = Engine(substitution_matrix=matrix, open=gaps[0], extend=gaps[1], capabilities=scope)
    import torch
    on_device = set()
    for regime in ("words", "tokens") if model == "classes" else ("long",):
        for arrangement, lay in placements(far, regime):
            for what, ta, tb, *where in forms(far, scope, lay):
                a, b = sides(lay, what[1], where)
                want = alignment_scores(orc, a, b, matrix, gaps, local)
                got = engine.pairs(ta, tb, scope)
                assert (got == want).all(), (regime, arrangement, what, np.nonzero(got != want)[0][:5])
                if what in (("raw u64", "2^32"), ("prepared u64", "2^32")):
                    out = torch.full((len(a),), -7, dtype=torch.int32, device="cuda")
                    engine.pairs(ta, tb, scope, out=out)
                    assert (device_result(scope, out, np.int32) == want).all(), (regime, arrangement, what, "device out")
                    on_device.add(what[0])
    assert on_device == {"raw u64", "prepared u64"}


# ---- d. cross-products ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("regime", ["words", "tokens"])
def test_cross_products(sw, orc, scope, far, lev, regime):
    """24 x 40 strings around the threshold: Levenshtein (cross.hip for the words) and Needleman-Wunsch; each once into a device matrix."""
    import torch
    byte_to_class, costs = sw.unary_class_costs(2, -1)
    as_matrix = np.array([[costs[i % 32, j % 32] for j in range(256)] for i in range(256)], dtype=np.int8)
    nw = sw.NeedlemanWunschScores(byte_to_class, costs, open=-3, extend=-3, capabilities=scope)
    shape = iter((24, 40) * 1000)
    on_device = False
    for arrangement, lay in placements(far, regime):
        for what, ta, tb, *where in forms(far, scope, lay, select=lambda r: r.window(next(shape)), raw32=False):
            queries, candidates = sides(lay, what[1], where)
            want = matrix_of(sw, orc, queries, candidates)
            got = lev(ta, tb, scope)
            assert (got == want).all(), (regime, arrangement, what, np.argwhere(got != want)[:5])
            scores = alignment_scores(orc, *expanded(queries, candidates), as_matrix, (-3, -3), False).reshape(want.shape)
            got = nw(ta, tb, scope)
            assert (got == scores).all(), ("nw", regime, arrangement, what, np.argwhere(got != scores)[:5])
            if what == ("raw u64", "2^32"):
                out = torch.full(want.shape, -7, dtype=torch.int64, device="cuda")
                lev(ta, tb, scope, out=out)
                assert (device_result(scope, out, np.int64) == want).all(), (regime, arrangement, "device out")
                out = torch.full(want.shape, -7, dtype=torch.int64, device="cuda")
                nw(ta, tb, scope, out=out)
                assert (device_result(scope, out, np.int64) == scores).all(), ("nw", regime, arrangement, "device out")
                on_device = True
    assert on_device


# ---- e. the searches ------------------------------------------------------------------------------------------------------------------
def search_forms(far, scope, lay):
    """(what, queries, candidates, their strings): 24 queries around a's threshold against the whole b side; and the same queries
    against themselves (candidates None)."""
    pick = iter((24, 1 << 30) * 1000)
    for what, tq, tc, *where in forms(far, scope, lay, select=lambda r: r.window(next(pick)), raw32=False):
        queries, candidates = sides(lay, what[1], where)
        yield what, tq, tc, queries, candidates
        if what[0] in ("raw u64", "prepared u64", "prepared u32", "sub-view of a spanning prepared tape"):
            yield (what[0] + ", self-search", what[1]), tq, None, queries, queries


@gpu
@pytest.mark.parametrize("regime", ["words", "lines"])
def test_topk(sw, orc, scope, far, lev, regime):
    """k = 1 and 5, with and without a bound: the fused kernel on the words (topk.hip), the general path on the lines."""
    import torch
    bound = 2 if regime == "words" else 40
    on_device = False
    for arrangement, lay in placements(far, regime):
        for what, tq, tc, queries, candidates in search_forms(far, scope, lay):
            d = matrix_of(sw, orc, queries, candidates)
            for k in (1, 5):
                for limit in (None, bound):
                    check_rows(lev.topk(tq, tc, scope, k=k, bound=limit), expected_topk(d, k, limit), (regime, arrangement, what, k, limit))
            if what == ("raw u64", "2^32") and arrangement == "inside":
                out = tuple(torch.full((d.shape[0], 5), -7, dtype=torch.int32, device="cuda") for _ in range(2))
                lev.topk(tq, tc, scope, k=5, out=out)
                check_rows([device_result(scope, x, np.uint32) for x in out], expected_topk(d, 5), (regime, arrangement, "device out"))
                on_device = True
    assert on_device


@gpu
@pytest.mark.parametrize("regime", ["words", "lines"])
def test_within(sw, orc, scope, far, lev, regime):
    """A bound of 2 on the words (the fused kernels of within.hip), of 40 on the lines (the general path)."""
    import torch
    bound = 2 if regime == "words" else 40
    on_device = False
    for arrangement, lay in placements(far, regime):
        for what, tq, tc, queries, candidates in search_forms(far, scope, lay):
            d = matrix_of(sw, orc, queries, candidates)
            want = expected_csr(d, bound)
            check_csr(lev.within(tq, tc, scope, bound=bound), want, (regime, arrangement, what))
            if what == ("raw u64", "2^32"):
                room = max(int(want[0][-1]), 1)
                out = (torch.full((d.shape[0] + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((room,), -7, dtype=torch.int32, device="cuda"),
                       torch.full((room,), -7, dtype=torch.int32, device="cuda"))
                lev.within(tq, tc, scope, bound=bound, out=out)
                scope.synchronize()
                check_csr(out, want, (regime, arrangement, "device out"))
                on_device = True
        assert int(want[0][-1]) > 0, (regime, arrangement)
    assert on_device


# ---- f. alignments and infix search ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("regime", ["tokens", "lines"])
def test_align(sw, orc, scope, far, lev, regime):
    """The distances, and every script replayed on the host strings: it turns a[k] into b[k] at the cost of the distance."""
    for arrangement, lay in placements(far, regime):
        for what, ta, tb, *where in forms(far, scope, lay, raw=False):
            a, b = sides(lay, what[1], where)
            want = levenshtein_of(sw, orc, a, b)
            got = lev.align(ta, tb, scope)
            assert (got.distances == want).all(), (regime, arrangement, what, np.nonzero(got.distances != want)[0][:5])
            errors = [(k, script_errors(a[k], b[k], got[k], int(want[k]))) for k in range(len(a))]
            assert not [e for e in errors if e[1]], (regime, arrangement, what, [e for e in errors if e[1]][:3])


@gpu
def test_infix(sw, scope, far, lev):
    """Patterns of at most 64 symbols (the tokens' a side, cut) in the lines' b side."""
    for arrangement, lay in placements(far, "infix"):
        remember("infix", [type("Case", (), {"a": lay[base][0].strings, "b": lay[base][1].strings}) for base in lay], False)
        for what, ta, tb, *where in forms(far, scope, lay, raw=False):
            a, b = sides(lay, what[1], where)
            got = lev.infix(ta, tb, scope)
            same("infix", np.stack([got.distances, got.starts, got.ends], axis=1).astype(np.int64), expected("infix", a, b, False), (arrangement, what))


# ---- g. OSA, LCS / Indel, Jaro --------------------------------------------------------------------------------------------------------
SCORED_REGIMES = {"words and tokens": ("words", "tokens"), "lines": ("lines",), "long": ("long",)}


@gpu
@pytest.mark.parametrize("regimes", list(SCORED_REGIMES))
@pytest.mark.parametrize("call", ["osa", "lcs", "jaro"])
def test_scored_families(sw, scope, far, lev, call, regimes):
    """Pairwise on the words, the tokens, the lines and the long pairs (their shorter side cut to 2048 symbols; both sides for Jaro);
    12 x 20 words as a cross-product; once with the results left on the device."""
    import torch
    on_device = False
    for regime in SCORED_REGIMES[regimes]:
        regime = {"long": "long_both" if call == "jaro" else "long_shorter"}.get(regime, regime)
        for arrangement, lay in placements(far, regime):
            remember(call, [type("Case", (), {"a": lay[base][0].strings, "b": lay[base][1].strings}) for base in lay], False)
            for what, ta, tb, *where in forms(far, scope, lay, raw=False):
                a, b = sides(lay, what[1], where)
                want = expected(call, a, b, False)
                same(call, run_pairs(call, lev, ta, tb, scope), want, (regime, arrangement, what))
                if what == ("prepared u64", "2^32") and regime == "tokens":
                    outs = [torch.full((len(a),), -7, dtype=torch.int32, device="cuda") for _ in range(want.shape[1])]
                    if call == "osa":
                        lev.osa(ta, tb, scope, out=outs[0])
                    elif call == "lcs":
                        lev.lcs(ta, tb, scope, out=outs[0]); lev.indel(ta, tb, scope, out=outs[1])
                    else:
                        lev.jaro_counts(ta, tb, scope, out=outs)
                    same(call, np.stack([device_result(scope, x, np.uint32).astype(np.int64) for x in outs], axis=1), want, (regime, arrangement, "device out"))
                    on_device = True
    if regimes != "words and tokens":
        return
    shape = iter((12, 20) * 1000)
    for arrangement, lay in placements(far, "words"):
        for what, tq, tc, *where in forms(far, scope, lay, select=lambda r: r.window(next(shape)), raw=False):
            queries, candidates = sides(lay, what[1], where)
            same(call, run_cross(call, lev, tq, tc, scope), expected(call, *expanded(queries, candidates), False), ("cross", arrangement, what))
    assert on_device


# ---- i. the score searches ----------------------------------------------------------------------------------------------------------
def search_counts(queries, candidates, utf8=False):
    return known(("search counts", utf8, tuple(queries), tuple(candidates)), lambda: counts_of(queries, candidates, utf8))


def check_searches(engine, scope, tq, tc, counts, what):
    """extract (k = 3) and extract_within (at the median score) of one form under all six scorers."""
    for scorer in SCORERS:
        scores, larger = reference_scores(scorer, counts), LARGER_IS_BETTER[scorer]
        assert_rows(extract_rows(engine, scope, tq, tc, scorer=scorer, k=3), expected_rows(scores, larger, 3), (what, scorer))
        cutoff = batch_cutoffs(scores, larger)[0]
        assert_csr(within_csr(engine, scope, tq, tc, scorer=scorer, cutoff=cutoff), expected_within(scores, larger, cutoff), (what, scorer, cutoff))


@gpu
@pytest.mark.parametrize("regime", ["words", "lines"])
def test_score_searches(sw, scope, far, lev, regime):
    """extract and extract_within: 12 queries x 20 candidates of the words around the threshold, 4 x 6 of the lines. The scoring kernels
    read a slice view while k_extract_select and the range search's kernel read the lengths from the whole tapes' offsets. Once with
    the outputs left on the device."""
    import torch
    shape = iter(((12, 20) if regime == "words" else (4, 6)) * 1000)
    on_device = False
    for arrangement, lay in placements(far, regime):
        for what, tq, tc, *where in forms(far, scope, lay, select=lambda r: r.window(next(shape)), raw32=False):
            queries, candidates = sides(lay, what[1], where)
            counts = search_counts(queries, candidates)
            check_searches(lev, scope, tq, tc, counts, (regime, arrangement, what))
            if what == ("raw u64", "2^32") and arrangement == "inside":
                scores = reference_scores("ratio", counts)
                rows = (torch.full((len(queries), 3), -7, dtype=torch.int32, device="cuda"), torch.full((len(queries), 3), 7.0, dtype=torch.float64, device="cuda"))
                lev.extract(tq, tc, scope, scorer="ratio", k=3, out=rows)
                assert_rows((device_result(scope, rows[0], np.uint32), device_result(scope, rows[1], np.uint64)), expected_rows(scores, True, 3), (regime, "device out"))
                cutoff = batch_cutoffs(scores, True)[0]
                want = expected_within(scores, True, cutoff)
                room = int(want[0][-1])
                out = (torch.full((len(queries) + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((room,), -7, dtype=torch.int32, device="cuda"),
                       torch.full((room,), 7.0, dtype=torch.float64, device="cuda"))
                lev.extract_within(tq, tc, scope, scorer="ratio", cutoff=cutoff, out=out)
                assert_csr((device_result(scope, out[0], np.uint64), device_result(scope, out[1], np.uint32), device_result(scope, out[2], np.uint64)), want,
                           (regime, "within, device out"))
                on_device = True
    assert on_device


# ---- j. partial_ratio -----------------------------------------------------------------------------------------------------------------
def partial_counts_of(a, b, utf8=False):
    return known(("partial", utf8, tuple(a), tuple(b)), lambda: partial_tests.expected(a, b, utf8))


@gpu
@pytest.mark.parametrize("regime", ["words", "tokens", "infix", "long_both", "long_near"])
def test_partial_ratio(sw, scope, far, lev, regime):
    """partial_counts pairwise: partial.hip cuts the haystack's windows into items by offsets of its own. Needles of one block (words),
    of 1 .. 3 (tokens), of at most 2 with hundreds of windows a pair (infix: the tokens' a side, cut, in the lines) and of 64 blocks, one
    window an item: at equal lengths, where both directions run (long_both), and 16 symbols under the haystack (long_near: the pair whose
    a side holds or begins at the threshold -- the reference takes 0.2 s for such a pair). 6 x 8 words as a cross-product."""
    for arrangement, lay in placements(far, regime):
        first = {id(r): regions[0].at for regions in lay.values() for r in regions}   # (both sides of a pairwise call take the same strings)
        select = (lambda r: (first[id(r)], 1)) if regime == "long_near" else (lambda r: (0, len(r.strings)))
        for what, ta, tb, *where in forms(far, scope, lay, select=select, raw=False):
            a, b = sides(lay, what[1], where)
            partial_tests.assert_counts(lev.partial_counts(ta, tb, scope), partial_counts_of(a, b), lambda k: (regime, arrangement, what, int(k)))
    if regime != "words":
        return
    shape = iter((6, 8) * 1000)
    for arrangement, lay in placements(far, "words"):
        for what, tq, tc, *where in forms(far, scope, lay, select=lambda r: r.window(next(shape)), raw=False):
            queries, candidates = sides(lay, what[1], where)
            want = partial_counts_of(*expanded(queries, candidates))
            partial_tests.assert_counts(lev.partial_counts_cross(tq, tc, scope), want, lambda k: ("cross", arrangement, what, int(k)))


# ---- k. token-sorted tapes ------------------------------------------------------------------------------------------------------------
def check_token_calls(engine, scope, ta, tb, a, b, utf8, what):
    """Both normal forms of both sides, derived on the device and read back; then token_sort_ratio, token_set_counts and token_set_ratio."""
    for tape, strings in ((ta, a), (tb, b)):
        for unique in (False, True):
            derived = tape.token_sorted(unique=unique)
            try:
                token_tests.assert_tape(derived.to_strs(), [token_tests.normal_form(x, unique) for x in strings])
            except AssertionError as wrong:
                raise AssertionError((what, unique)) from wrong
            derived.free()
    want = known(("tokens", utf8, tuple(a), tuple(b)), lambda: token_tests.reference(a, b, utf8))
    token_tests.check_scores(engine, scope, ta, tb, utf8, want=want)


@gpu
@pytest.mark.parametrize("regime", SPACED)
def test_token_sorted_tapes(sw, scope, far, lev, regime):
    """tokens.hip addresses a string through base + rel against the view's span and total, and stages "laid out like the source": the
    words, the tokens and the lines with every `t` a space, on every prepared form and the sub-views of the spanning tape. The
    spanning tape as a whole is refused: its filler string holds more than 4096 bytes."""
    refused = False
    for arrangement, lay in placements(far, regime):
        for what, ta, tb, *where in forms(far, scope, lay, raw=False):
            a, b = sides(lay, what[1], where)
            check_token_calls(lev, scope, ta, tb, a, b, False, (regime, arrangement, what))
        if "2^32" in lay and "above" in lay and not refused:
            whole, _ = far.spanning(lay, 0, scope)
            with pytest.raises(sw.StringWarsError) as refusal:
                whole.token_sorted()
            assert refusal.value.status == "unsupported_length", str(refusal.value)
            refused = True
    assert refused


# ---- l. the code-point engine on i, j and k ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("regime", ["words", "spaced_words"])
def test_searches_partial_and_tokens_utf8(sw, far, regime):
    """The code-point engine at its two bases, on prepared tapes (decoded once; freed form by form: the module's docstring): the
    searches on windows of 12 x 20 words and partial_ratio on the words, pairwise and 6 x 8; the token calls on the spaced words. The
    searches then run raw, one far tape against a small one (18.1 GiB: the docstring); partial_ratio and the token calls prepare the
    device tapes they are given, so for them a raw form would be the prepared one again."""
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope)
    try:
        for arrangement, lay in placements(far, regime, utf8=True):
            for what, ta, tb, *where in forms(far, scope, lay, raw=False, utf8=True, u32=UTF8_BASES):
                a, b = sides(lay, what[1], where, utf8=True)
                if regime == "spaced_words":
                    check_token_calls(engine, scope, ta, tb, a, b, True, (arrangement, what))
                else:
                    partial_tests.assert_counts(engine.partial_counts(ta, tb, scope), partial_counts_of(a, b, True), lambda k: (arrangement, what, int(k)))
                    for rows, columns, check in ((12, 20, "searches"), (6, 8, "partial")):
                        (fq, nq), (fc, nc) = lay[what[1]][0].window(rows), lay[what[1]][1].window(columns)
                        queries, candidates = a[fq:fq + nq], b[fc:fc + nc]
                        if check == "searches":
                            check_searches(engine, scope, ta[fq:fq + nq], tb[fc:fc + nc], search_counts(queries, candidates, True), (arrangement, what))
                        else:
                            partial_tests.assert_counts(engine.partial_counts_cross(ta[fq:fq + nq], tb[fc:fc + nc], scope),
                                                             partial_counts_of(*expanded(queries, candidates), True), lambda k: ("cross", arrangement, what, int(k)))
                ta.free(); tb.free()
            if regime != "words":
                continue
            # the searches' raw exports (utf8_u64tape), staged in the call: one far tape against a small one, as test_levenshtein_utf8 runs its raw form
            for base in lay:
                (fq, nq), (fc, nc) = lay[base][0].window(12), lay[base][1].window(20)
                counts = search_counts(*sides(lay, base, (fq, nq, fc, nc), utf8=True), True)
                for small_side in (1, 0):
                    tq, tc = far.tape(lay, base, 0, 64, fq, nq, small=small_side == 0), far.tape(lay, base, 1, 64, fc, nc, small=small_side == 1)
                    check_searches(engine, scope, tq, tc, counts, (arrangement, "raw, small side %d" % small_side, base))
    finally:
        del engine
        scope.close()


# ---- h. strings the windows cannot index are refused --------------------------------------------------------------------------------
@gpu
def test_a_string_of_2_to_the_30_symbols_is_refused(sw, scope, far, lev):
    """One string holds fewer than 2^30 bytes. Preparing a tape refuses a longer one on the offsets alone (the data pointer here is
    null: nothing may read it), for byte and UTF-8 tapes, in both widths; so do the calls that prepare their raw tapes. The pairwise
    and cross-product calls on raw tapes refuse it once the batch is measured, with nothing scored against the fill -- also a string of
    2^32 bytes or more, whose length does not fit the 32 bits the kernels hold it in; a string of 2^30 - 1 bytes is prepared. The engine and the scope go on working afterwards."""
    import ctypes as C
    from stringwars_amd import _native as N
    limit = 1 << 30
    for width, Tape, prepare in ((32, N.TapeU32, N.lib.swh_tape_prepare_u32), (64, N.TapeU64, N.lib.swh_tape_prepare_u64)):
        for lengths, refused in (((3, limit, 5), True), ((limit + 7,), True), ((3, limit - 1, 5), False)):
            offsets = far.offsets(np.concatenate([[16], 16 + np.cumsum(lengths)]), width)
            for utf8 in (0, 1) if refused else (0,):
                handle, err = C.c_void_p(), C.c_char_p()
                tape = Tape(None if refused else far.data[0].data_ptr(), offsets.data_ptr(), len(lengths))
                status = prepare(scope.handle, C.byref(tape), utf8, C.byref(handle), C.byref(err))
                assert N.STATUS_NAMES[status] == ("unsupported_length" if refused else "success"), (width, lengths, utf8, err.value)
                if refused:
                    assert b"fewer than 2^30" in err.value and not handle.value
                else:
                    N.lib.swh_prepared_free(handle)
    b = sw.DeviceTape.from_torch(far.data[1], far.offsets([0, 4, 8, 12], 64))
    nw = sw.NeedlemanWunschScores(*sw.unary_class_costs(2, -1), open=-2, extend=-2, capabilities=scope)
    # (2^32 and 2^32 + 4 bytes: cut to 32 bits they would be an empty string and one of four bytes, which scores without complaint)
    for length in (limit, (1 << 32) - 1, 1 << 32, (1 << 32) + 4):
        wrapping = sw.DeviceTape.from_torch(far.data[0], far.offsets([0, 4, length + 4, length + 8], 64))
        scope.forget()   # (no belief about lengths: the planned path, whose planner measures them)
        for believing in (False, True):   # ... and then with what the calls on `b` alone left the scope believing: the plan-free kernels' own checks
            for at, call in enumerate((lambda: lev.pairs(wrapping, b, scope), lambda: lev.pairs(b, wrapping, scope, bound=3), lambda: lev(wrapping, b, scope),
                                       lambda: lev(b, wrapping, scope), lambda: nw.pairs(wrapping, b, scope), lambda: nw(b, wrapping, scope))):
                with pytest.raises(sw.StringWarsError) as refusal:
                    call()
                    pytest.fail("not refused: length %d, believing %s, call %d" % (length, believing, at))
                assert refusal.value.status == "unsupported_length", (length, believing, str(refusal.value))
            assert (lev.pairs(b, b, scope) == 0).all() and (lev(b, b, scope) == 0).all() and (nw.pairs(b, b, scope) == 8).all()
        # tiled.hip takes any text under a pattern of up to 2048 symbols: on a scope that believes in strings of 40 bytes, and forced
        tiled = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")
        for engine in (lev, tiled):
            assert (engine.pairs([b"acgt" * 10] * 3, [b"tgca" * 10] * 3, scope) > 0).all()
            for call in (lambda: engine.pairs(wrapping, b, scope), lambda: engine.pairs(b, wrapping, scope)):
                with pytest.raises(sw.StringWarsError) as refusal:
                    call()
                assert refusal.value.status == "unsupported_length", (length, "tiled", str(refusal.value))
    long_a = sw.DeviceTape.from_torch(far.data[0], far.offsets([0, 4, limit + 4, limit + 8], 64))
    for call in (lambda: lev.pairs(long_a, b, scope), lambda: lev.pairs(b, long_a, scope, bound=3), lambda: lev(long_a, b, scope),
                 lambda: lev.topk(b, long_a, scope, k=1), lambda: lev.within(long_a, b, scope, bound=1), lambda: lev.osa(long_a, b, scope),
                 lambda: nw.pairs(long_a, b, scope)):
        with pytest.raises(sw.StringWarsError) as refusal:
            call()
        assert refusal.value.status == "unsupported_length", str(refusal.value)
    assert (lev.pairs(b, b, scope) == 0).all() and (lev.pairs([b"acgt", b"zzzz"], [b"acct", b"zzz"], scope) == [1, 1]).all()
