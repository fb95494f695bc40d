"""Tape sizes around the read widths of the alignment-score kernels and of the Levenshtein calls that test_tape_edges.py leaves out:
NW / SW scores, general-cost Levenshtein, Levenshtein cross-products and the fused range search, bounded and forced-algorithm pairs and
edit scripts -- on tapes of 0..80 bytes, on lopsided pairs of tapes, on views into larger prepared tapes and next to neighbours that
continue a string.

How the kernels under these calls read their strings, and so what the sizes straddle (the totals are those of the VIEW):
  * alignshort.hip (k_align_short w16 / w32 / w64, k_align_cross_wide w64 / w128, k_align_cross_long): `align_fetch<WORDS>` reads up
    to four 16-byte windows from a string's start -- `total >= 16`: one clamped 128-bit load each (ByteWindow::fetch16_raw), repaired
    by `fix16` where the clamp moved it (a string that ends within 16 x WORDS / 4 bytes of its tape's end); under 16 bytes dword loads
    realigned by a shift (fetch4_wide), under 4 bytes byte by byte (fetch4_tiny). The queries of the cross kernels are staged through
    ByteWindow::fetch4. The variant (16, 32, 64 columns) follows the longest string of both tapes;
  * wavefront.hip (the class-table, wide-table and 256 x 256 matrix kernels, and the cost kernel of general-cost Levenshtein):
    RowStream<uint8_t> prefetches dwords clamped into the tape, `tiny = total < 4` reads bytes; RowStream<uint32_t> clamps every code
    point's index; the column strings go through ByteWindow / SymWindow32 (`hi - lo >= 3` for tapes under four symbols);
  * nwprofile.hip: pairs of more than 384 columns on a class or wide table, the same windows;
  * cross.hip (`b_total >= 16`: 128-bit candidate loads, else dwords; the queries are staged bytewise) and within.hip (the same
    branch on both of its passes, count and fill);
  * banded.hip: batched unaligned dword loads of both strings; align.hip: the blocks' windows of the edit-script kernels.
The sizes below straddle 4 and 16 on either tape independently, with the first and last strings touching the tapes' ends. Where a
stamp tells the variants apart (`align_short..w16`, `align_wide..w128`, `nwprofile..`, `banded`, `cross_short`) the tests assert that the
sweep reached it, and print every other name they met.

Every comparison is exact (==): scores against oracle.nw_score / oracle.nw_pairs, distances against oracle.levenshtein_pairs and
oracle.levenshtein_costs_pairs, scripts through test_align.py's check_valid_batch / check_exact. Each reference is computed once and
shared. The one CPU test runs the generators alone and asserts what the sweeps hold -- above all that every neighbour case of section
f would change its reference score if a neighbour's symbols were read."""
import contextlib
import functools
from collections import namedtuple

import numpy as np
import pytest

from conftest import run_in_child
from test_align import check_exact, check_valid_batch, code_point_tape, same_alignments
from test_tape_edges import (FOUR_BYTE, OTHERS, SHORT_TOTALS, SIZES, VIEW_SIZES, WIDE_LETTERS, as_items, combinations, cross_sweep, csr_of, cut,
                             expanded, make_sweep, pair_sweep, random_tape, symbol_cross_sweep, symbol_sweep, tape_bytes)

gpu = pytest.mark.gpu

LETTERS8 = "abcdefgh"                      # one symbol class each in every scoring model below
LETTERS12 = "abcdefghijkl"                 # more classes than k_align_cross_wide takes per item: it refuses some items, the call is redone
DNA = "ACGT"
GAPS = ((-2, -2), (-5, -1))                # linear, affine
NEIGHBOUR_GAPS = ((-2, -2), (-5, -1), (-11, -1))
MODELS = ("classes8", "classes32", "wide", "matrix")
CLASS_MODELS = ("classes8", "classes32")
FORM_GROUPS = ("raw", "device", "prepared")
COSTS = ((0, 2, 3, 3), (1, 3, 4, 2))       # general-cost Levenshtein: linear and affine gaps
LOPSIDED_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 129, 385, 513, 1100)
PROFILE_LENGTHS = tuple(n for n in LOPSIDED_LENGTHS if n >= 385)   # more than nwprofile's 384 columns
BOUNDS = (0, 1, 3, 31, 63, 100)
WITHIN_BOUNDS = (0, 2, 40)
EDGE_PAIR_LENGTHS = (16, 32, 64)           # |x + t|: the first symbol past the string is the first column of the next window

Scoring = namedtuple("Scoring", "byte_to_class costs full")


def orc():
    import oracle
    return oracle


# ---- the scoring models -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scoring(model) -> Scoring:
    """Asymmetric random int8 costs in [-9, 11]. `classes8`, `classes32`: a byte -> class map and 32 x 32 class costs (8 and 32 classes
    in use); `wide`: a 256 x 256 matrix that folds into 100 classes (the wide table); `matrix`: one that folds into none (the LDS
    matrix kernel). `unary`, `positive`: section f's tables, a strictly positive diagonal over strictly negative costs."""
    rng = np.random.default_rng(9100 + sum(map(ord, model)))
    if model == "matrix":
        return Scoring(None, None, rng.integers(-9, 12, (256, 256)).astype(np.int8))
    classes = {"classes8": 8, "classes32": 32, "wide": 100, "unary": 32, "positive": 32}[model]
    byte_to_class = (np.arange(256) % classes).astype(np.uint8)
    if model == "unary":
        costs = np.where(np.eye(classes, dtype=bool), 2, -1).astype(np.int8)
    elif model == "positive":
        costs = rng.integers(-9, 0, (classes, classes)).astype(np.int8)
        costs[np.arange(classes), np.arange(classes)] = rng.integers(1, 12, classes)
    else:
        costs = rng.integers(-9, 12, (classes, classes)).astype(np.int8)
    full = costs[byte_to_class][:, byte_to_class].astype(np.int8)
    if classes > 32:
        return Scoring(None, None, full)
    table = np.zeros((32, 32), dtype=np.int8)
    table[:classes, :classes] = costs
    return Scoring(byte_to_class, table, full)


def classes_of(full) -> int:
    """Into how many symbol classes a matrix folds: bytes whose rows and columns coincide are one class."""
    return len({(full[b].tobytes(), full[:, b].tobytes()) for b in range(256)})


def engine_of(sw, scope, model, local, gaps):
    Engine = sw.SmithWatermanScores if local else sw.NeedlemanWunschScores
    s = scoring(model)
    if s.byte_to_class is None:
        return Engine(substitution_matrix=s.full, open=gaps[0], extend=gaps[1], capabilities=scope)
    return Engine(s.byte_to_class, s.costs, open=gaps[0], extend=gaps[1], capabilities=scope)


# ---- the references, computed once per pair -----------------------------------------------------------------------------------------
_scores = {}


def want_scores(model, local, gaps, xs, ys) -> np.ndarray:
    full, out = scoring(model).full, []
    for x, y in zip(xs, ys):
        key = (model, local, gaps, x, y)
        if key not in _scores:
            _scores[key] = orc().nw_score(x, y, full, gaps[0], gaps[1], local=local)
        out.append(_scores[key])
    return np.array(out, dtype=np.int64)


RENAME = {ch: bytes([65 + i]) for i, ch in enumerate(dict.fromkeys(WIDE_LETTERS + FOUR_BYTE))}


def byte_symbols(x) -> bytes:
    """The costs oracle scores bytes, and a distance depends on the symbols only through equality: every code point renamed to a byte."""
    return x if isinstance(x, bytes) else b"".join(RENAME[ch] for ch in x)


_distances = {}


def want_distances(costs, xs, ys, utf8) -> np.ndarray:
    """General-cost (`costs` a tuple) or unit-cost (None) Levenshtein distances of the pairs, one batched oracle call for the new ones."""
    import stringwars_amd as sw
    missing = list(dict.fromkeys((x, y) for x, y in zip(xs, ys) if (costs, x, y) not in _distances))
    if missing:
        if costs is None:   # the unit-cost oracle decodes UTF-8 itself: it gets the strings as they are
            got = orc().levenshtein_pairs(sw.Strs([x for x, _ in missing]), sw.Strs([y for _, y in missing]), utf8=utf8)
        else:
            got = orc().levenshtein_costs_pairs(sw.Strs([byte_symbols(x) for x, _ in missing]), sw.Strs([byte_symbols(y) for _, y in missing]), *costs)
        for pair, d in zip(missing, got):
            _distances[(costs,) + pair] = int(d)
    return np.array([_distances[(costs, x, y)] for x, y in zip(xs, ys)], dtype=np.int64)


def same(got, want, describe):
    got = np.asarray(got).astype(np.int64).ravel()
    assert got.shape == want.shape, (describe, got.shape, want.shape)
    wrong = np.nonzero(got != want)[0]
    assert not len(wrong), [(describe, int(k), int(got[k]), int(want[k])) for k in wrong[:5]]


# ---- the generators -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_pair_sweep():
    return make_sweep(9101, False, SIZES, OTHERS, LETTERS8, True, (1, 4), None)


@functools.lru_cache(maxsize=None)
def score_cross_sweep(alphabet):
    return make_sweep(9102 + len(alphabet), False, SIZES, OTHERS, alphabet, True, (1, 4), (1, 5))


def pair_cases(kind):
    """Sweep (a)'s cases: `bytes` over eight letters, `utf8` over pair_sweep(True)'s alphabet, `symbols`: four-byte characters."""
    return {"bytes": score_pair_sweep, "utf8": lambda: pair_sweep(True), "symbols": symbol_sweep}[kind]()


def longest(items) -> int:
    return max(len(x) for x in items)


def related(rng, s, length, alphabet):
    """`length` symbols that hold `s` over and over, a few of them changed: an alignment that is no mere run of gaps."""
    base = list((s * (length // max(len(s), 1) + 1))[:length] if s else "".join(random_tape(rng, length, alphabet, True)))
    for at in rng.integers(0, length, int(rng.integers(1, 6))):
        base[int(at)] = alphabet[int(rng.integers(0, len(alphabet)))]
    return "".join(base)


@functools.lru_cache(maxsize=None)
def lopsided_cases(alphabet):
    """(short total, long length, the small tape's strings, the other tape's one string): one or two strings that total 0, 1, 3, 4 or
    15 bytes against a single string that is its whole tape."""
    rng = np.random.default_rng(9110 + len(alphabet))
    cases = []
    for total in SHORT_TOTALS:
        for at, length in enumerate(LOPSIDED_LENGTHS):
            small = cut(rng, random_tape(rng, total, alphabet, True), 1 + (at + total) % 2, False)
            cases.append((total, length, as_items(small, False), as_items([related(rng, small[-1], length, alphabet)], False)))
    return cases


@functools.lru_cache(maxsize=None)
def profile_cases():
    """(length, [x], [y]): two equally long single-string tapes of more than 384 bytes -- both strings touch both ends of their tapes."""
    rng = np.random.default_rng(9111)
    cases = []
    for length in PROFILE_LENGTHS:
        x = "".join(random_tape(rng, length, LETTERS8, True))
        cases.append((length, as_items([x], False), as_items([related(rng, x, length, LETTERS8)], False)))
    return cases


@functools.lru_cache(maxsize=None)
def placed_views(kind):
    """(size, trial, position, tape a, tape b, first, count): the diagonal cases of VIEW_SIZES between junk strings of the same letters
    -- at the start (the view ends below 16 bytes in a large tape), in the middle, and at the tail, as test_tape_edges.view_cases."""
    rng = np.random.default_rng(9120 + len(kind))
    utf8 = kind != "bytes"
    alphabet = WIDE_LETTERS if utf8 else LETTERS8
    junk = lambda count: as_items(["".join(random_tape(rng, int(rng.integers(4, 24)), alphabet, False)) for _ in range(count)], utf8)
    cases = []
    for case in pair_cases(kind):
        if case.total_a == case.total_b and case.total_a in VIEW_SIZES:
            for position in ("start", "middle", "tail"):
                before, after = 0 if position == "start" else 5, 0 if position == "tail" else 5
                front_a, front_b, back_a, back_b = junk(before), junk(before), junk(after), junk(after)
                cases.append((case.total_a, case.trial, position, front_a + case.a + back_a, front_b + case.b + back_b, before, len(case.a)))
    return cases


Neighbour = namedtuple("Neighbour", "x t direction mirrored position small a b")


@functools.lru_cache(maxsize=None)
def neighbour_pairs():
    """(x, t): 1 .. 7 symbols followed (or preceded) by 1 .. 4, and pairs whose longer string ends exactly on a 16-, 32- or 64-column
    variant."""
    rng = np.random.default_rng(9130)
    word = lambda n: "".join(random_tape(rng, n, LETTERS8, True))
    lengths = [(nx, nt) for nx in range(1, 8) for nt in range(1, 5)] + [(edge - nt, nt) for edge in EDGE_PAIR_LENGTHS for nt in range(1, 5)]
    return [(word(nx), word(nt)) for nx, nt in lengths]


@functools.lru_cache(maxsize=None)
def neighbour_cases():
    """Tapes of three strings (two where the pair is first or last) whose neighbours WOULD show if they were read. `a` holds x between a
    predecessor that ends in t and a successor that begins with t. Forwards, `b` holds x + t followed by the junk that follows t in `a`:
    from the first byte of the pair onwards both tapes hold the same bytes, and a read past x's end meets the very symbols that x + t
    goes on with. Backwards, `b` holds t + x behind the junk that precedes t in `a`. Mirrored: the roles of a and b swapped. The pair
    stands first, in the middle and last, with no junk (tapes under 16 bytes) and with 20 to 28 bytes of it on either side."""
    rng = np.random.default_rng(9131)
    junk = lambda n: "".join(random_tape(rng, n, LETTERS8, True))
    cases = []
    for x, t in neighbour_pairs():
        for direction in ("forwards", "backwards"):
            for small in (True, False):
                if small and 2 * len(t) + len(x) >= 16:
                    continue
                before, after, other = ("", "", "") if small else (junk(int(rng.integers(20, 29))) for _ in range(3))
                for position in range(3):
                    a = [before + t, x, t + after]
                    if direction == "forwards":
                        b = [other[:15 - len(x + t)] if small else other, x + t, after]
                    else:
                        b = [before, t + x, other[:15 - len(x + t)] if small else other]
                    a, b = (side[1:] if position == 0 else side[:2] if position == 2 else side for side in (a, b))
                    a, b = as_items(a, False), as_items(b, False)
                    for mirrored in (False, True):
                        cases.append(Neighbour(x, t, direction, mirrored, position, small, *((b, a) if mirrored else (a, b))))
    return cases


def over_reads(x, t, direction, junk):
    """What a kernel that read past the short string would score instead of (x, x + t): x with 1 .. |t| of its neighbour's symbols,
    alone and with as many of the long string's own neighbour. (short, long) pairs."""
    out = []
    for k in range(1, len(t) + 1):
        if direction == "forwards":
            out += [(x + t[:k], x + t), (x + t[:k], x + t + junk[:k])]
        else:
            out += [(t[len(t) - k:] + x, t + x), (t[len(t) - k:] + x, junk[len(junk) - k:] + t + x)]
    return list(dict.fromkeys(out))


# ---- running a call in its forms ----------------------------------------------------------------------------------------------------
class Names:
    """The `dominant_name`s a sweep met, per form."""

    def __init__(self, scope):
        self.scope, self.seen = scope, {}

    def note(self, form):
        name = self.scope.last_timing()["dominant_name"]
        if name:
            self.seen.setdefault(form, set()).add(name)

    def of(self, *forms):
        return set().union(*(self.seen.get(form, set()) for form in forms))

    def need(self, forms, wanted, what):
        """Every entry of `wanted` -- a tuple of (prefix, suffix) -- matches a name met in `forms`."""
        met = self.of(*forms)
        missing = [w for w in wanted if not any(name.startswith(w[0]) and name.endswith(w[1]) for name in met)]
        assert not missing, (what, "not reached:", missing, "reached:", {form: sorted(names) for form, names in self.seen.items()})

    def __str__(self):
        return "; ".join("%s: %s" % (form, ", ".join(sorted(names))) for form, names in self.seen.items())


@contextlib.contextmanager
def profiled(scope, report=None):
    names = Names(scope)
    scope.set_profiling(True)
    try:
        yield names
    finally:
        scope.set_profiling(False)
    if report is not None:
        print("\n[names] %s -> %s" % (report, names))


def in_forms(sw, scope, group, a, b, utf8, run, trial=0, widths=(np.uint32, np.uint64)):
    """`run(form, tape a, tape b)` in the forms of one group. `raw`: host tapes on a scope that believes nothing (the planned path),
    then the same call again (the scope believes the lengths it saw); `device`: device tapes, on every other case after a forget();
    `prepared`: PreparedTapes (guaranteed lengths), with 32- and with 64-bit offsets. `b` None: a self-product."""
    sa, sb = sw.Strs(a), None if b is None else sw.Strs(b)
    if group == "raw":
        scope.forget()
        run("nothing believed", sa, sb)
        run("believed", sa, sb)
    elif group == "device":
        da, db = sa.to_device(scope), None if sb is None else sb.to_device(scope)
        if trial:
            scope.forget()
        run("device", da, db)
    else:
        for width in widths:
            pa = sw.PreparedTape(scope, sa.with_offsets(width), utf8=utf8)
            run(width.__name__, pa, None if sb is None else sw.PreparedTape(scope, sb.with_offsets(width), utf8=utf8))


PREPARED = ("uint32", "uint64")


# ---- a. the size sweep, pairwise ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("group", FORM_GROUPS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
def test_size_sweep_score_pairs(sw, scope, local, model, group):
    """NW / SW scores on tapes of SIZES bytes against tapes of the same size, of 3, 15, 16 and 80 bytes, in both orders, linear and
    affine gaps. The planned path (nothing believed) runs the wavefront kernels: RowStream's `tiny` under 4 bytes of row tape, the
    clamped windows above. A scope that believes the lengths, and prepared tapes, run k_align_short on a class table: align_fetch's
    `total >= 16` is per tape, its 16 / 32 / 64 columns follow the longest string of both tapes -- all three occur here."""
    engines = [(gaps, engine_of(sw, scope, model, local, gaps)) for gaps in GAPS]
    with profiled(scope, ("pairs", "sw" if local else "nw", model, group)) as names:
        for case in score_pair_sweep():
            for gaps, engine in engines:
                want = want_scores(model, local, gaps, case.a, case.b)

                def run(form, ta, tb):
                    got = engine.pairs(ta, tb, scope)
                    names.note(form)
                    same(got, want, (form, gaps, case.total_a, case.total_b, case.trial, case.a, case.b))
                in_forms(sw, scope, group, case.a, case.b, False, run, case.trial)
    if group == "raw":
        names.need(["nothing believed"], [("wavefront", "")], (model, "the planned path"))
        if model in CLASS_MODELS:
            names.need(["believed"], [("align_short", "")], (model, "a scope that believes the lengths"))
    if group == "prepared" and model in CLASS_MODELS:
        for form in PREPARED:
            names.need([form], [("align_short", "w16"), ("align_short", "w32"), ("align_short", "w64")], (model, form))


@gpu
@pytest.mark.parametrize("group", FORM_GROUPS)
@pytest.mark.parametrize("kind", ["bytes", "utf8", "symbols"])
@pytest.mark.parametrize("costs", COSTS, ids=["linear", "affine"])
def test_size_sweep_general_cost_pairs(sw, scope, costs, kind, group):
    """General-cost Levenshtein on the wavefront cost kernel through the same sweep, unbounded and with bound=2: over bytes
    (RowStream<uint8_t>), over code points (RowStream<uint32_t>, every index clamped on its own) and over tapes of 0 .. 8 four-byte
    characters (SymWindow32's branch for tapes under four symbols)."""
    utf8 = kind != "bytes"
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(*costs, capabilities=scope)
    with profiled(scope, ("general-cost pairs", costs, kind, group)) as names:
        for case in pair_cases(kind):
            want = want_distances(costs, case.a, case.b, utf8)
            for bound in (None, 2):
                def run(form, ta, tb):
                    got = engine.pairs(ta, tb, scope, bound=bound)
                    names.note(form)
                    same(got, want if bound is None else np.minimum(want, bound + 1), (form, bound, case.total_a, case.total_b, case.trial, case.a, case.b))
                in_forms(sw, scope, group, case.a, case.b, utf8, run, case.trial)
    if group == "raw" and not utf8:   # (a small call over code points is named after its staging or its planner)
        names.need(["nothing believed"], [("wavefront", "")], (costs, kind))


# ---- b. the size sweep, cross-products ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("group", FORM_GROUPS)
@pytest.mark.parametrize("alphabet", [LETTERS12, DNA], ids=["letters", "dna"])
@pytest.mark.parametrize("gaps", GAPS, ids=["linear", "affine"])
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
def test_size_sweep_score_cross(sw, scope, local, gaps, alphabet, group):
    """The same sizes with 1 .. 4 queries against 1 .. 5 candidates on the 32-class table, and the self-product of the queries. Over
    twelve letters k_align_cross_wide refuses the items that hold more than eight classes and the call is redone on the planned path;
    over DNA it keeps them: a tape of 33 .. 80 bytes that holds one string longer than 32 runs its 64-column variant, one longer than
    64 the 128-column one (linear gaps, prepared tapes)."""
    engine = engine_of(sw, scope, "classes32", local, gaps)   # (of this test alone: the scope remembers per engine that the wide kernel refused)
    with profiled(scope, ("cross", "sw" if local else "nw", gaps, alphabet, group)) as names:
        for case in score_cross_sweep(alphabet):
            for what, candidates in (("cross", case.b), ("self", None)):
                want = want_scores("classes32", local, gaps, *expanded(case.a, case.a if candidates is None else candidates))

                def run(form, tq, tc):
                    got = engine(tq, tc, scope)
                    names.note(form)
                    same(got, want, (what, form, alphabet, case.total_a, case.total_b, case.trial, case.a, case.b))
                in_forms(sw, scope, group, case.a, candidates, False, run, case.trial, widths=(np.uint64,))
    if group == "prepared" and alphabet == DNA:
        names.need(["uint64"], [("align_short", "")], "word-sized DNA")
        if gaps[0] == gaps[1]:
            names.need(["uint64"], [("align_wide", "w64"), ("align_wide", "w128")], "DNA strings of 33 .. 80 bytes")


@gpu
@pytest.mark.parametrize("group", FORM_GROUPS)
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_size_sweep_levenshtein_cross(sw, scope, utf8, group):
    """Unit-cost Levenshtein `engine(queries, candidates)` and the self-product: cross.hip reads its candidates with 128-bit loads
    where `b_total >= 16` and with dwords below, and stages its queries bytewise. Word-sized prepared tapes run k_cross_short."""
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
    cases = cross_sweep(utf8) + (symbol_cross_sweep() if utf8 else [])
    with profiled(scope, ("levenshtein cross", "utf8" if utf8 else "bytes", group)) as names:
        for case in cases:
            for what, candidates in (("cross", case.b), ("self", None)):
                want = want_distances(None, *expanded(case.a, case.a if candidates is None else candidates), utf8)

                def run(form, tq, tc):
                    got = engine(tq, tc, scope)
                    names.note(form)
                    same(got, want, (what, form, case.total_a, case.total_b, case.trial, case.a, case.b))
                in_forms(sw, scope, group, case.a, candidates, utf8, run, case.trial, widths=(np.uint64,))
    if group == "prepared":
        names.need(["uint64"], [("cross_short", "")], "word-sized prepared tapes")


@gpu
@pytest.mark.parametrize("group", FORM_GROUPS)
@pytest.mark.parametrize("what", ["cross", "self"])
@pytest.mark.parametrize("bound", WITHIN_BOUNDS)
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_size_sweep_within(sw, scope, utf8, bound, what, group):
    """The range search on the same cases, and the self-search of their queries: offsets, indices and distances against the dense
    oracle matrix, rows in candidate order. The fused kernel (within.hip) takes word-sized byte tapes and has cross.hip's
    `b_total >= 16` branch on both of its passes, the count and the fill; everything else scores blocks on the cross-product routes."""
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
    cases = cross_sweep(utf8) + (symbol_cross_sweep() if utf8 else [])
    with profiled(scope, ("within", "utf8" if utf8 else "bytes", bound, what, group)) as names:
        for case in cases:
            candidates = None if what == "self" else case.b
            others = case.a if candidates is None else candidates
            dense = want_distances(None, *expanded(case.a, others), utf8).reshape(len(case.a), len(others))
            want = csr_of(dense, bound)

            def run(form, tq, tc):
                got = engine.within(tq, tc, scope, bound=bound)
                names.note(form)
                describe = (what, form, bound, case.total_a, case.total_b, case.trial, case.a, case.b)
                assert np.asarray(got.offsets).tolist() == want[0].tolist(), describe
                assert np.asarray(got.indices).tolist() == want[1].tolist() and np.asarray(got.distances).tolist() == want[2].tolist(), describe
            in_forms(sw, scope, group, case.a, candidates, utf8, run, case.trial, widths=(np.uint64,))
    if group == "prepared" and not utf8:
        names.need(["uint64"], [("cross_within", "")], "word-sized prepared byte tapes")


# ---- c. lopsided tapes --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("model", ["classes32", "wide", "matrix"])
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
def test_lopsided_score_pairs(sw, scope, local, model):
    """One tape of 0 .. 15 bytes against a single string of up to 1100 bytes that is its whole tape, in both orders: the planned
    wavefront kernels get many rows (or columns) against a tiny tape -- a small tape of one string as a pair, one of two strings as a
    cross-product on raw tapes, which plans the same kernels. Then two equally long single-string tapes of 385 bytes and more: the
    column-profile kernel (class and wide tables) with both strings touching both ends of their tapes."""
    with profiled(scope, ("lopsided pairs", "sw" if local else "nw", model)) as names:
        for gaps in GAPS:
            engine = engine_of(sw, scope, model, local, gaps)
            for total, length, small, large in lopsided_cases(LETTERS8):
                for a, b in ((small, large), (large, small)):
                    want = want_scores(model, local, gaps, *expanded(a, b))

                    def run(form, ta, tb):
                        got = engine.pairs(ta, tb, scope) if len(small) == 1 else engine(ta, tb, scope)
                        names.note(form)
                        same(got, want, (form, gaps, total, length, len(a[0]), len(b[0])))
                    in_forms(sw, scope, "raw", a, b, False, run)
                    if len(small) == 1:
                        in_forms(sw, scope, "prepared", a, b, False, run, widths=(np.uint64,))
    with profiled(scope, ("equally long pairs", "sw" if local else "nw", model)) as long_names:
        for gaps in GAPS:
            engine = engine_of(sw, scope, model, local, gaps)
            for length, x, y in profile_cases():
                want = want_scores(model, local, gaps, x, y)

                def run(form, ta, tb):
                    got = engine.pairs(ta, tb, scope)
                    long_names.note(form)
                    same(got, want, (form, gaps, length))
                in_forms(sw, scope, "raw", x, y, False, run)
                in_forms(sw, scope, "prepared", x, y, False, run, widths=(np.uint64,))
    if model != "matrix":
        long_names.need(["nothing believed", "believed", "uint64"], [("nwprofile", "")], (model, "385 bytes and more"))


@gpu
@pytest.mark.parametrize("gaps", GAPS, ids=["linear", "affine"])
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
def test_lopsided_score_cross(sw, scope, local, gaps):
    """Prepared tapes over ACGT: k_align_cross_long stages its queries through ByteWindow::fetch4 and reads its candidates through
    align_fetch in passes -- with a tiny query tape under a long candidate, and with a tiny candidate tape under a long query."""
    engine = engine_of(sw, scope, "classes32", local, gaps)
    orders = {}
    for order in ("tiny queries", "tiny candidates"):
        with profiled(scope, ("lopsided cross", "sw" if local else "nw", gaps, order)) as names:
            for total, length, small, large in lopsided_cases(DNA):
                q, c = (small, large) if order == "tiny queries" else (large, small)
                want = want_scores("classes32", local, gaps, *expanded(q, c))

                def run(form, tq, tc):
                    got = engine(tq, tc, scope)
                    names.note(form)
                    same(got, want, (order, form, total, length))
                in_forms(sw, scope, "prepared", q, c, False, run, widths=(np.uint64,))
        orders[order] = names
    for order, names in orders.items():
        names.need(["uint64"], [("align_long", "")], order)


# ---- d. bounded, forced and scripted Levenshtein ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("group", ["raw", "prepared"])
@pytest.mark.parametrize("bounds", [BOUNDS[:3], BOUNDS[3:]], ids=["0-1-3", "31-63-100"])
@pytest.mark.parametrize("kind", ["bytes", "utf8"])
def test_size_sweep_bounded_pairs(sw, scope, kind, bounds, group):
    """`pairs(..., bound=k)` on sweep (a): a string of more than 32 symbols on a tape of at most 80 bytes reaches banded.hip's batched
    unaligned dword loads at both ends of its tape."""
    utf8 = kind != "bytes"
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
    cases = pair_cases(kind) + (symbol_sweep() if utf8 else [])
    with profiled(scope, ("bounded pairs", kind, bounds, group)) as names:
        for case in cases:
            want = want_distances(None, case.a, case.b, utf8)
            for bound in bounds:
                def run(form, ta, tb):
                    got = engine.pairs(ta, tb, scope, bound=bound)
                    names.note(form)
                    same(got, np.minimum(want, bound + 1), (form, bound, case.total_a, case.total_b, case.trial, case.a, case.b))
                in_forms(sw, scope, group, case.a, case.b, utf8, run, widths=(np.uint64,))
    # (no name is asked for here: a call is named after the longest of its stamps, the planner's among them, and next to a band of a
    # few cells on one to four pairs the planner takes longer on some machines and not on others -- the test below reads every stamp)


@gpu
@pytest.mark.parametrize("kind", ["bytes", "utf8"])
def test_bounded_sweep_reaches_the_banded_kernel(request, capfd, sw, scope, kind):
    """That sweep (d) runs banded.hip at all: STRINGWARS_AMD_STAMPS=1, which the library reads once per process, makes it list EVERY
    stamp of a profiled call on stderr, whichever took longest -- so the cases that hold a string of more than 32 symbols run once more
    in a child process, and `banded` must be among the stamps. The message says under which bounds and forms it was."""
    if not run_in_child(request, env={"STRINGWARS_AMD_STAMPS": "1"}, timeout=300):
        return
    utf8 = kind != "bytes"
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
    cases = [c for c in pair_cases(kind) if max(longest(c.a), longest(c.b)) > 32]
    assert len(cases) >= 50
    reached = {}
    with profiled(scope):
        for bound in BOUNDS:
            for group in ("raw", "prepared"):
                capfd.readouterr()
                for case in cases:
                    want = np.minimum(want_distances(None, case.a, case.b, utf8), bound + 1)
                    in_forms(sw, scope, group, case.a, case.b, utf8, lambda form, ta, tb: same(engine.pairs(ta, tb, scope, bound=bound), want, (form, bound, case.a, case.b)),
                             widths=(np.uint64,))
                stamps = {line.split()[2] for line in capfd.readouterr().err.splitlines() if line.startswith("[swh] stamp ")}
                assert stamps, "no stamps on stderr: STRINGWARS_AMD_STAMPS was not in force"
                reached[(bound, group)] = "banded" in stamps
    assert any(reached.values()), reached
    print("\n[names] banded reached under (bound, form):", sorted(key for key, hit in reached.items() if hit))


@gpu
@pytest.mark.parametrize("kind", ["bytes", "utf8"])
@pytest.mark.parametrize("algorithm", ["wavefront", "bitparallel", "tiled"])
def test_size_sweep_forced_algorithms(sw, scope, algorithm, kind):
    """Plain pairs under each forced algorithm, unbounded: raw tapes twice (planned, then on believed lengths) and prepared tapes."""
    utf8 = kind != "bytes"
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope, algorithm=algorithm)
    cases = pair_cases(kind) + (symbol_sweep() if utf8 else [])
    with profiled(scope, ("forced", algorithm, kind)) as names:
        for case in cases:
            want = want_distances(None, case.a, case.b, utf8)

            def run(form, ta, tb):
                got = engine.pairs(ta, tb, scope)
                names.note(form)
                same(got, want, (algorithm, form, case.total_a, case.total_b, case.trial, case.a, case.b))
            in_forms(sw, scope, "raw", case.a, case.b, utf8, run)
            in_forms(sw, scope, "prepared", case.a, case.b, utf8, run, widths=(np.uint64,))
    names.need(["nothing believed", "believed", "uint64"],
               [({"wavefront": "wavefront", "bitparallel": "bitparallel", "tiled": "bitparallel_tiled"}[algorithm], "")], algorithm)


@gpu
@pytest.mark.parametrize("bound", [None, 3])
@pytest.mark.parametrize("kind", ["bytes", "utf8"])
def test_size_sweep_edit_scripts(sw, scope, kind, bound):
    """`engine.align` on sweep (a): exact distances, and scripts that are valid and the canonical ones, from raw and from prepared
    tapes alike."""
    utf8 = kind != "bytes"
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
    for case in pair_cases(kind) + (symbol_sweep() if utf8 else []):
        describe = (bound, case.total_a, case.total_b, case.trial, case.a, case.b)
        sa, sb = sw.Strs(case.a), sw.Strs(case.b)
        got = engine.align(sa, sb, scope, bound=bound)
        want = want_distances(None, case.a, case.b, utf8)
        same(got.distances, want if bound is None else np.minimum(want, bound + 1), describe)
        check_exact(sw, got, case.a, case.b, utf8=utf8, bound=bound)
        if bound is None:
            check_valid_batch(*((code_point_tape(case.a), code_point_tape(case.b)) if utf8 else ((sa.data, sa.offsets), (sb.data, sb.offsets))), got, utf8=utf8)
        prepared = engine.align(sw.PreparedTape(scope, sa, utf8=utf8), sw.PreparedTape(scope, sb, utf8=utf8), scope, bound=bound)
        assert same_alignments(prepared, got), ("prepared",) + describe


# ---- e. views into a larger prepared tape -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
def test_score_views_into_a_larger_tape(sw, scope, local):
    """The tape total a kernel sees is offsets[first + count] of the VIEW: class-table pairs on a view at the start of a large prepared
    tape (under 16 bytes of it), in the middle between junk strings, and at the tail, where the last string ends where the buffer ends."""
    engines = [(gaps, engine_of(sw, scope, "classes32", local, gaps)) for gaps in GAPS]
    for size, trial, position, a, b, first, count in placed_views("bytes"):
        pa, pb = sw.PreparedTape(scope, sw.Strs(a)), sw.PreparedTape(scope, sw.Strs(b))
        for gaps, engine in engines:
            want = want_scores("classes32", local, gaps, a[first:first + count], b[first:first + count])
            same(engine.pairs(pa[first:first + count], pb[first:first + count], scope), want, (gaps, size, trial, position, a, b))


@gpu
@pytest.mark.parametrize("kind", ["bytes", "utf8"])
def test_levenshtein_views_into_a_larger_tape(sw, scope, kind):
    """The same views under general-cost pairs and under the unit-cost cross-product, with views on both sides."""
    utf8 = kind != "bytes"
    Engine = sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances
    costly, unit = [Engine(*costs, capabilities=scope) for costs in COSTS], Engine(capabilities=scope)
    for size, trial, position, a, b, first, count in placed_views(kind):
        pa, pb = sw.PreparedTape(scope, sw.Strs(a), utf8=utf8), sw.PreparedTape(scope, sw.Strs(b), utf8=utf8)
        va, vb, xs, ys = pa[first:first + count], pb[first:first + count], a[first:first + count], b[first:first + count]
        for costs, engine in zip(COSTS, costly):
            same(engine.pairs(va, vb, scope), want_distances(costs, xs, ys, utf8), (costs, size, trial, position, a, b))
        same(unit(va, vb, scope), want_distances(None, *expanded(xs, ys), utf8), ("cross", size, trial, position, a, b))


# ---- f. neighbours that would show --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gaps", NEIGHBOUR_GAPS, ids=["linear", "affine", "wide affine"])
@pytest.mark.parametrize("table", ["unary", "positive"])
@pytest.mark.parametrize("local", [False, True], ids=["nw", "sw"])
def test_score_neighbours_never_show(sw, scope, local, table, gaps):
    """alignshort.hip: "what lies past the string is whatever the tape holds there: the callers never let it decide anything" -- and
    Smith-Waterman lets phantom cells right of the string run. On these tapes whatever lies past (or before) a string continues the
    match, so a neighbour that was read would raise the score: pairs from raw tapes (planned, then believed) and prepared ones, and
    the cross-product of the two tapes."""
    if table == "unary":
        byte_to_class, costs = sw.unary_class_costs(2, -1)
        assert (np.asarray(byte_to_class) == scoring("unary").byte_to_class).all() and (np.asarray(costs) == scoring("unary").costs).all()
    engine = engine_of(sw, scope, table, local, gaps)
    with profiled(scope, ("neighbours", "sw" if local else "nw", table, gaps)) as names:
        for case in neighbour_cases():
            want = want_scores(table, local, gaps, case.a, case.b)
            describe = tuple(case)

            def run(form, ta, tb):
                got = engine.pairs(ta, tb, scope)
                names.note(form)
                same(got, want, (form,) + describe)
            in_forms(sw, scope, "raw", case.a, case.b, False, run)
            in_forms(sw, scope, "prepared", case.a, case.b, False, run, widths=(np.uint64,))
            pq, pc = sw.PreparedTape(scope, sw.Strs(case.a)), sw.PreparedTape(scope, sw.Strs(case.b))
            same(engine(pq, pc, scope), want_scores(table, local, gaps, *expanded(case.a, case.b)), ("cross",) + describe)
            names.note("cross")


@gpu
def test_levenshtein_neighbours_never_show(sw, scope):
    """The analogue for the Levenshtein calls: x against x + t is |t| edits away, and fewer if x's neighbour were read. Unit costs as
    pairs and as a cross-product, general costs as pairs."""
    unit = sw.LevenshteinDistances(capabilities=scope)
    costly = [sw.LevenshteinDistances(*costs, capabilities=scope) for costs in COSTS]
    for case in neighbour_cases():
        at = min(case.position, 1)
        want = want_distances(None, case.a, case.b, False)
        assert want[at] == len(case.t), tuple(case)
        describe = tuple(case)

        def run(form, ta, tb):
            same(unit.pairs(ta, tb, scope), want, (form,) + describe)
            same(unit(ta, tb, scope), want_distances(None, *expanded(case.a, case.b), False), ("cross", form) + describe)
            for costs, engine in zip(COSTS, costly):
                same(engine.pairs(ta, tb, scope), want_distances(costs, case.a, case.b, False), (costs, form) + describe)
        in_forms(sw, scope, "raw", case.a, case.b, False, run)
        in_forms(sw, scope, "prepared", case.a, case.b, False, run, widths=(np.uint64,))


# ---- g. what the sweeps hold: no GPU ------------------------------------------------------------------------------------------------
def test_score_sweeps_hold_what_they_are_meant_to():
    """The generators alone. Every (total_a, total_b) is there twice, the totals lie on both sides of 4 and of 16 on either tape, first
    strings start at 0 and last strings end at the total, the empty-edge trials exist on both sides; the sweeps hold the string lengths
    that the 16-, 32-, 64- and 128-column claims need; the scoring models fold into the class counts they are named for; the lopsided
    and the view sets are complete; and EVERY neighbour case is sensitive: its reference score differs from the reference score with
    1 .. |t| neighbour symbols read on the short side, and with neighbours read on both sides."""
    wanted = set(combinations(SIZES, OTHERS))
    assert wanted == {(t, t) for t in SIZES} | {(t, o) for t in SIZES for o in OTHERS} | {(o, t) for t in SIZES for o in OTHERS}
    sweeps = [(score_pair_sweep(), LETTERS8, True), (score_cross_sweep(LETTERS12), LETTERS12, False), (score_cross_sweep(DNA), DNA, False)]
    for cases, alphabet, both_cut_alike in sweeps:
        assert sorted({(c.total_a, c.total_b) for c in cases}) == sorted(wanted)
        assert all(sum(1 for c in cases if (c.total_a, c.total_b) == pair) == 2 for pair in wanted)
        for case in cases:
            assert (tape_bytes(case.a), tape_bytes(case.b)) == (case.total_a, case.total_b)   # the first string starts at 0, the last ends at the total
            assert 1 <= len(case.a) <= 4 and 1 <= len(case.b) <= (4 if both_cut_alike else 5) and (not both_cut_alike or len(case.a) == len(case.b))
            assert set(b"".join(case.a + case.b)) <= set(alphabet.encode())
            if case.empty_side:
                side = case.a if case.empty_side == "a" else case.b
                assert case.trial == 1 and len(side) >= 3 and len(side[0]) == 0 and len(side[-1]) == 0
        assert {c.empty_side for c in cases} == {None, "a", "b"} and sum(c.empty_side is not None for c in cases) == len(wanted)
        for side in ("total_a", "total_b"):
            other = "total_b" if side == "total_a" else "total_a"
            for low, high in ((0, 3), (4, 15), (16, 80)):
                partners = {getattr(c, other) for c in cases if low <= getattr(c, side) <= high}
                assert any(p < 4 for p in partners) and any(4 <= p < 16 for p in partners) and any(p >= 16 for p in partners)
        # the column variants follow the longest string of both tapes: some case for each of them, and nothing beyond the tapes' 80 bytes
        most = [max(longest(c.a), longest(c.b)) for c in cases]
        assert any(m <= 16 for m in most) and any(16 < m <= 32 for m in most) and any(32 < m <= 64 for m in most) and max(most) <= 80
        if not both_cut_alike:   # k_align_cross_wide: 33 .. 64 is its 64-column variant, 65 .. 80 the 128-column one
            assert any(64 < m <= 80 for m in most)
    assert len(LETTERS8) >= 8 and len(set(LETTERS12)) > 8
    # sweep (d) reaches banded.hip: a string of more than 32 symbols, over bytes and over code points
    for kind in ("bytes", "utf8"):
        assert sum(max(longest(c.a), longest(c.b)) > 32 for c in pair_cases(kind)) >= 50
    assert any(len(x.encode()) > len(x) for c in pair_sweep(True) for x in c.a)
    # the scoring models: how many classes their matrices fold into, every letter a class of its own, costs in [-9, 11] and asymmetric
    for model, low, high in (("classes8", 8, 8), ("classes32", 32, 32), ("wide", 33, 128), ("matrix", 129, 256), ("unary", 32, 32), ("positive", 32, 32)):
        full = scoring(model).full
        assert low <= classes_of(full) <= high, (model, classes_of(full))
        assert full.min() >= -9 and full.max() <= 11 and (model == "unary" or (full != full.T).any())
        for alphabet in (LETTERS8, DNA) + ((LETTERS12,) if model == "classes32" else ()):
            rows = {(full[ord(ch)].tobytes(), full[:, ord(ch)].tobytes()) for ch in alphabet}
            assert len(rows) == len(alphabet), (model, alphabet)
    for model in ("unary", "positive"):
        full = scoring(model).full.astype(np.int64)
        letters = [ord(ch) for ch in LETTERS8]
        assert all(full[p, p] > 0 for p in letters) and all(full[p, q] < 0 for p in letters for q in letters if p != q)
    # the lopsided cases: one tape under 16 bytes in one or two strings, every length as a single string that is its whole tape
    for alphabet in (LETTERS8, DNA):
        cases = lopsided_cases(alphabet)
        assert {(c[0], c[1]) for c in cases} == {(t, n) for t in SHORT_TOTALS for n in LOPSIDED_LENGTHS}
        assert all(tape_bytes(c[2]) == c[0] < 16 and len(c[2]) in (1, 2) and [len(s) for s in c[3]] == [c[1]] for c in cases)
        assert {(c[0], len(c[2])) for c in cases} >= {(t, k) for t in SHORT_TOTALS for k in (1, 2)}
    assert LOPSIDED_LENGTHS == (1, 31, 32, 33, 63, 64, 65, 129, 385, 513, 1100) and PROFILE_LENGTHS == (385, 513, 1100)
    assert [(n, len(x[0]), len(y[0]), len(x), len(y)) for n, x, y in profile_cases()] == [(n, n, n, 1, 1) for n in PROFILE_LENGTHS]
    # the views: every size, trial and position; the view alone is `size` bytes of a tape that is far larger
    for kind in ("bytes", "utf8"):
        views = placed_views(kind)
        assert {(c[0], c[1], c[2]) for c in views} == {(s, t, p) for s in VIEW_SIZES for t in (0, 1) for p in ("start", "middle", "tail")}
        for size, trial, position, a, b, first, count in views:
            assert tape_bytes(a[first:first + count]) == size == tape_bytes(b[first:first + count])
            assert (first == 0) == (position == "start") and (first + count == len(a)) == (position == "tail") and len(a) == len(b)
            assert tape_bytes(a) >= 16 + size and tape_bytes(b) >= 16 + size
    # the neighbour cases: complete ...
    pairs, cases = neighbour_pairs(), neighbour_cases()
    assert {(len(x), len(t)) for x, t in pairs} >= {(nx, nt) for nx in range(1, 8) for nt in range(1, 5)}
    assert {len(x + t) for x, t in pairs} >= set(EDGE_PAIR_LENGTHS)
    for x, t in pairs:
        mine = [c for c in cases if (c.x, c.t) == (x, t)]
        sizes = {True, False} if 2 * len(t) + len(x) < 16 else {False}
        assert {(c.direction, c.mirrored, c.position, c.small) for c in mine} == \
            {(d, m, p, s) for d in ("forwards", "backwards") for m in (False, True) for p in range(3) for s in sizes}
    assert any(c.small for c in cases if len(c.x) == 7 and len(c.t) == 4)
    for c in cases:
        short, long_ = (c.b, c.a) if c.mirrored else (c.a, c.b)
        at = min(c.position, 1)
        assert len(short) == len(long_) == (3 if c.position == 1 else 2)
        assert short[at] == c.x.encode() and long_[at] == (c.x + c.t if c.direction == "forwards" else c.t + c.x).encode()
        assert (tape_bytes(short) < 16 and tape_bytes(long_) < 16) if c.small else (tape_bytes(short) > 16 + len(c.x) and tape_bytes(long_) > 16 + len(c.x))
        joined_short, joined_long = b"".join(short), b"".join(long_)
        start_short, start_long = tape_bytes(short[:at]), tape_bytes(long_[:at])
        if c.position < 2:    # what follows x in its tape is t, ...
            assert joined_short[start_short + len(c.x):].startswith(c.t.encode())
            if c.direction == "forwards":   # ... and from the pair's first byte onwards both tapes hold the same bytes
                assert joined_short[start_short:] == joined_long[start_long:]
        if c.position > 0:    # what precedes x is t, and backwards both tapes hold the same bytes up to the pair's last
            assert joined_short[:start_short].endswith(c.t.encode())
            if c.direction == "backwards":
                assert joined_short[:start_short + len(c.x)] == joined_long[:start_long + len(c.t + c.x)]
    # ... and sensitive, every one of them, under every table, gap model and kind of alignment; and for the Levenshtein calls
    rng = np.random.default_rng(9132)
    junk = "".join(random_tape(rng, 8, LETTERS8, True))
    insensitive, checked = [], 0
    for table in ("unary", "positive"):
        full = scoring(table).full
        for gaps in NEIGHBOUR_GAPS:
            for local in (False, True):
                score = lambda s, l: orc().nw_score(s.encode(), l.encode(), full, gaps[0], gaps[1], local=local)
                for x, t in pairs:
                    for direction in ("forwards", "backwards"):
                        long_ = x + t if direction == "forwards" else t + x
                        for s, l in over_reads(x, t, direction, junk):
                            checked += 1
                            # the short string may be a or b: the costs are asymmetric
                            if score(s, l) == score(x, long_) or score(l, s) == score(long_, x):
                                insensitive.append((table, gaps, local, x, t, direction, s, l))
    assert not insensitive and checked >= 12 * 400, (len(insensitive), checked, insensitive[:5])   # (each in both orders of a and b)
    for x, t in pairs:
        assert orc().levenshtein(x, x + t) == len(t) == orc().levenshtein(t + x, x)
        for costs in COSTS:
            for direction in ("forwards", "backwards"):
                long_ = x + t if direction == "forwards" else t + x
                for s, l in over_reads(x, t, direction, junk)[::2]:
                    assert orc().levenshtein_costs(s, l, *costs) != orc().levenshtein_costs(x, long_, *costs), (costs, x, t, s, l)
