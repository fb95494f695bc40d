"""Tape sizes around the read widths of infix.hip, osa.hip, lcs.hip and jaro.hip: OSA, LCS / Indel, Jaro and infix search on tapes of
0..80 bytes, on lopsided pairs of tapes, on views into larger prepared tapes and next to neighbours that continue a string.

The four kernel files share one way of reading strings, and the variant is chosen by the tape totals of the VIEW (offsets[first + count]):
  * OSA, LCS, Jaro: `wide = !cp && a_total >= 16 && b_total >= 16` -- the columns' string is read with one clamped 128-bit load, which
    `fix16` repairs where the clamp moved the window; otherwise the kWide = false kernel reads dwords through ByteWindow::fetch4_raw;
  * infix: `wide_text = !cp && text_symbols >= 16` looks at the text tape alone, so a pattern tape of 1..3 bytes meets the 128-bit path;
  * a byte tape under 4 bytes is `tiny` and read byte by byte (fetch4_tiny);
  * the code-point kernels read through SymWindow32::fetch4, with a branch of its own for tapes under four symbols (`hi - lo >= 3`).
The sizes below straddle 4 and 16 on either tape independently, with the first and last strings touching the tapes' ends. The stamps
(`osa`, `lcs`, `jaro`, `infix`) do not tell the variants apart: the sizes themselves are the route selection.

Every comparison is exact, against the references of test_osa.py, test_lcs.py, test_jaro.py and test_infix.py; each pair's reference
is computed once (`expected` remembers it) and shared by the tests. The one CPU test runs the generators alone and asserts what the
sweeps are meant to contain.

OSA, LCS and Jaro share their host path (two_tape.hip: scored_run and its front ends); section f holds each of them to its own argument
rules and error texts at the C ABI, from one table."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest

from test_infix import BLOCK_M, brute_force, check_exact, reference_infix
from test_jaro import BLOCK_N, assert_counts, r1, r2, reference, similarities
from test_lcs import lcs_by_definition, reference_indel, reference_lcs
from test_osa import mutated, osa_by_definition, reference_osa

gpu = pytest.mark.gpu

SIZES = tuple(range(0, 41)) + (47, 48, 49, 63, 64, 65, 80)   # bytes of tape: test_small_tapes_and_strings_at_tape_edges' list
OTHERS = (3, 15, 16, 80)                                     # the other tape's total: tiny, narrow, the first wide size, wide
SYMBOL_TOTALS = tuple(range(0, 9))                           # symbols of tape, four-byte characters only (SymWindow32's small tapes)
SYMBOL_OTHERS = (1, 3, 4, 8)
LETTERS = "abc"
WIDE_LETTERS = LETTERS + "éЖ中\U0001f600"
FOUR_BYTE = "\U0001f600\U0001f601\U0001f602"
SHORT_TOTALS = (0, 1, 3, 4, 15)                              # of the lopsided cases' small tape
LONG_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 96, 2047, 2048, 3000)
JARO_LENGTHS = tuple(min(n, 2048) for n in BLOCK_N)
TINY_PATTERNS = (1, 2, 3)
LONG_TEXTS = (16, 17, 300, 5000)
VIEW_SIZES = (3, 15, 16, 17, 40)
CALLS = ("osa", "lcs", "jaro", "infix")
CROSS_CALLS = ("osa", "lcs", "jaro")
TO_CODE_POINTS = str.maketrans("bc", "Ж\U0001f600")   # the lopsided strings as code points: as many symbols as bytes before

Case = namedtuple("Case", "total_a total_b trial empty_side a b")


# ---- the generators -----------------------------------------------------------------------------------------------------------------
def combinations(sizes=SIZES, others=OTHERS):
    """(total_a, total_b): the diagonal, and every size against each of `others` in both orders."""
    out = []
    for total in sizes:
        out.append((total, total))
        for other in others:
            out += [(total, other), (other, total)]
    return list(dict.fromkeys(out))


def random_tape(rng, total, alphabet, in_bytes):
    """Characters of `alphabet` that come to `total` bytes (or symbols)."""
    chars, left = [], total
    while left:
        c = alphabet[int(rng.integers(0, len(alphabet)))]
        size = len(c.encode()) if in_bytes else 1
        if size <= left:
            chars.append(c)
            left -= size
    return chars


def cut(rng, chars, count, empty_edges):
    """`chars` cut at random into `count` strings: the first starts at the tape's first byte, the last ends at its last. With
    `empty_edges` the first and the last string are empty and the ones between them hold the tape."""
    inner = count - 2 if empty_edges else count
    at = np.sort(rng.integers(0, len(chars) + 1, inner - 1)).tolist()
    bounds = [0] + at + [len(chars)]
    pieces = ["".join(chars[bounds[k]:bounds[k + 1]]) for k in range(inner)]
    return [""] + pieces + [""] if empty_edges else pieces


def as_items(strs, utf8):
    return list(strs) if utf8 else [s.encode() for s in strs]


def make_sweep(seed, utf8, sizes, others, alphabet, in_bytes, counts_a, counts_b):
    """Two trials per (total_a, total_b); the second has an empty first and an empty last string on one side (a and b in turn).
    counts_b None: both tapes are cut into the same number of strings (pairs); else each into its own (a cross-product)."""
    rng = np.random.default_rng(seed)
    cases = []
    for at, (total_a, total_b) in enumerate(combinations(sizes, others)):
        for trial in range(2):
            empty_side = (None, "ab"[at % 2])[trial]
            least = 3 if empty_side else counts_a[0]
            count_a = int(rng.integers(least, counts_a[1] + 1))
            count_b = count_a if counts_b is None else int(rng.integers(3 if empty_side else counts_b[0], counts_b[1] + 1))
            a = cut(rng, random_tape(rng, total_a, alphabet, in_bytes), count_a, empty_side == "a")
            b = cut(rng, random_tape(rng, total_b, alphabet, in_bytes), count_b, empty_side == "b")
            cases.append(Case(total_a, total_b, trial, empty_side, as_items(a, utf8), as_items(b, utf8)))
    return cases


@functools.lru_cache(maxsize=None)
def pair_sweep(utf8):
    return make_sweep(9001 + utf8, utf8, SIZES, OTHERS, WIDE_LETTERS if utf8 else LETTERS, True, (1, 4), None)


@functools.lru_cache(maxsize=None)
def symbol_sweep():
    return make_sweep(9003, True, SYMBOL_TOTALS, SYMBOL_OTHERS, FOUR_BYTE, False, (1, 4), None)


@functools.lru_cache(maxsize=None)
def cross_sweep(utf8):
    return make_sweep(9004 + utf8, utf8, SIZES, OTHERS, WIDE_LETTERS if utf8 else LETTERS, True, (1, 4), (1, 5))


@functools.lru_cache(maxsize=None)
def symbol_cross_sweep():
    return make_sweep(9006, True, SYMBOL_TOTALS, SYMBOL_OTHERS, FOUR_BYTE, False, (1, 4), (1, 5))


def tape_bytes(items):
    return sum(len(x.encode()) if isinstance(x, str) else len(x) for x in items)


def split(rng, s, parts):
    """s as one string, or cut at random into two."""
    if parts == 1:
        return [s]
    at = int(rng.integers(0, len(s) + 1))
    return [s[:at], s[at:]]


def letters(rng, n, alphabet=LETTERS):
    return "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), int(n)))


@functools.lru_cache(maxsize=None)
def lopsided_distance_cases():
    """(short total, long length, the small tape's strings, the other tape's): one or two strings that total 0, 1, 3, 4 or 15 bytes
    against strings of `long length` symbols each, mutated repetitions of their partner (every other one without its partner's first letter),
    so that the answer is not simply the length difference."""
    rng = np.random.default_rng(9010)
    cases = []
    for total in SHORT_TOTALS:
        for at, length in enumerate(LONG_LENGTHS):
            small = split(rng, letters(rng, total), 1 + (at + total) % 2)
            large = []
            for s in small:
                base = (s * (length // max(len(s), 1) + 1))[:length] if s else letters(rng, length)
                drawn = LETTERS
                if at % 2 and s:   # the short string's first letter occurs nowhere in the long one: it is no subsequence of it
                    base, drawn = base.replace(s[0], "d"), LETTERS.replace(s[0], "d")
                edited = "".join(mutated(rng, base, int(rng.integers(1, 6)), lambda: drawn[int(rng.integers(0, 3))]))
                large.append((edited + letters(rng, length, drawn))[:length])
            cases.append((total, length, small, large))
    return cases


@functools.lru_cache(maxsize=None)
def lopsided_jaro_cases():
    """(short total, long length, kind, the small tape's strings, the other tape's, known (M, t) with the small string as a, the same
    with it as b -- or None): the constructed ones as test_jaro.block_edge_cases builds them. The fillers y and z match nothing."""
    rng = np.random.default_rng(9011)
    cases = []
    for total in SHORT_TOTALS:
        for at, n in enumerate(JARO_LENGTHS):
            small = split(rng, letters(rng, total), 1 + (at + total) % 2)
            large = []
            for s in small:
                base = (s * (n // max(len(s), 1) + 1))[:n] if s else letters(rng, n)
                large.append(("".join(mutated(rng, base, int(rng.integers(0, 4)), lambda: LETTERS[int(rng.integers(0, 3))])) + letters(rng, n))[:n])
            cases.append((total, n, "random", small, large, None, None))
            if total:
                both = (min(total, n), 0)   # every column finds its match one row further on: the found bit stops every block above
                cases.append((total, n, "one symbol", ["a" * total], ["a" * n], both, both))
                R = max(0, max(total, n) // 2 - 1)
                for where, M in ((R, 1), (R + 1, 0)):
                    if R >= 1 and where < n:
                        # x is the small string's first symbol; in the long one it lies at the window's edge, or one past it
                        far = "z" * where + "x" + "z" * (n - where - 1)
                        cases.append((total, n, "window: x at %d" % where, ["x" + "y" * (total - 1)], [far], (M, 0), (M, 0)))
    return cases


@functools.lru_cache(maxsize=None)
def lopsided_infix_cases():
    """(kind, sizes, patterns, texts): patterns of BLOCK_M symbols against text tapes of 0 .. 15 bytes (the narrow and the tiny text
    reads under up to 64 blocks), and pattern tapes of 1 .. 3 bytes against one text of 16 .. 5000 bytes (the tiny pattern reads next
    to the 128-bit text reads), the occurrence at the front, in the middle and at the very end of the text."""
    rng = np.random.default_rng(9012)
    cases = []
    for total in SHORT_TOTALS:
        for at, m in enumerate(BLOCK_M):
            texts = split(rng, letters(rng, total), 1 + (at + total) % 2)
            patterns = []
            for t in texts:   # the text, a few edits off, somewhere in the pattern
                where = int(rng.integers(0, m + 1))
                edited = "".join(mutated(rng, t, int(rng.integers(0, 2)), lambda: LETTERS[int(rng.integers(0, 3))]))
                patterns.append((letters(rng, where) + edited + letters(rng, m))[:m])
            cases.append(("long pattern", (m, total), patterns, texts))
    for m in TINY_PATTERNS:
        for n in LONG_TEXTS:
            for where in ("front", "middle", "end"):
                p = "cab"[:m]   # c occurs nowhere else in the text
                filler = letters(rng, n - m, "ab")
                at = {"front": 0, "middle": (n - m) // 2, "end": n - m}[where]
                cases.append(("tiny pattern, " + where, (m, n), [p], [filler[:at] + p + filler[at:]]))
    return cases


@functools.lru_cache(maxsize=None)
def view_cases(utf8):
    """(size, trial, position, tape a, tape b, first, count): the sweep's diagonal batches of VIEW_SIZES between junk strings of the
    same letters -- at the start (the view ends below 16 bytes in a large tape), in the middle, and at the tail, where the view's
    last string ends where the buffer ends."""
    rng = np.random.default_rng(9020 + utf8)
    alphabet = WIDE_LETTERS if utf8 else LETTERS
    junk = lambda count: as_items([letters(rng, rng.integers(4, 24), alphabet) for _ in range(count)], utf8)
    cases = []
    for case in pair_sweep(utf8):
        if case.total_a == case.total_b and case.total_a in VIEW_SIZES:
            for position in ("start", "middle", "tail"):
                before = 0 if position == "start" else 5
                after = 0 if position == "tail" else 5
                front_a, front_b, back_a, back_b = junk(before), junk(before), junk(after), junk(after)
                cases.append((case.total_a, case.trial, position, front_a + case.a + back_a, front_b + case.b + back_b, before, len(case.a)))
    return cases


@functools.lru_cache(maxsize=None)
def neighbour_cases():
    """(x, y, tapes): a pair of strings of 1 .. 7 symbols that share a prefix of 0 .. 4, and for small neighbours (tapes under 16
    bytes) and large ones the pair placed first, in the middle and last. The neighbours continue the pair's strings with the same
    letters: what follows x in its tape is what follows the common prefix in y, and the other way round, so a read past a string's
    end that showed would lengthen the prefix or add a match."""
    rng = np.random.default_rng(9030)
    cases = []
    for shared in (0, 1, 2, 3, 4, 4, 3, 1):
        prefix = letters(rng, shared)
        rest_x, rest_y = (letters(rng, rng.integers(0 if shared else 1, 8 - shared)) for _ in range(2))
        if rest_x and rest_y and rest_x[0] == rest_y[0]:   # the common prefix is `shared` symbols, no more
            rest_y = LETTERS[(LETTERS.index(rest_y[0]) + 1) % 3] + rest_y[1:]
        x, y = prefix + rest_x, prefix + rest_y
        tapes = []
        for extra in (1, 12):   # the neighbours' own letters: 2 x (<= 3 + 1) + 7 <= 15 bytes of tape, or far more than 16
            after_x = (y[len(x):] or y)[:3] + letters(rng, extra)
            after_y = (x[len(y):] or x)[:3] + letters(rng, extra)
            other_x, other_y = x[:2] + letters(rng, extra), y[:2] + letters(rng, extra)
            for position in range(3):
                a, b = [other_x, after_x], [other_y, after_y]
                a.insert(position, x); b.insert(position, y)
                tapes.append((position, a, b))
        cases.append((x, y, tapes))
    return cases


# ---- the references, computed once per pair -----------------------------------------------------------------------------------------
_known = {}


def expected(call, a, b, utf8) -> np.ndarray:
    """One row per pair (a[k], b[k]): osa (d), lcs (LCS, indel), jaro (M, t, prefix), infix (d, start, end) of pattern a[k] in b[k]."""
    missing = list(dict.fromkeys((x, y) for x, y in zip(a, b) if (call, utf8, x, y) not in _known))
    if missing:
        xs, ys = [x for x, _ in missing], [y for _, y in missing]
        if call == "osa":
            rows = reference_osa(xs, ys, utf8=utf8)[:, None]
        elif call == "lcs":
            lcs = reference_lcs(xs, ys, utf8=utf8)
            rows = np.stack([lcs, reference_indel(xs, ys, utf8=utf8, lcs=lcs)], axis=1)
        elif call == "jaro":
            rows = reference(xs, ys, utf8=utf8)
        else:
            rows = np.array([reference_infix(x, y, utf8) for x, y in missing], dtype=np.int64).reshape(len(missing), 3)
        for pair, row in zip(missing, rows):
            _known[(call, utf8) + pair] = tuple(int(v) for v in row)
    width = {"osa": 1, "lcs": 2, "jaro": 3, "infix": 3}[call]
    return np.array([_known[(call, utf8, x, y)] for x, y in zip(a, b)], dtype=np.int64).reshape(len(a), width)


def remember(call, cases, utf8, cross=False):
    """The references of a whole sweep in one batch (the numpy references advance many pairs at once)."""
    pairs = [(case.a, case.b) for case in cases]
    if cross:
        pairs = [expanded(a, b) for a, b in pairs] + [expanded(a, a) for a, _ in pairs]
    expected(call, [x for a, _ in pairs for x in a], [y for _, b in pairs for y in b], utf8)


def expanded(queries, candidates):
    return [q for q in queries for _ in candidates], [c for _ in queries for c in candidates]


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
def run_pairs(call, engine, a, b, scope) -> np.ndarray:
    """The call's results in `expected`'s layout."""
    if call == "osa":
        columns = [engine.osa(a, b, scope)]
    elif call == "lcs":
        columns = [engine.lcs(a, b, scope), engine.indel(a, b, scope)]
    elif call == "jaro":
        columns = engine.jaro_counts(a, b, scope)
    else:
        got = engine.infix(a, b, scope)
        columns = [got.distances, got.starts, got.ends]
    return np.stack([np.asarray(c).astype(np.int64) for c in columns], axis=1)


def run_cross(call, engine, queries, candidates, scope) -> np.ndarray:
    if call == "osa":
        columns = [engine.osa_cross(queries, candidates, scope)]
    elif call == "lcs":
        columns = [engine.lcs_cross(queries, candidates, scope), engine.indel_cross(queries, candidates, scope)]
    else:
        columns = engine.jaro_counts_cross(queries, candidates, scope)
    return np.stack([np.asarray(c).astype(np.int64).ravel() for c in columns], axis=1)


def same(call, got, want, describe):
    if call == "jaro":
        assert_counts(list(got.T), want, lambda k: (describe, int(k)))
    else:
        assert got.shape == want.shape, (describe, got.shape, want.shape)
        wrong = np.nonzero((got != want).any(axis=1))[0]
        assert not len(wrong), [(describe, int(k), got[k].tolist(), want[k].tolist()) for k in wrong[:5]]


def forms(sw, scope, sa, sb, utf8):
    """The tapes of a call in the forms besides host raw tapes: device tapes, prepared tapes, prepared tapes of either offset width."""
    yield "device", sa.to_device(scope), sb.to_device(scope)
    yield "prepared", sw.PreparedTape(scope, sa, utf8=utf8), sw.PreparedTape(scope, sb, utf8=utf8)
    for width in (np.uint32, np.uint64):
        yield width.__name__, sw.PreparedTape(scope, sa.with_offsets(width), utf8=utf8), sw.PreparedTape(scope, sb.with_offsets(width), utf8=utf8)


def check_similarities(sw, engine, scope, a, b, utf8):
    """jaro and jaro_winkler of one batch: the header's expressions on the reference's counts, with ==."""
    jaro, winkler = similarities(a, b, expected("jaro", a, b, utf8), utf8=utf8)
    assert (engine.jaro(sw.Strs(a), sw.Strs(b), scope) == jaro).all()
    assert (engine.jaro_winkler(sw.Strs(a), sw.Strs(b), scope) == winkler).all()


@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


# ---- a. the size sweep, pairwise ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
@pytest.mark.parametrize("call", CALLS)
def test_size_sweep_pairs(sw, scope, lev, lev8, call, utf8):
    """Tapes of SIZES bytes against tapes of the same size, of 3, 15, 16 and 80 bytes, in both orders: `wide` is an AND of the two
    totals (for infix the text tape's alone -- b here), `tiny` is per tape. Host raw tapes everywhere; on the diagonal device tapes,
    prepared tapes and prepared tapes of 32- and 64-bit offsets too. The code-point engine also runs tapes of 0 .. 8 four-byte
    symbols: SymWindow32::fetch4's `hi - lo >= 3`."""
    engine = lev8 if utf8 else lev
    cases = pair_sweep(utf8) + (symbol_sweep() if utf8 else [])
    remember(call, cases, utf8)
    for case in cases:
        want = expected(call, case.a, case.b, utf8)
        describe = (case.total_a, case.total_b, case.trial, case.a, case.b)
        sa, sb = sw.Strs(case.a), sw.Strs(case.b)
        same(call, run_pairs(call, engine, sa, sb, scope), want, ("raw",) + describe)
        if case.total_a == case.total_b:
            for form, ta, tb in forms(sw, scope, sa, sb, utf8):
                same(call, run_pairs(call, engine, ta, tb, scope), want, (form,) + describe)
    if call == "jaro":
        some = [c for c in cases if c.total_a in (3, 15, 16) and c.total_a == c.total_b]
        for case in some:
            check_similarities(sw, engine, scope, case.a, case.b, utf8)
        check_similarities(sw, engine, scope, [x for c in cases for x in c.a], [y for c in cases for y in c.b], utf8)
    if call == "infix":   # the same through test_infix's own comparison, InfixMatches' indexing included
        for case in cases[::40]:
            check_exact(engine.infix(sw.Strs(case.a), sw.Strs(case.b), scope), case.a, case.b, utf8=utf8)


# ---- b. the size sweep, cross-products ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
@pytest.mark.parametrize("call", CROSS_CALLS)
def test_size_sweep_cross(sw, scope, lev, lev8, call, utf8):
    """The same sizes with 1 .. 4 queries against 1 .. 5 candidates, and the self-product of the queries (candidates None: both
    sides are the same tape), against the references on the expanded pairs."""
    engine = lev8 if utf8 else lev
    cases = cross_sweep(utf8) + (symbol_cross_sweep() if utf8 else [])
    remember(call, cases, utf8, cross=True)
    for case in cases:
        describe = (case.total_a, case.total_b, case.trial, case.a, case.b)
        sq, sc = sw.Strs(case.a), sw.Strs(case.b)
        same(call, run_cross(call, engine, sq, sc, scope), expected(call, *expanded(case.a, case.b), utf8), ("cross",) + describe)
        same(call, run_cross(call, engine, sq, None, scope), expected(call, *expanded(case.a, case.a), utf8), ("self",) + describe)
    if call == "jaro":
        case = next(c for c in cross_sweep(utf8) if c.total_a == 15 and c.total_b == 16)
        x, y = expanded(case.a, case.b)
        jaro, winkler = similarities(x, y, expected("jaro", x, y, utf8), utf8=utf8)
        assert (engine.jaro_cross(sw.Strs(case.a), sw.Strs(case.b), scope).ravel() == jaro).all()
        assert (engine.jaro_winkler_cross(sw.Strs(case.a), sw.Strs(case.b), scope).ravel() == winkler).all()


# ---- c. lopsided tapes --------------------------------------------------------------------------------------------------------------
def lopsided_pairs(case):
    return [s.encode() for s in case[2]], [s.encode() for s in case[3]]


def lopsided_items(strs, utf8):
    return [s.translate(TO_CODE_POINTS) for s in strs] if utf8 else [s.encode() for s in strs]


@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
@pytest.mark.parametrize("call", ["osa", "lcs"])
def test_lopsided_distances(sw, scope, lev, lev8, call, utf8):
    """One tape of 0 .. 15 bytes, the other holds strings of up to 3000 symbols: the kWide = false kernel (fetch4_raw, and
    fetch4_tiny under 4 bytes) runs thousands of columns, in either order of the tapes."""
    engine = lev8 if utf8 else lev
    for total, length, small, large in lopsided_distance_cases():
        small, large = lopsided_items(small, utf8), lopsided_items(large, utf8)
        for a, b in ((small, large), (large, small)):
            want = expected(call, a, b, utf8)
            same(call, run_pairs(call, engine, sw.Strs(a), sw.Strs(b), scope), want, (total, length, len(a[0]), len(b[0])))


@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_lopsided_jaro(sw, scope, lev, lev8, utf8):
    """b long and a tiny -- up to 64 blocks and min(m, n + R) columns on the narrow reads -- and a long with b tiny: one block, the
    window term decides. The constructed cases give a known (M, t), which the reference is held to first."""
    engine = lev8 if utf8 else lev
    assert {c[1] for c in lopsided_jaro_cases()} == set(JARO_LENGTHS)
    for total, n, kind, small, large, known_small_a, known_small_b in lopsided_jaro_cases():
        small, large = lopsided_items(small, utf8), lopsided_items(large, utf8)
        for a, b, known in ((small, large, known_small_a), (large, small, known_small_b)):
            want = expected("jaro", a, b, utf8)
            if known is not None:
                assert tuple(want[0, :2]) == known, (total, n, kind)
            same("jaro", run_pairs("jaro", engine, sw.Strs(a), sw.Strs(b), scope), want, (total, n, kind, len(a[0]), len(b[0])))
    total, n, kind, small, large, _, _ = next(c for c in lopsided_jaro_cases() if c[0] == 15 and c[1] == 2048)
    check_similarities(sw, engine, scope, lopsided_items(small, utf8), lopsided_items(large, utf8), utf8)


@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_lopsided_infix(sw, scope, lev, lev8, utf8):
    """Patterns of up to 2048 symbols -- 64 blocks -- against text tapes of 0 .. 15 bytes: the narrow and the tiny text reads; and
    pattern tapes of 1 .. 3 bytes (`tiny`) against one text of 16 .. 5000 bytes, which `wide_text` alone puts on the 128-bit text
    reads, with the occurrence at the front, in the middle and at the very end of the text."""
    engine = lev8 if utf8 else lev
    placed = set()
    for kind, sizes, patterns, texts in lopsided_infix_cases():
        patterns, texts = lopsided_items(patterns, utf8), lopsided_items(texts, utf8)
        got = engine.infix(sw.Strs(patterns), sw.Strs(texts), scope)
        check_exact(got, patterns, texts, utf8=utf8)
        if kind.startswith("tiny pattern"):   # the planted occurrence is the only exact one
            at = {"front": 0, "middle": (sizes[1] - sizes[0]) // 2, "end": sizes[1] - sizes[0]}[kind.split(", ")[1]]
            assert got[0] == (0, at, at + sizes[0]), (kind, sizes, got[0])
            placed.add((at == 0, at + sizes[0] == sizes[1]))
    assert placed == {(True, False), (False, False), (False, True)}


# ---- d. views into a larger prepared tape -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
@pytest.mark.parametrize("call", CALLS)
def test_views_into_a_larger_tape(sw, scope, lev, lev8, call, utf8):
    """The tape total a kernel sees is offsets[first + count] of the VIEW: a view at the start of a large prepared tape lands on the
    narrow (or tiny) side, one in the middle reads between junk strings, one at the tail ends where the buffer ends. The results
    are those of the small batch alone."""
    engine = lev8 if utf8 else lev
    assert {c[0] for c in view_cases(utf8)} == set(VIEW_SIZES) and {c[2] for c in view_cases(utf8)} == {"start", "middle", "tail"}
    for size, trial, position, a, b, first, count in view_cases(utf8):
        pa, pb = sw.PreparedTape(scope, sw.Strs(a), utf8=utf8), sw.PreparedTape(scope, sw.Strs(b), utf8=utf8)
        want = expected(call, a[first:first + count], b[first:first + count], utf8)
        got = run_pairs(call, engine, pa[first:first + count], pb[first:first + count], scope)
        same(call, got, want, (size, trial, position, a, b))
        if call in CROSS_CALLS and trial == 0:
            want = expected(call, *expanded(a[first:first + count], b[first:first + count]), utf8)
            same(call, run_cross(call, engine, pa[first:first + count], pb[first:first + count], scope), want, ("cross", size, position, a, b))


# ---- e. neighbour independence ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
@pytest.mark.parametrize("call", CALLS)
def test_neighbours_never_show(sw, scope, lev, lev8, call, utf8):
    """jaro.hip: "bytes past a string's end are whatever follows it: prefix_max cuts them off" -- and so must every other read past
    a string's end be cut off. One pair first, in the middle and last in its tapes, among neighbours that continue its strings,
    on tapes under and over 16 bytes: the same results in every place, and the reference's."""
    engine = lev8 if utf8 else lev
    sizes = set()
    for x, y, tapes in neighbour_cases():
        want = expected(call, lopsided_items([x], utf8), lopsided_items([y], utf8), utf8)
        for position, a, b in tapes:
            a, b = lopsided_items(a, utf8), lopsided_items(b, utf8)
            sizes.add(sum(map(len, a)) < 16)
            got = run_pairs(call, engine, sw.Strs(a), sw.Strs(b), scope)
            same(call, got[position:position + 1], want, ("the pair", x, y, position, a, b))
            same(call, got, expected(call, a, b, utf8), ("its neighbours", x, y, position, a, b))
            if call == "infix":
                check_exact(engine.infix(sw.Strs(a), sw.Strs(b), scope), a, b, utf8=utf8)
            if call == "jaro" and position == 1:
                check_similarities(sw, engine, scope, a, b, utf8)
    assert sizes == {True, False}


# ---- f. the argument rules of the three scored families, family by family ----------------------------------------------------------
UNIT_COSTS = " (match 0, mismatch 1, open 1, extend 1)"
# What differs between the families at the C ABI. `outputs`: in ABI order, as columns of `expected`; `bound`: the pairwise calls take one;
# `null_on_empty`: what a call with every output null says on empty tapes (None: success); `stride_2` / `stride_6`: a pairwise
# out_stride_bytes of 2 / 6 (None: accepted); `row_plus_4`: a row_stride_bytes of nb * 8 + 4; `oversize_cross`: the first refused pair
# of OVERSIZE_A x OVERSIZE_B in row order, with its lengths.
FAMILY_RULES = {
    "osa": dict(outputs=(0,), bound=True,
                unit_costs="OSA distances need unit costs" + UNIT_COSTS,
                null="null output pointer", null_on_empty=None,
                stride_2="out_stride_bytes must be >= 4", stride_6=None, row_plus_4=None,
                tail="the shorter string exceeds SWH_OSA_MAX_SHORTER (2048)", oversize_cross=(1, 1, 2049, 2049)),
    "lcs": dict(outputs=(1, 0), bound=True,
                unit_costs="LCS lengths and Indel distances are called on a unit-cost engine" + UNIT_COSTS,
                null="null output pointers: one of indel and lcs is needed",
                null_on_empty="null output pointers: one of indel and lcs is needed",
                stride_2="out_stride_bytes must be >= 4", stride_6=None, row_plus_4=None,
                tail="the shorter string exceeds SWH_LCS_MAX_SHORTER (2048)", oversize_cross=(1, 1, 2049, 2049)),
    "jaro": dict(outputs=(0, 1, 2), bound=False,
                 unit_costs="Jaro and Jaro-Winkler counts are called on a unit-cost engine" + UNIT_COSTS,
                 null="null output pointers: one of matches, transpositions and prefix is needed",
                 null_on_empty="null output pointers: one of matches, transpositions and prefix is needed",
                 stride_2="out_stride_bytes must be 0 or a multiple of 4", stride_6="out_stride_bytes must be 0 or a multiple of 4",
                 row_plus_4="row_stride_bytes must be 0 or a multiple of 8",
                 tail="a string exceeds SWH_JARO_MAX_LENGTH (2048)", oversize_cross=(0, 1, 2, 2049)),
}
RULE_A, RULE_B = [b"ab", b"ca"], [b"ba", b"ac"]
OVERSIZE_A, OVERSIZE_B = [b"ab", b"a" * 2049], [b"ba", b"b" * 2049]
SENTINEL = 0x4D


def raw_scored(sw, call, kind, engine_handle, scope, a, b, outs, stride):
    """One of the 18 scored exports as it stands: `a` / `b` are both Strs or both PreparedTape (b None: a null pointer), `outs` the
    family's output pointers (None: null). Returns (status name, message)."""
    from stringwars_amd import _native as N
    if isinstance(a, sw.PreparedTape):
        sides, form = [None if x is None else x.view() for x in (a, b)], "prepared"
    else:
        kept = [None if x is None else sw.engines._c_tape(x, want64=True) for x in (a, b)]
        sides, form = [None if k is None else k[0] for k in kept], "u64tape"
    extra = (C.c_uint32(N.UNBOUNDED),) if kind == "pairs" and FAMILY_RULES[call]["bound"] else ()
    err = C.c_char_p()
    status = getattr(N.lib, "swh_levenshtein_%s_%s_%s" % (call, kind, form))(
        engine_handle, scope.handle, *(None if x is None else C.byref(x) for x in sides), *extra, *(C.c_void_p(p) for p in outs), stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode() if status else ""


@gpu
@pytest.mark.parametrize("call", CROSS_CALLS)
def test_each_family_keeps_its_own_argument_rules(sw, scope, lev, call):
    """OSA, LCS and Jaro go through one set of host checks, and each keeps the rules and the words it had: the status and the whole
    message of every refusal, on raw and on prepared tapes, with not a byte of the outputs written; and the results of the strides
    that one family accepts and another refuses, at those strides. Two pairs of two-byte strings; one pair of 2049 symbols for the
    length limit."""
    rules = FAMILY_RULES[call]
    outputs = len(rules["outputs"])
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    global_scores = sw.NeedlemanWunschScores(substitution_matrix=sw.substitution_matrix(42), open=-4, extend=-4, capabilities=scope)
    want = {"pairs": expected(call, RULE_A, RULE_B, False)[:, rules["outputs"]],
            "cross": expected(call, *expanded(RULE_A, RULE_B), False)[:, rules["outputs"]],
            "self": expected(call, *expanded(RULE_A, RULE_A), False)[:, rules["outputs"]]}
    room = 64   # bytes per output: two results at a stride of 12, two rows at a stride of 20

    def fresh():
        return [np.full(room, SENTINEL, np.uint8) for _ in range(outputs)]

    def pointers(buffers):
        return [x.ctypes.data for x in buffers]

    def refused(status, message, kind, engine, a, b, outs, stride, buffers=()):
        got = raw_scored(sw, call, kind, engine._handle, scope, a, b, outs, stride)
        assert got == (status, message), (call, kind, type(a).__name__, stride, got)
        assert all((x == SENTINEL).all() for x in buffers), (call, kind, message)

    def accepted(kind, a, b, stride, want_rows, nb=1):
        """The call's results lie at `stride` (of results for pairs, of rows of `nb` for cross) and nothing else is written."""
        buffers = fresh()
        got = raw_scored(sw, call, kind, lev._handle, scope, a, b, pointers(buffers), stride)
        assert got == ("success", ""), (call, kind, stride, got)
        width = 4 if kind == "pairs" else 8
        for column, buffer in enumerate(buffers):
            written = np.zeros(room, bool)
            for k, value in enumerate(want_rows[:, column]):
                at = (k // nb) * stride + (k % nb) * width if kind == "cross" else k * stride
                assert int.from_bytes(buffer[at:at + width].tobytes(), "little") == value, (call, kind, stride, column, k)
                written[at:at + width] = True
            assert (buffer[~written] == SENTINEL).all(), (call, kind, stride, column)

    sa, sb = sw.Strs(RULE_A), sw.Strs(RULE_B)
    pa, pb = sw.PreparedTape(scope, sa), sw.PreparedTape(scope, sb)
    for a, b in ((sa, sb), (pa, pb)):
        for kind in ("pairs", "cross"):
            buffers = fresh()
            outs = pointers(buffers)
            # the engine: general costs, and a handle of another kind
            refused("not_implemented", rules["unit_costs"], kind, costly, a, b, outs, 0, buffers)
            refused("invalid_argument", "not a Levenshtein engine", kind, global_scores, a, b, outs, 0, buffers)
            # every output null: on two pairs, and on no pairs at all
            refused("invalid_argument", rules["null"], kind, lev, a, b, [None] * outputs, 0)
            none = (sw.Strs([]), sw.Strs([])) if a is sa else (pa[0:0], pb[0:0])
            if rules["null_on_empty"] is None:
                assert raw_scored(sw, call, kind, lev._handle, scope, *none, [None] * outputs, 0) == ("success", "")
            else:
                refused("invalid_argument", rules["null_on_empty"], kind, lev, *none, [None] * outputs, 0)
        # pairwise: the counts, and strides of 2, 6 and 12 bytes
        buffers = fresh()
        outs = pointers(buffers)
        refused("invalid_argument", "a and b must hold the same number of strings", "pairs", lev, a, sw.Strs(RULE_B[:1]) if a is sa else pb[0:1],
                outs, 0, buffers)
        refused("invalid_argument", rules["stride_2"], "pairs", lev, a, b, outs, 2, buffers)
        if rules["stride_6"] is None:
            accepted("pairs", a, b, 6, want["pairs"])
        else:
            refused("invalid_argument", rules["stride_6"], "pairs", lev, a, b, outs, 6, buffers)
        accepted("pairs", a, b, 12, want["pairs"])
        # cross: rows of nb * 8 - 8 and of nb * 8 + 4 bytes
        nb = len(RULE_B)
        refused("invalid_argument", "row_stride_bytes too small", "cross", lev, a, b, outs, nb * 8 - 8, buffers)
        if rules["row_plus_4"] is None:
            accepted("cross", a, b, nb * 8 + 4, want["cross"], nb)
        else:
            refused("invalid_argument", rules["row_plus_4"], "cross", lev, a, b, outs, nb * 8 + 4, buffers)
        accepted("cross", a, b, nb * 8 + 8, want["cross"], nb)
    # the length limit: the pair, its lengths and the family's own words, before anything is written
    la, lb = sw.Strs(OVERSIZE_A), sw.Strs(OVERSIZE_B)
    i, j, m, n = rules["oversize_cross"]
    for a, b in ((la, lb), (sw.PreparedTape(scope, la), sw.PreparedTape(scope, lb))):
        buffers = fresh()
        refused("unsupported_length", "pair 1: 2049 x 2049 symbols, " + rules["tail"], "pairs", lev, a, b, pointers(buffers), 0, buffers)
        refused("unsupported_length", "pair (%d, %d): %d x %d symbols, %s" % (i, j, m, n, rules["tail"]), "cross", lev, a, b, pointers(buffers), 0,
                buffers)
    # prepared views: a null b is the self-product of a cross call, and an error of a pairwise one
    accepted("cross", pa, None, 16, want["self"], len(RULE_A))
    accepted("cross", pa, pa, 16, want["self"], len(RULE_A))
    assert (want["self"] != want["cross"]).any()
    buffers = fresh()
    refused("invalid_argument", "null prepared view", "pairs", lev, pa, None, pointers(buffers), 0, buffers)
    refused("invalid_argument", "null tape", "pairs", lev, sa, None, pointers(buffers), 0, buffers)


# ---- f2. the argument rules of top-k, within, align and infix, call by call ---------------------------------------------------------
TWO_TAPE_CALLS = ("topk", "within", "align", "infix")
UNBOUNDED = 0xFFFFFFFF
# What differs between the four calls at the C ABI. `bad`: an argument of the call's own that it refuses, and the words it has for it
# (a view beyond its tape wins over it, it wins over a UTF-8 tape next to a byte tape); `null_b`: what a null second side is;
# `tape_first`: a null tape is tested before a null engine.
CALL_RULES = {
    "topk": dict(bad=dict(k=0), bad_says="k must lie in [1, SWH_TOPK_MAX]", null_b="self", tape_first=True, costs=None),
    "within": dict(bad=dict(bound=UNBOUNDED), bad_says="a range search needs a bound: without one it is the dense cross-product", null_b="self",
                   tape_first=True, costs=None),
    "align": dict(bad=dict(null=(1,)), bad_says="null output pointer", null_b="null", tape_first=True,
                  costs="alignments need unit costs" + UNIT_COSTS, counts="a and b must hold the same number of strings"),
    "infix": dict(bad=dict(null=(0,)), bad_says="null output pointer", null_b="null", tape_first=False,
                  costs="infix search needs unit costs" + UNIT_COSTS, counts="patterns and texts must hold the same number of strings"),
}
ROOM = 64   # bytes per output


def raw_two_tape(sw, call, engine, scope, a, b, tail, form=None):
    """One of the twelve exports as it stands. `a` / `b`: a Strs, a PreparedTape, a PreparedView passed as it is, or None (a null
    pointer; `form` then says which export); `engine` None: a null handle; `tail`: the C arguments between the tapes and the error.
    Returns (status name, message)."""
    from stringwars_amd import _native as N
    sides, kept = [], []
    for x in (a, b):
        if isinstance(x, sw.PreparedTape):
            x = x.view()
        elif isinstance(x, sw.Strs):
            kept.append(sw.engines._c_tape(x, want64=True))
            x = kept[-1][0]
        sides.append(x)
    if form is None:
        form = "prepared" if isinstance(sides[0], N.PreparedView) else "u64tape"
    err = C.c_char_p()
    status = getattr(N.lib, "swh_levenshtein_%s_%s" % (call, form))(
        None if engine is None else engine._handle, scope.handle, *(None if x is None else C.byref(x) for x in sides), *tail, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode() if status else ""


def two_tape_tail(call, buffers, k=2, bound=None, capacity=ROOM // 4, null=()):
    """The call's own arguments in ABI order. `buffers`: its outputs in ABI order (top-k: indices, distances; within: row_offsets,
    indices, distances; align: distances, ops_offsets, ops; infix: distances, starts, ends); `null`: which of them are passed as null."""
    outs = [None if i in null else x.ctypes.data for i, x in enumerate(buffers)]
    if call == "topk":
        return (k, UNBOUNDED if bound is None else bound, *outs)
    if call == "within":
        return (1 if bound is None else bound, *outs, capacity)
    if call == "align":
        return (UNBOUNDED if bound is None else bound, *outs, capacity)
    return (UNBOUNDED if bound is None else bound, *outs)


def fresh_outputs(call):
    return [np.full(ROOM, SENTINEL, np.uint8) for _ in range(2 if call == "topk" else 3)]


def words(buffer, dtype, count):
    return buffer[:count * np.dtype(dtype).itemsize].view(dtype)


def topk_of(d, k):
    """(indices, distances) of the k smallest of every row of a dense matrix, ties by candidate index."""
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.uint32), np.take_along_axis(d, order, axis=1).astype(np.uint32)


def csr_of(d, bound):
    hits = d <= bound
    offsets = np.concatenate([[0], np.cumsum(hits.sum(axis=1))]).astype(np.uint64)
    return offsets, np.nonzero(hits)[1].astype(np.uint32), d[hits].astype(np.uint32)


@gpu
@pytest.mark.parametrize("call", TWO_TAPE_CALLS)
def test_each_two_tape_call_keeps_its_own_argument_rules(sw, scope, lev, call):
    """Top-k, within, align and infix resolve their tapes through one front end, and each keeps the rules, the order and the words it
    had: the status and the whole message of every refusal, which refusal wins where two apply, on raw and on prepared tapes, with
    not a byte of the outputs written; what an empty call writes; and the searches' self-search and general-cost results. Two strings
    of two bytes a side."""
    from stringwars_amd import _native as N
    rules = CALL_RULES[call]
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    global_scores = sw.NeedlemanWunschScores(substitution_matrix=sw.substitution_matrix(42), open=-4, extend=-4, capabilities=scope)
    sa, sb = sw.Strs(RULE_A), sw.Strs(RULE_B)
    pa, pb = sw.PreparedTape(scope, sa), sw.PreparedTape(scope, sb)
    pb8 = sw.PreparedTape(scope, sb, utf8=True)

    def refused(status, message, engine, a, b, form=None, **tail):
        buffers = fresh_outputs(call)
        got = raw_two_tape(sw, call, engine, scope, a, b, two_tape_tail(call, buffers, **tail), form)
        assert got == (status, message), (call, type(a).__name__, tail, got)
        assert all((x == SENTINEL).all() for x in buffers), (call, message)

    def accepted(engine, a, b, form=None, **tail):
        buffers = fresh_outputs(call)
        got = raw_two_tape(sw, call, engine, scope, a, b, two_tape_tail(call, buffers, **tail), form)
        assert got == ("success", ""), (call, type(a).__name__, tail, got)
        return buffers

    def untouched(buffer, written=0):
        assert (buffer[written:] == SENTINEL).all(), call

    for a, b, one, none, form in ((sa, sb, sw.Strs(RULE_B[:1]), sw.Strs([]), "u64tape"), (pa, pb, pb[0:1], pa[0:0], "prepared")):
        null_says = "null prepared view" if form == "prepared" else "null tape"
        # ---- what all four share -------------------------------------------------------------------------------------------------------
        refused("invalid_argument", "not a Levenshtein engine", global_scores, a, b)
        refused("invalid_argument", "null scope or engine", None, a, b)
        refused("invalid_argument", null_says if rules["tape_first"] else "null scope or engine", None, None, b, form)
        refused("invalid_argument", null_says, lev, None, b, form)
        refused("invalid_argument", rules["bad_says"], lev, a, b, **rules["bad"])
        if form == "prepared":
            beyond = N.PreparedView(pa._handle, 1, 2)
            for x, y in ((beyond, b.view()), (a.view(), beyond)):
                refused("invalid_argument", "view exceeds the prepared tape", lev, x, y)
                refused("invalid_argument", "view exceeds the prepared tape", lev, x, y, **rules["bad"])
            refused("invalid_argument", "one tape was prepared as UTF-8, the other as bytes", lev, pa, pb8)
            refused("invalid_argument", rules["bad_says"], lev, pa, pb8, **rules["bad"])
        # ---- a null second side, general costs, the counts ----------------------------------------------------------------------------
        no_tape = N.PreparedView(None, 0, 0)
        if rules["null_b"] == "null":
            refused("invalid_argument", null_says, lev, a, None)
            if form == "prepared":
                refused("invalid_argument", null_says, lev, a, no_tape)
                refused("invalid_argument", null_says, lev, no_tape, b)
            refused("not_implemented", rules["costs"], costly, a, b)
            refused("invalid_argument", rules["counts"], lev, a, one)
        else:
            twice = accepted(lev, a, a)
            for nothing in (None,) + ((no_tape,) if form == "prepared" else ()):
                assert all((x == y).all() for x, y in zip(accepted(lev, a, nothing), twice)), (call, form)
            assert any((x != y).any() for x, y in zip(accepted(lev, a, b), twice)), call

        # ---- each call's own ----------------------------------------------------------------------------------------------------------
        if call == "topk":
            refused("invalid_argument", rules["bad_says"], lev, a, b, k=N.TOPK_MAX + 1)
            refused("invalid_argument", "null output pointer", lev, a, b, null=(0,))
            refused("invalid_argument", "null output pointer", lev, a, b, null=(1,))
            for buffer in accepted(lev, none, b, null=(0, 1)) + accepted(lev, none, b):
                untouched(buffer)
            for engine in (lev, costly):
                indices, distances = accepted(engine, a, b)
                want = topk_of(np.asarray(engine(sa, sb, scope)), 2)
                assert (words(indices, np.uint32, 4) == want[0].ravel()).all() and (words(distances, np.uint32, 4) == want[1].ravel()).all(), (call, form)
                untouched(indices, 16), untouched(distances, 16)
        elif call == "within":
            refused("invalid_argument", "null row_offsets", lev, a, b, null=(0,))
            refused("invalid_argument", "indices and distances must both be given, or neither", lev, a, b, null=(1,))
            refused("invalid_argument", "indices and distances must both be given, or neither", lev, a, b, null=(2,))
            refused("invalid_argument", "a capacity without arrays: the counting call passes NULL, NULL, 0", lev, a, b, null=(1, 2), capacity=1)
            offsets, indices, distances = accepted(lev, none, b)
            assert (words(offsets, np.uint64, 1) == 0).all()
            untouched(offsets, 8), untouched(indices), untouched(distances)
            offsets, indices, distances = accepted(lev, a, none)
            assert (words(offsets, np.uint64, 3) == 0).all()
            untouched(offsets, 24), untouched(indices), untouched(distances)
            for engine, bound in ((lev, 1), (costly, 2)):
                offsets, indices, distances = accepted(engine, a, b, bound=bound)
                want = csr_of(np.asarray(engine(sa, sb, scope)), bound)
                total = int(want[0][-1])
                assert total and (words(offsets, np.uint64, 3) == want[0]).all(), (call, form)
                assert (words(indices, np.uint32, total) == want[1]).all() and (words(distances, np.uint32, total) == want[2]).all(), (call, form)
                untouched(offsets, 24), untouched(indices, 4 * total), untouched(distances, 4 * total)
            offsets, indices, distances = accepted(lev, a, b, null=(1, 2), capacity=0)   # the counting call
            assert (words(offsets, np.uint64, 3) == csr_of(np.asarray(lev(sa, sb, scope)), 1)[0]).all()
        elif call == "align":
            refused("invalid_argument", "null output pointer", lev, a, b, null=(0,))
            refused("invalid_argument", "null output pointer", lev, a, b, null=(2,))
            refused("invalid_argument", "null output pointer", lev, none, none, null=(1,))
            for null in ((), (0, 2)):
                distances, offsets, ops = accepted(lev, none, none, null=null)
                assert (words(offsets, np.uint64, 1) == 0).all()
                untouched(distances), untouched(offsets, 8), untouched(ops)
        else:
            for null in ((0,), (1,), (2,)):
                refused("invalid_argument", "null output pointer", lev, a, b, null=null)
            for buffer in accepted(lev, none, none, null=(0, 1, 2)) + accepted(lev, none, none):
                untouched(buffer)


@gpu
def test_two_tape_calls_refuse_mixed_and_mismatched_tapes_in_python(sw, scope, lev, lev8):
    """The wrapper's own refusals of topk, within, align and infix, before any C call: a prepared tape next to a raw one is a TypeError,
    byte-prepared tapes on a UTF-8 engine a ValueError. A UTF-8 tape as the second side only: align and infix say so themselves, the
    two searches leave it to the library."""
    sa, sb = sw.Strs(RULE_A), sw.Strs(RULE_B)
    pa, pb, pb8 = sw.PreparedTape(scope, sa), sw.PreparedTape(scope, sb), sw.PreparedTape(scope, sb, utf8=True)
    calls = {"topk": lambda e, a, b: e.topk(a, b, scope, k=1), "within": lambda e, a, b: e.within(a, b, scope, bound=1),
             "align": lambda e, a, b: e.align(a, b, scope), "infix": lambda e, a, b: e.infix(a, b, scope)}
    needs = "a %s engine needs tapes prepared with utf8=%s"
    for name, call in calls.items():
        for a, b in ((pa, sb), (sa, pb)):
            with pytest.raises(TypeError, match="^both tapes of a call must be prepared, or neither$"):
                call(lev, a, b)
        with pytest.raises(ValueError, match="^" + needs % ("LevenshteinDistancesUTF8", True) + "$"):
            call(lev8, pa, pb)
        if name in ("align", "infix"):
            with pytest.raises(ValueError, match="^" + needs % ("LevenshteinDistances", False) + "$"):
                call(lev, pa, pb8)
        else:
            with pytest.raises(sw.StringWarsError, match="^invalid_argument: one tape was prepared as UTF-8, the other as bytes$"):
                call(lev, pa, pb8)


@gpu
def test_topk_and_within_score_the_general_path_alike(sw, scope, lev8):
    """One sweep scores the blocks of both searches: on the same views, bound and scope, the general path (code points: never the fused
    kernel's) names the same scoring kernel after `topk_select/` and `within_select/`, and top-k and the counting call of within count
    the same cells. 300 x 200 words."""
    rng = np.random.default_rng(11)
    items = ["".join(rng.choice(list("abé中"), int(rng.integers(1, 12)))) for _ in range(500)]
    pq, pc = sw.PreparedTape(scope, sw.Strs(items[:300]), utf8=True), sw.PreparedTape(scope, sw.Strs(items[300:]), utf8=True)
    scope.set_profiling(True)
    try:
        lev8.topk(pq, pc, scope, k=3, bound=4)
        top = scope.last_timing()
        lev8.within(pq, pc, scope, bound=4, out=(np.zeros(301, np.uint64), None, None))
        counted = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert top["dominant_name"].startswith("topk_select/") and counted["dominant_name"].startswith("within_select/"), (top, counted)
    assert top["dominant_name"].split("/", 1)[1] == counted["dominant_name"].split("/", 1)[1] != "", (top, counted)
    assert top["cells"] == counted["cells"] > 0, (top, counted)


# ---- g. what the sweeps hold, and what the references are worth: no GPU -------------------------------------------------------------
def test_sweeps_hold_what_they_are_meant_to():
    """The generators alone. Every (total_a, total_b) is there twice, the totals lie on both sides of 4 and of 16 on either tape,
    the forced empty-edge trials exist on both sides, every lopsided length is present; and on a sample of the sweep the imported
    references agree with the definition-level ones (osa_by_definition, lcs_by_definition, r1 against r2, brute_force)."""
    wanted = {(t, t) for t in SIZES} | {(t, o) for t in SIZES for o in OTHERS} | {(o, t) for t in SIZES for o in OTHERS}
    assert SIZES == tuple(range(41)) + (47, 48, 49, 63, 64, 65, 80) and len(wanted) == len(combinations())
    for utf8 in (False, True):
        for cases, both_cut_alike in ((pair_sweep(utf8), True), (cross_sweep(utf8), False)):
            assert sorted({(c.total_a, c.total_b) for c in cases}) == sorted(wanted)
            for case in cases:
                assert (tape_bytes(case.a), tape_bytes(case.b)) == (case.total_a, case.total_b)
                assert 1 <= len(case.a) <= 4 and 1 <= len(case.b) <= (4 if both_cut_alike else 5)
                assert not both_cut_alike or len(case.a) == len(case.b)
                if case.empty_side:
                    side = case.a if case.empty_side == "a" else case.b
                    assert case.trial == 1 and len(side) >= 3 and len(side[0]) == 0 and len(side[-1]) == 0
            assert all(sum(1 for c in cases if (c.total_a, c.total_b) == pair) == 2 for pair in wanted)
            assert {c.empty_side for c in cases} == {None, "a", "b"} and sum(c.empty_side is not None for c in cases) == len(wanted)
            for side in ("total_a", "total_b"):   # either tape: tiny, narrow and wide, next to a partner that is narrow and one that is wide
                other = "total_b" if side == "total_a" else "total_a"
                for low, high in ((0, 3), (4, 15), (16, 80)):
                    partners = {getattr(c, other) for c in cases if low <= getattr(c, side) <= high}
                    assert any(p < 4 for p in partners) and any(4 <= p < 16 for p in partners) and any(p >= 16 for p in partners)
            if not both_cut_alike:
                assert {len(c.a) for c in cases} == {1, 2, 3, 4} and {len(c.b) for c in cases} == {1, 2, 3, 4, 5}
    assert any(len(x.encode()) > len(x) for c in pair_sweep(True) for x in c.a)
    for cases in (symbol_sweep(), symbol_cross_sweep()):
        assert {(len("".join(c.a)), len("".join(c.b))) for c in cases} == set(combinations(SYMBOL_TOTALS, SYMBOL_OTHERS))
        assert all(len(ch.encode()) == 4 for c in cases for s in c.a + c.b for ch in s)
        assert {len("".join(c.a)) for c in cases} >= {0, 1, 2, 3, 4, 5} and {len("".join(c.b)) for c in cases} >= {0, 1, 2, 3, 4, 5}
    # the lopsided cases: one tape under 16 bytes, every length on the other
    distance = lopsided_distance_cases()
    assert {(c[0], c[1]) for c in distance} == {(t, n) for t in SHORT_TOTALS for n in LONG_LENGTHS}
    assert all(sum(map(len, c[2])) == c[0] < 16 and len(c[2]) in (1, 2) and [len(s) for s in c[3]] == [c[1]] * len(c[2]) for c in distance)
    assert {len(c[2]) for c in distance if c[0] == 15} == {1, 2}
    for at, c in enumerate(distance):   # without its first letter in the long string, a short string costs more than the length difference
        for (d,), (lcs, _), x, y in zip(expected("osa", *lopsided_pairs(c), False), expected("lcs", *lopsided_pairs(c), False), c[2], c[3]):
            if (at % len(LONG_LENGTHS)) % 2 and x and len(y) >= len(x):
                assert x[0] not in y and d > len(y) - len(x) and lcs < len(x), (x, y)
    jaro = lopsided_jaro_cases()
    assert JARO_LENGTHS == (1, 31, 32, 33, 63, 64, 65, 96, 97, 2047, 2048)
    assert {(c[0], c[1]) for c in jaro} == {(t, n) for t in SHORT_TOTALS for n in JARO_LENGTHS}
    assert all(sum(map(len, c[3])) == c[0] < 16 and all(len(s) == c[1] for s in c[4]) for c in jaro)
    assert sum(c[5] is not None for c in jaro) >= 2 * len(JARO_LENGTHS) and {c[5][0] for c in jaro if c[2].startswith("window")} == {0, 1}
    for c in jaro:
        if c[5] is not None:   # the constructed cases give what they were built to give, with either string driving
            assert r1(list(c[3][0].encode()), list(c[4][0].encode()))[:2] == c[5], c[:3]
            assert r1(list(c[4][0].encode()), list(c[3][0].encode()))[:2] == c[6], c[:3]
    infix = lopsided_infix_cases()
    assert {c[1] for c in infix if c[0] == "long pattern"} == {(m, t) for m in BLOCK_M for t in SHORT_TOTALS}
    assert all(sum(map(len, c[3])) == c[1][1] and all(len(p) == c[1][0] for p in c[2]) for c in infix if c[0] == "long pattern")
    assert {(c[0], c[1]) for c in infix if c[0] != "long pattern"} == \
        {("tiny pattern, " + w, (m, n)) for w in ("front", "middle", "end") for m in TINY_PATTERNS for n in LONG_TEXTS}
    assert all(len(c[2]) == 1 and len(c[2][0]) == c[1][0] and len(c[3][0]) == c[1][1] for c in infix if c[0] != "long pattern")
    for utf8 in (False, True):
        views = view_cases(utf8)
        assert {(c[0], c[1], c[2]) for c in views} == {(s, t, p) for s in VIEW_SIZES for t in (0, 1) for p in ("start", "middle", "tail")}
        for size, trial, position, a, b, first, count in views:
            assert tape_bytes(a[first:first + count]) == size == tape_bytes(b[first:first + count])
            assert (first == 0) == (position == "start") and (first + count == len(a)) == (position == "tail") and len(a) == len(b)
            assert tape_bytes(a) >= 16 + size and tape_bytes(b) >= 16 + size
    pairs = neighbour_cases()
    assert {len(x) for x, _, _ in pairs} | {len(y) for _, y, _ in pairs} <= set(range(1, 8))
    assert {r1(list(x.encode()), list(y.encode()))[2] for x, y, _ in pairs} == {0, 1, 2, 3, 4}
    for x, y, tapes in pairs:
        assert {(position, sum(map(len, a)) < 16, sum(map(len, b)) < 16) for position, a, b in tapes} == \
            {(p, small, small) for p in range(3) for small in (True, False)}
        assert all(a[position] == x and b[position] == y for position, a, b in tapes)
    # the imported references against the definitions, on a sample of the sweep
    sample = [c for c in pair_sweep(False) if c.total_a <= 12 and c.total_b <= 12][::2] + [c for c in pair_sweep(True) if c.total_a <= 12 and c.total_b <= 12][::3]
    checked = 0
    for case in sample:
        utf8 = isinstance(case.a[0], str)
        as_symbols = (lambda s: [ord(ch) for ch in s]) if utf8 else list
        for x, y in zip(case.a, case.b):
            sx, sy = as_symbols(x), as_symbols(y)
            assert expected("osa", [x], [y], utf8)[0, 0] == osa_by_definition(tuple(sx), tuple(sy)), (x, y)
            assert tuple(expected("lcs", [x], [y], utf8)[0]) == (lcs_by_definition(sx, sy), len(sx) + len(sy) - 2 * lcs_by_definition(sx, sy)), (x, y)
            assert tuple(expected("jaro", [x], [y], utf8)[0]) == r1(sx, sy) == r2(sx, sy), (x, y)
            if len(sx) <= 6 and len(sy) <= 9:
                assert tuple(expected("infix", [x], [y], utf8)[0]) == brute_force(sx, sy), (x, y)
            checked += 1
    assert checked >= 100
