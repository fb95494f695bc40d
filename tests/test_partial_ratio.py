"""Partial ratios (swh_levenshtein_partial_*): rapidfuzz's fuzz.partial_ratio and fuzz.partial_ratio_alignment.

The contract is include/stringwars_amd.h's: the shorter string is the needle p (m symbols), the longer one the haystack t (n symbols);
window o, -(m - 1) <= o <= n - 1, is t[max(0, o) : min(n, o + m)], l symbols, and scores L / (m + l), L = LCS(p, window), compared
exactly; the smallest offset wins among equals; with m == n both directions run, and the second wins only on a strictly larger score.

Two references live here, both on the CPU.
  * `partial_by_windows`: every window, its LCS from test_lcs.py's numpy table (or, on tiny strings, from `lcs_by_definition`), the
    order by `fractions.Fraction`. It is pinned on the header's worked examples.
  * `partial_fast`: Hyyro's bit-vector LCS on Python integers, V = (V + (V & Eq)) | (V - (V & Eq)), the order by cross-multiplied
    integers. The windows that overhang the haystack's front are its prefixes, so ONE pass over t[:m - 1] scores all of them (the
    vector after j columns is that of t[:j]); those that overhang its back are its suffixes, the prefixes of the two strings
    reversed; only the n - m + 1 full windows take a pass each. It is held to the first reference before the GPU is held to it.
Every GPU comparison is exact: the four outputs as integers, the float64 scores bit for bit against 100.0 * (2.0 * L) / (m + (e - s))."""
import ctypes as C
import fractions
import functools
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child
from test_lcs import _lcs_batch, all_strings, lcs_by_definition, mutated, rand_bytes, reference_lcs, symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE, PACKAGE = os.path.join(ROOT, "include"), os.path.join(ROOT, "stringwars_amd")
gpu = pytest.mark.gpu

# a, b, score, L, start, end, side: the worked examples of include/stringwars_amd.h
EXAMPLES = [("kitten", "the sitting cat", 200 * 4 / 12, 4, 4, 10, 0), ("abc", "xxabcxx", 100.0, 3, 2, 5, 0),
            ("lawn", "flaw in law", 200 * 3 / 7, 3, 8, 11, 0), ("yankees", "new york yankees", 100.0, 7, 9, 16, 0),
            ("ab", "ba", 200 * 1 / 3, 1, 0, 1, 0), ("abcx", "xabc", 200 * 3 / 7, 3, 1, 4, 0), ("aab", "baa", 80.0, 2, 1, 3, 0),
            ("abbb", "abab", 200 * 3 / 7, 3, 0, 3, 1), ("aaa", "bbb", 0.0, 0, 0, 3, 0), ("", "", 100.0, 0, 0, 0, 0), ("", "abc", 0.0, 0, 0, 0, 0)]
PARTIAL_SYMBOLS = ("swh_levenshtein_partial_pairs_u64tape", "swh_levenshtein_utf8_partial_pairs_u64tape", "swh_levenshtein_partial_pairs_prepared",
                   "swh_levenshtein_partial_cross_u64tape", "swh_levenshtein_utf8_partial_cross_u64tape", "swh_levenshtein_partial_cross_prepared")
METHODS = ("partial_ratio", "partial_ratio_alignment", "partial_ratio_cross", "partial_counts", "partial_counts_cross")
# partial.hpp: an item holds at most kPartialItemSteps = 4096 column steps of a wave. A needle of 8 symbols is one block, so a pass
# scores 64 windows in 16 steps: 256 passes, 16384 windows per item.
ITEM_WINDOWS_M8 = 16384


# ---- the references -----------------------------------------------------------------------------------------------------------------
def score_of(L, m, n, start, end) -> float:
    """The host expression, operation by operation."""
    total = float(m) + (float(end) - float(start))
    if total > 0:
        return 100.0 * (2.0 * float(L)) / total
    return 100.0 if n == 0 else 0.0


def windows_of(m, n):
    """(o, start, end) of every window, offsets ascending."""
    return [(o, max(0, o), min(n, o + m)) for o in range(-(m - 1), n)] if m else []


@functools.lru_cache(maxsize=None)
def _greater(L, total, than_L, than_total):
    """L / total > than_L / than_total as Fractions (remembered: the tests ask about the same few rationals millions of times)."""
    return fractions.Fraction(L, total) > fractions.Fraction(than_L, than_total)


def _combine(la, lb, best_of):
    """The rules around the window search: which string is the needle, both directions at equal lengths, the results without windows.
    best_of(side) -> (L, start, end) or None when no window shares a symbol with the needle."""
    m = min(la, lb)
    first = 1 if la > lb else 0
    result, key = (0, 0, m, first), (0, 1)
    for side in ((0, 1) if la == lb else (first,)):
        if m == 0:
            break
        found = best_of(side)
        if found is not None and _greater(found[0], m + found[2] - found[1], *key):
            result, key = (found[0], found[1], found[2], side), (found[0], m + found[2] - found[1])
    return result


def partial_by_windows(a, b, utf8=False, lcs=None):
    """(L, start, end, side) by the definition: every window, Fractions for the order. `lcs(p, w)`: another LCS than the numpy table."""
    sa, sb = symbols(a, utf8).tolist(), symbols(b, utf8).tolist()

    def best_of(side):
        p, t = (sa, sb) if side == 0 else (sb, sa)
        wins = windows_of(len(p), len(t))
        if lcs is None:
            Ls = _lcs_many(p, [t[s:e] for _, s, e in wins]) if wins else []
        else:
            Ls = [lcs(p, t[s:e]) for _, s, e in wins]
        best, key = None, (0, 1)
        for (o, s, e), L in zip(wins, Ls):
            if _greater(int(L), len(p) + e - s, *key):   # strict: the smallest offset among equals
                best, key = (int(L), s, e), (int(L), len(p) + e - s)
        return best

    return _combine(len(sa), len(sb), best_of)


def _lcs_many(p, windows):
    rows, columns = [np.array(p, dtype=np.int64)] * len(windows), [np.array(w, dtype=np.int64) for w in windows]
    return _lcs_batch(rows, columns)   # (the windows are no longer than the needle: it is the rows' string)


def _masks(p):
    masks = {}
    for i, c in enumerate(p):
        masks[c] = masks.get(c, 0) | 1 << i
    return masks


def _prefix_lcs(masks, m, t):
    """LCS(p, t[:j]) for j = 1 .. len(t): the zeros of Hyyro's V after every column."""
    full = (1 << m) - 1
    V, out = full, []
    for c in t:
        u = V & masks.get(c, 0)
        V = ((V + u) | (V - u)) & full
        out.append(m - bin(V).count("1"))
    return out


def _best_window(p, t):
    """The best window of t for the needle p by integer cross-multiplication, or None. Candidates in offset order."""
    m, n = len(p), len(t)
    masks, reversed_masks = _masks(p), _masks(p[::-1])
    front = _prefix_lcs(masks, m, t[:m - 1])                   # o = j - m for j = 1 .. m - 1: t[:j]
    back = _prefix_lcs(reversed_masks, m, t[::-1][:m - 1])     # the suffix of j symbols, o = n - j
    best = None
    for o in range(-(m - 1), n):
        s, e = max(0, o), min(n, o + m)
        if o < 0:
            L = front[e - 1]
        elif o + m > n:
            L = back[n - s - 1]
        else:
            L = _prefix_lcs(masks, m, t[s:e])[-1]
        if L and (best is None or L * (m + best[2] - best[1]) > best[0] * (m + e - s)):
            best = (L, s, e)
    return best


@functools.lru_cache(maxsize=None)
def _fast_cached(a, b):
    return _combine(len(a), len(b), lambda side: _best_window(a, b) if side == 0 else _best_window(b, a))


def partial_fast(a, b, utf8=False):
    return _fast_cached(tuple(symbols(a, utf8).tolist()), tuple(symbols(b, utf8).tolist()))


def expected(a, b, utf8=False) -> np.ndarray:
    """(count, 4) int64: L, start, end, side of every pair."""
    return np.array([partial_fast(x, y, utf8) for x, y in zip(a, b)], dtype=np.int64).reshape(len(a), 4)


def expected_scores(a, b, want, utf8=False) -> np.ndarray:
    return np.array([score_of(w[0], min(len(symbols(x, utf8)), len(symbols(y, utf8))), max(len(symbols(x, utf8)), len(symbols(y, utf8))), w[1], w[2])
                     for x, y, w in zip(a, b, want)], dtype=np.float64)


def expanded(queries, candidates):
    return [q for q in queries for _ in candidates], [c for _ in queries for c in candidates]


# ---- calling -------------------------------------------------------------------------------------------------------------------------
def raw_call(sw, engine, scope, a, b, outs, cross=False, stride=0, utf8=False):
    """The C ABI itself on raw u64 tapes; `outs`: four pointers (host or device) or None. Returns (status name, message)."""
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True) if b is not None else (None, None, None)
    fn = getattr(N.lib, "swh_levenshtein_%spartial_%s_u64tape" % ("utf8_" if utf8 else "", "cross" if cross else "pairs"))
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb) if tb is not None else None, *(C.c_void_p(o) for o in outs), stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def assert_counts(got, want, describe=lambda k: int(k)):
    """`got`: the four arrays of a call; `want`: (count, 4)."""
    got = np.stack([np.asarray(g).astype(np.int64).ravel() for g in got], axis=1)
    assert got.shape == want.shape, (got.shape, want.shape)
    wrong = np.nonzero((got != want).any(axis=1))[0]
    assert not len(wrong), [(describe(k), got[k].tolist(), want[k].tolist()) for k in wrong[:5]]


def check_pairs(sw, scope, engine, a, b, utf8=False, describe=None):
    """One pairwise call held to the reference: the four counts, the scores bit for bit, the alignment's five arrays."""
    want = expected(a, b, utf8)
    describe = describe or (lambda k: (int(k), a[k] if len(a[k]) < 40 else len(a[k]), b[k] if len(b[k]) < 40 else len(b[k])))
    sa, sb = sw.Strs(a), sw.Strs(b)
    got = engine.partial_counts(sa, sb, scope)
    assert all(g.dtype == np.uint32 for g in got)
    assert_counts(got, want, describe)
    scores = expected_scores(a, b, want, utf8)
    ratio = engine.partial_ratio(sa, sb, scope)
    assert ratio.dtype == np.float64 and (ratio.view(np.uint64) == scores.view(np.uint64)).all()
    return want, scores


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in PARTIAL_SYMBOLS:
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "partial" in sw.capabilities().split(",")
    for name in METHODS:
        assert callable(getattr(sw.LevenshteinDistances, name)), name
        assert getattr(sw.LevenshteinDistancesUTF8, name) is getattr(sw.LevenshteinDistances, name), name
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_PARTIAL_MAX_NEEDLE 2048u", header) and N.PARTIAL_MAX_NEEDLE == 2048 == sw.PARTIAL_MAX_NEEDLE
    test_library = C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    assert all(hasattr(test_library, name) for name in PARTIAL_SYMBOLS)
    rust = open(os.path.join(ROOT, "stringwars_amd", "rust", "src", "lib.rs")).read()
    cxx = open(os.path.join(ROOT, "include", "stringwars_amd.hpp")).read()
    assert all("fn %s(" % name in rust and name in cxx for name in PARTIAL_SYMBOLS)


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    ta, _, keep_a = sw.engines._c_tape(sw.Strs([b"ab"]), want64=True)
    tb, _, keep_b = sw.engines._c_tape(sw.Strs([b"ba"]), want64=True)
    out32, out64 = np.full(4, 77, np.uint32), np.full(4, 77, np.uint64)
    view = N.PreparedView(None, 0, 1)
    for name in PARTIAL_SYMBOLS:
        sides = (C.byref(view), C.byref(view)) if name.endswith("_prepared") else (C.byref(ta), C.byref(tb))
        out = out64 if "_cross_" in name else out32
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, *sides, *(C.c_void_p(out[k:].ctypes.data) for k in range(4)), 0, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    assert (out32 == 77).all() and (out64 == 77).all()
    with pytest.raises(ValueError):   # the Python front end asks for a scope before anything else
        sw.LevenshteinDistances.partial_ratio(object.__new__(sw.LevenshteinDistances), [b"a"], [b"b"], None)


def test_references_on_the_worked_examples(sw):
    for a, b, score, L, start, end, side in EXAMPLES:
        for reference in (partial_by_windows, partial_fast, lambda x, y: partial_by_windows(x, y, lcs=lcs_by_definition)):
            assert reference(a, b) == (L, start, end, side), (a, b, reference(a, b))
        m, n = min(len(a), len(b)), max(len(a), len(b))
        assert score_of(L, m, n, start, end) == score, (a, b)
    assert abs(score_of(3, 4, 11, 8, 11) - 85.71428571428571) < 1e-12 and abs(score_of(4, 6, 15, 4, 10) - 66.66666666666667) < 1e-12
    # the sides of the rules without windows, and the two directions of the header's equal-length example
    assert partial_fast("abc", "") == (0, 0, 0, 1) and partial_fast("bbb", "aa") == (0, 0, 2, 1)
    assert partial_fast("abab", "abbb") == (3, 0, 3, 0)   # the needle abab reaches 85.71 in abbb: side 0 when it is a
    assert _best_window(tuple(b"abbb"), tuple(b"abab")) == (3, 0, 4) and score_of(3, 4, 4, 0, 4) == 75.0
    # the utf8 switch counts code points
    assert partial_fast("é", "xèx", utf8=True) == (0, 0, 1, 0) and partial_fast("é", "xèx")[0] == 1
    # the engine's host expression is the same one
    lcs, starts, ends = (np.array([e[k] for e in EXAMPLES], dtype=np.uint32) for k in (3, 4, 5))
    m, n = (np.array([f(len(e[0]), len(e[1])) for e in EXAMPLES]) for f in (min, max))
    got = sw.LevenshteinDistances._partial_score(lcs, starts, ends, m, n)
    assert got.dtype == np.float64 and got.tolist() == [e[2] for e in EXAMPLES]


def canonical(strs, alphabet="abc"):
    """The strings whose letters first appear in the alphabet's order: one of every class under renaming the letters."""
    return [s for s in strs if [c for k, c in enumerate(s) if c not in s[:k]] == list(alphabet[:len(set(s))])]


def test_fast_reference_equals_the_window_reference():
    """All pairs over {a, b, c} of a needle of at most 5 symbols and a haystack of at most 7, up to renaming the letters: neither
    reference looks at what a symbol is, only at which symbols are equal, so every needle is scored in the one spelling whose letters
    first appear in the order a, b, c (64 of 364), against all 3280 haystacks; then random pairs, long needles among them. The
    tiny pairs take their LCS lengths by definition."""
    needles, haystacks = canonical(all_strings("abc", 5)), all_strings("abc", 7)
    assert len(needles) == 1 + 1 + 2 + 5 + 14 + 41 and len(haystacks) == 3280
    memo = {}

    def lcs(p, w):
        key = (tuple(p), tuple(w))
        if key not in memo:
            memo[key] = lcs_by_definition(p, w)
        return memo[key]

    equal_lengths = differing = 0
    for p in needles:
        for t in haystacks:
            if len(t) < len(p):
                continue
            want = partial_by_windows(p, t, lcs=lcs)
            assert partial_fast(p, t) == want, (p, t, partial_fast(p, t), want)
            if len(p) == len(t):
                equal_lengths += 1
                differing += partial_by_windows(t, p, lcs=lcs)[:3] != want[:3]
            elif len(p) <= 3:   # the other way round the same window, on side 1
                assert partial_fast(t, p) == want[:3] + (1,), (t, p)
    assert equal_lengths and differing
    rng = np.random.default_rng(70)
    for i in range(300):
        alphabet = (2, 3, 4, 26)[i % 4]
        m = int(rng.integers(0, 12)) if i % 10 else int(rng.integers(30, 80))
        p = rand_bytes(rng, m, alphabet)
        t = rand_bytes(rng, m + int(rng.integers(0, 40)), alphabet)
        if i % 3 == 0 and len(t) > m:   # a mutated copy of the needle inside the haystack
            at = int(rng.integers(0, len(t) - m + 1))
            t = t[:at] + bytes(mutated(rng, p, 1 + m // 8, lambda: int(rng.integers(97, 97 + alphabet)))) + t[at + m:]
        if i % 2:
            p, t = t, p
        assert partial_fast(p, t) == partial_by_windows(p, t), (p, t)


def test_bench_tool_counts_the_window_columns():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_partial_module", os.path.join(ROOT, "tools", "bench_partial.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    la, lb = np.meshgrid(np.arange(0, 9), np.arange(0, 12), indexing="ij")
    want = np.array([[sum(e - s for _, s, e in windows_of(min(x, y), max(x, y))) * (2 if x == y else 1) for y in range(12)] for x in range(9)])
    assert (tool.window_columns(la, lb) == want).all()


# ---- the C++ wrappers: a program of their own -----------------------------------------------------------------------------------------
def build_check_partial(tmp_path):
    """tests/bindings/check_partial.cpp against include/stringwars_amd.hpp and the shipped library."""
    binary = tmp_path / "check_partial"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "tests", "bindings", "check_partial.cpp"),
                    "-o", str(binary), "-L", PACKAGE, "-lstringwars_amd", f"-Wl,-rpath,{PACKAGE}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True, timeout=300)
    return binary


def write_case(path, utf8, a, b):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", int(utf8)))
        for strs in (a, b):
            raw = [x.encode() if isinstance(x, str) else bytes(x) for x in strs]
            offsets = np.cumsum([0] + [len(x) for x in raw]).astype("<u8")
            f.write(struct.pack("<Q", len(raw)) + offsets.tobytes() + b"".join(raw))


def test_cpp_wrappers_build_and_refuse_without_device(tmp_path):
    import torch
    binary = build_check_partial(tmp_path)
    if torch.cuda.is_available():
        return   # (run on the device by test_cpp_wrappers)
    write_case(tmp_path / "case", False, [b"ab"], [b"ba"])
    done = subprocess.run([str(binary), str(tmp_path / "case"), str(tmp_path / "result")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2 and "status" in done.stderr, (done.returncode, done.stderr)


@gpu
def test_cpp_wrappers(tmp_path):
    """LevenshteinDistances::partial and ::partial_cross, the raw and the prepared overloads, bytes and code points."""
    binary = build_check_partial(tmp_path)
    rng = np.random.default_rng(79)
    for utf8 in (False, True):
        a = [e[0] for e in EXAMPLES] + ["".join("abé中"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 12)))) for _ in range(20)]
        b = [e[1] for e in EXAMPLES] + ["".join("abé中"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 40)))) for _ in range(20)]
        if not utf8:
            a, b = [x.encode() for x in a], [x.encode() for x in b]
        write_case(tmp_path / "case", utf8, a, b)
        done = subprocess.run([str(binary), str(tmp_path / "case"), str(tmp_path / "result")], capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stderr
        blob, count, at = open(tmp_path / "result", "rb").read(), len(a), 0
        xa, xb = expanded(a, b)
        oa, ob = expanded(a, a)
        for dtype, n, want in (("<u4", count, expected(a, b, utf8)), ("<u4", count, expected(a, b, utf8)),
                               ("<u8", count * count, expected(xa, xb, utf8)), ("<u8", count * count, expected(oa, ob, utf8))):
            size = np.dtype(dtype).itemsize * n
            assert_counts([np.frombuffer(blob[at + k * size:at + (k + 1) * size], dtype=dtype) for k in range(4)], want)
            at += 4 * size
        assert at == len(blob)


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


def transliterated(s, base):
    """Every letter moved to the code point base + its own: 2-, 3- or 4-byte characters for base 0x100, 0x1000, 0x10000."""
    return "".join(chr(base + ord(c)) for c in s)


@gpu
def test_worked_examples(sw, scope, lev, lev8):
    a, b = [e[0] for e in EXAMPLES], [e[1] for e in EXAMPLES]
    table = np.array([e[3:] for e in EXAMPLES], dtype=np.int64)
    for engine, base in ((lev, 0), (lev8, 0), (lev8, 0x100), (lev8, 0x1000), (lev8, 0x10000)):
        x, y = ([transliterated(s, base) for s in side] for side in (a, b))
        got = engine.partial_counts(sw.Strs(x), sw.Strs(y), scope)
        assert_counts(got, table, lambda k: EXAMPLES[k][:2])
        assert engine.partial_ratio(sw.Strs(x), sw.Strs(y), scope).tolist() == [e[2] for e in EXAMPLES]
        found = engine.partial_ratio_alignment(sw.Strs(x), sw.Strs(y), scope)
        assert isinstance(found, sw.PartialAlignments) and len(found) == len(EXAMPLES)
        for k, (s, t, score, L, start, end, side) in enumerate(EXAMPLES):
            want = (score, 0, len(s), start, end) if side == 0 else (score, start, end, 0, len(t))
            assert found[k] == want, (s, t, found[k], want)
    assert lev.partial_ratio([b"lawn"], [b"flaw in law"], scope)[0] == 200 * 3 / 7    # lists are accepted
    assert lev.partial_ratio_alignment([b"abbb"], [b"abab"], scope)[0] == (200 * 3 / 7, 0, 3, 0, 4)


@gpu
def test_exhaustive_small_strings(sw, scope, lev, lev8):
    """All pairs over {a, b} with 0..6 symbols on both sides, pairwise (16 129 pairs in one call) and as one cross-product; the same
    over a one-byte and a two-byte code point."""
    for alphabet, engine, utf8 in (("ab", lev, False), ("aé", lev8, True)):
        strs = all_strings(alphabet, 6)
        assert len(strs) == 127
        x, y = expanded(strs, strs)
        want, scores = check_pairs(sw, scope, engine, x, y, utf8)
        assert (want[:, 3] == 1).sum() > (127 * 127 - 5461) // 2   # every pair with the longer string first, and some of equal length
        matrices = engine.partial_counts_cross(sw.Strs(strs), sw.Strs(strs), scope)
        assert all(mat.dtype == np.uint64 and mat.shape == (127, 127) for mat in matrices)
        assert_counts(matrices, want, lambda k: (x[k], y[k]))
        ratios = engine.partial_ratio_cross(sw.Strs(strs), None, scope)
        assert ratios.dtype == np.float64 and (ratios.ravel().view(np.uint64) == scores.view(np.uint64)).all()


BLOCK_M = (1, 31, 32, 33, 63, 64, 65, 96, 97, 672, 673, 1024, 1025, 2047, 2048)


@functools.lru_cache(maxsize=None)
def block_edge_cases():
    """(m, n, needle, haystack) for every m against n = m, m + 1 and m + 40 over four letters: the haystack drawn on its own, or with a
    mutated copy of the needle at a random place. Two pairs of either kind per shape, one from 1024 symbols on."""
    rng = np.random.default_rng(71)
    draw = lambda: int(rng.integers(97, 101))
    cases = []
    for m in BLOCK_M:
        for n in (m, m + 1, m + 40):
            for k in range(2 if m >= 1024 else 4):
                needle = rand_bytes(rng, m, 4)
                if k % 2 == 0:
                    haystack = rand_bytes(rng, n, 4)
                else:
                    copy = bytes(mutated(rng, needle, 1 + m // 16, draw))[:n]
                    at = int(rng.integers(0, n - len(copy) + 1))
                    haystack = rand_bytes(rng, at, 4) + copy + rand_bytes(rng, n - at - len(copy), 4)
                assert len(haystack) == n
                cases.append((m, n, needle, haystack))
    return cases


@gpu
def test_block_and_slot_edges(sw, scope, lev):
    """G = 1, 2, 3, 4, 21, 22, 32, 33 and 64 blocks: 64, 32, 21 (a lane idle), 16, 3 (a lane idle), 2 (twenty idle), 2, 1 and 1 windows
    per pass."""
    cases = block_edge_cases()
    assert {(c[0] + 31) // 32 for c in cases} == {1, 2, 3, 4, 21, 22, 32, 33, 64}
    a, b = [c[2] for c in cases], [c[3] for c in cases]
    describe = lambda k: (int(k), cases[k][0], cases[k][1])
    want, _ = check_pairs(sw, scope, lev, a, b, describe=describe)
    assert (want[12:, 0] > 0).all() and len({tuple(w[1:3]) for w in want}) > len(cases) // 2   # (a needle of one symbol may find none)
    swapped, _ = check_pairs(sw, scope, lev, b, a, describe=describe)     # the needle is b: side 1 but where the lengths are equal
    assert all(s[3] == 1 or c[0] == c[1] for s, c in zip(swapped, cases))


@gpu
def test_pass_seams(sw, scope, lev):
    """One block: 64 windows per pass. n + m - 1 = 63, 64, 65, 127, 128 and 129 windows straddle one and two whole passes; a copy of
    the needle sits in the first window, the last window and the windows on either side of every pass seam."""
    rng = np.random.default_rng(72)
    a, b = [], []
    for m in (1, 8, 32):
        for count in (63, 64, 65, 127, 128, 129):
            n = count - m + 1
            for w in sorted({0, m - 1, 62, 63, 64, 126, 127, 128, count - m, count - 1} & set(range(count))):
                needle = rand_bytes(rng, m, 3)
                haystack = bytearray(rand_bytes(rng, n, 3, base=100))   # letters d, e, f: the copy's letters a, b, c stand alone
                o = w - (m - 1)
                for i in range(max(0, o), min(n, o + m)):
                    haystack[i] = needle[i - o]
                a.append(needle); b.append(bytes(haystack))
    want, _ = check_pairs(sw, scope, lev, a, b)
    assert {64, 128} <= {int(w[1]) + len(x) - 1 for w, x in zip(want, a)}   # (the windows right behind a seam are among the results)


@gpu
def test_item_seams(sw, scope, lev):
    """A needle of 8 symbols against 40 000: 40 007 windows, three items of at most ITEM_WINDOWS_M8. Window w has the offset w - 7,
    so the second item begins at offset 16 377 and the third at 32 761."""
    rng = np.random.default_rng(73)
    needle = b"abcdefgh"
    n = 40000
    assert (n + 7 + ITEM_WINDOWS_M8 - 1) // ITEM_WINDOWS_M8 == 3
    seam = ITEM_WINDOWS_M8 - 7

    def haystack(plants):
        text = bytearray(rand_bytes(rng, n, 6, base=99))   # c .. h: every window shares letters with the needle
        for at, what in plants:
            text[at:at + len(what)] = what
        return bytes(text)

    cases = [("first item", [(100, needle)]), ("last item", [(n - 10, needle)]), ("the very last window", [(n - 1, b"a")]),
             ("last window of the first item", [(seam - 1, needle)]), ("first window of the second item", [(seam, needle)]),
             ("across the seam", [(seam - 4, needle)]), ("across the second seam", [(2 * ITEM_WINDOWS_M8 - 7 - 3, needle)]),
             ("two copies, two items", [(5000, needle), (36000, needle)]), ("two copies, first and second item", [(seam - 8, needle), (seam + 1, needle)]),
             ("two near copies in two items", [(9000, b"abcdefgx"), (20000, b"abcdefgx")]), ("nothing planted", [])]
    a, b = [needle] * len(cases), [haystack(plants) for _, plants in cases]
    want, _ = check_pairs(sw, scope, lev, a, b, describe=lambda k: cases[k][0])
    assert want[0].tolist() == [8, 100, 108, 0] and want[1].tolist() == [8, n - 10, n - 2, 0]
    assert want[3, 1] == seam - 1 and want[4, 1] == seam and want[5, 1] == seam - 4
    assert want[7].tolist() == [8, 5000, 5008, 0] and want[8, 1] == seam - 8 and want[9, 0] == 7 and want[9, 1] <= 9000
    check_pairs(sw, scope, lev, b[:3], a[:3])   # side 1
    # the same bytes on every run
    first = lev.partial_counts(sw.Strs(a), sw.Strs(b), scope)
    for _ in range(3):
        assert all((x == y).all() for x, y in zip(first, lev.partial_counts(sw.Strs(a), sw.Strs(b), scope)))


@gpu
def test_equal_lengths(sw, scope, lev):
    rng = np.random.default_rng(74)
    a, b = [b"abbb", b"abab"], [b"abab", b"abbb"]
    for _ in range(1500):
        m = int(rng.integers(1, 13))
        a.append(rand_bytes(rng, m, 2)); b.append(rand_bytes(rng, m, 2))
    want, scores = check_pairs(sw, scope, lev, a, b)
    assert want[0].tolist() == [3, 0, 3, 1] and want[1].tolist() == [3, 0, 3, 0]
    one_way = np.array([_best_window(tuple(x), tuple(y)) or (0, 0, len(x)) for x, y in zip(a, b)])
    other_way = np.array([_best_window(tuple(y), tuple(x)) or (0, 0, len(x)) for x, y in zip(a, b)])
    differing = (one_way != other_way).any(axis=1)
    assert differing.sum() > 150 and 20 < (want[:, 3] == 1).sum() < differing.sum()


def raw_outputs(count, cross_shape=None, fill=77):
    if cross_shape:
        return [np.full(cross_shape, fill, np.uint64) for _ in range(4)]
    return [np.full(count, fill, np.uint32) for _ in range(4)]


@gpu
def test_refusals(sw, scope, lev, lev8):
    rng = np.random.default_rng(75)
    a = [b"abc", rand_bytes(rng, 2048, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 3000, 4)]
    b = [b"acb", rand_bytes(rng, 2048, 4), rand_bytes(rng, 5, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 4000, 4)]
    outs = raw_outputs(5)
    status, message = raw_call(sw, lev, scope, sw.Strs(a), sw.Strs(b), [o.ctypes.data for o in outs])
    assert status == "unsupported_length" and "pair 3" in message and "2049" in message and "SWH_PARTIAL_MAX_NEEDLE" in message, message
    assert all((o == 77).all() for o in outs)
    with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
        lev.partial_ratio(sw.Strs(a), sw.Strs(b), scope)
    assert "pair 3" in str(info.value)
    matrices = raw_outputs(0, (5, 5))
    status, message = raw_call(sw, lev, scope, sw.Strs(a), sw.Strs(b), [o.ctypes.data for o in matrices], cross=True)
    assert status == "unsupported_length" and "pair (2, 3)" in message and all((o == 77).all() for o in matrices), message
    check_pairs(sw, scope, lev, a[:3], b[:3])   # 2048 x 2048 and 2049 x 5 are accepted
    # a general-cost engine
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    for call in (costly.partial_ratio, costly.partial_ratio_alignment, costly.partial_ratio_cross, costly.partial_counts, costly.partial_counts_cross):
        with pytest.raises(sw.StringWarsError, match="not_implemented"):
            call(sw.Strs([b"ab"]), sw.Strs([b"ba"]), scope)
    # count mismatch, all outputs null, stride 2, invalid UTF-8
    pointers = [o.ctypes.data for o in outs]
    assert raw_call(sw, lev, scope, sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), pointers)[0] == "invalid_argument"
    with pytest.raises(ValueError):
        lev.partial_ratio(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope)
    status, message = raw_call(sw, lev, scope, sw.Strs(a[:2]), sw.Strs(b[:2]), [None] * 4)
    assert status == "invalid_argument" and "lcs, starts, ends and sides" in message
    assert raw_call(sw, lev, scope, sw.Strs(a[:2]), sw.Strs(b[:2]), [None] * 4, cross=True)[0] == "invalid_argument"
    assert raw_call(sw, lev, scope, sw.Strs(a[:2]), sw.Strs(b[:2]), pointers, stride=2)[0] == "invalid_argument"
    for bad_a, bad_b in (([b"ok", b"\xff\xfe"], [b"ok", b"x"]), ([b"ok", b"x"], [b"ok", b"\xc3"])):
        assert raw_call(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), pointers, utf8=True)[0] == "invalid_utf8"
        assert raw_call(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), [o.ctypes.data for o in matrices], cross=True, utf8=True)[0] == "invalid_utf8"
    assert all((o == 77).all() for o in outs + matrices)
    # count == 0: success, nothing written
    assert len(lev.partial_ratio(sw.Strs([]), sw.Strs([]), scope)) == 0 and lev.partial_ratio_cross(sw.Strs([]), sw.Strs([b"a"]), scope).shape == (0, 1)
    assert raw_call(sw, lev, scope, sw.Strs([]), sw.Strs([]), pointers)[0] == "success" and all((o == 77).all() for o in outs)
    # each output alone
    x, y = [e[0].encode() for e in EXAMPLES], [e[1].encode() for e in EXAMPLES]
    for k in range(4):
        outs = raw_outputs(len(EXAMPLES))
        status, message = raw_call(sw, lev, scope, sw.Strs(x), sw.Strs(y), [o.ctypes.data if j == k else None for j, o in enumerate(outs)])
        assert status == "success", message
        assert outs[k].tolist() == [e[3 + k] for e in EXAMPLES] and all((o == 77).all() for j, o in enumerate(outs) if j != k)


def cross_batch():
    rng = np.random.default_rng(76)
    draw = lambda: int(rng.integers(97, 101))
    queries = [rand_bytes(rng, rng.integers(0, 25), 4) for _ in range(37)]
    candidates = []
    for k in range(53):
        copy = bytes(mutated(rng, queries[k % 37], int(rng.integers(0, 4)), draw))
        candidates.append(rand_bytes(rng, rng.integers(0, 30), 4) + copy + rand_bytes(rng, rng.integers(0, 30), 4) if k % 3 else copy)
    return queries, candidates


@gpu
def test_cross_and_output_placement(sw, scope, lev):
    import torch
    queries, candidates = cross_batch()
    sq, sc = sw.Strs(queries), sw.Strs(candidates)
    a, b = expanded(queries, candidates)
    want = expected(a, b)
    scores = expected_scores(a, b, want)
    assert_counts(lev.partial_counts_cross(sq, sc, scope), want, lambda k: divmod(int(k), 53))
    ratios = lev.partial_ratio_cross(sq, sc, scope)
    assert ratios.shape == (37, 53) and (ratios.ravel().view(np.uint64) == scores.view(np.uint64)).all()
    # a row stride wider than the row, on the host and on the device: the columns past the rows stay
    wide = np.full((4, 37, 56), 77, np.uint64)
    status, message = raw_call(sw, lev, scope, sq, sc, [wide[k].ctypes.data for k in range(4)], cross=True, stride=56 * 8)
    assert status == "success", message
    assert_counts([wide[k, :, :53] for k in range(4)], want); assert (wide[:, :, 53:] == 77).all()
    wide_d = torch.full((4, 37, 56), 77, dtype=torch.int64, device="cuda")
    status, message = raw_call(sw, lev, scope, sq, sc, [wide_d[k].data_ptr() for k in range(4)], cross=True, stride=56 * 8)
    assert status == "success", message
    assert (wide_d.cpu().numpy() == wide.astype(np.int64)).all()
    # outputs of both kinds in one call, pairwise and cross; a pairwise stride of 12
    host, on_device = raw_outputs(0, (37, 53)), torch.full((4, 37, 53), 77, dtype=torch.int64, device="cuda")
    status, message = raw_call(sw, lev, scope, sq, sc, [host[0].ctypes.data, on_device[1].data_ptr(), host[2].ctypes.data, on_device[3].data_ptr()], cross=True)
    assert status == "success", message
    back = on_device.cpu().numpy()
    assert_counts([host[0], back[1], host[2], back[3]], want); assert (host[1] == 77).all() and (back[0] == 77).all()
    pa, pb = sw.Strs(a[:700]), sw.Strs(b[:700])
    host, on_device = raw_outputs(700), torch.full((4, 700), 77, dtype=torch.int32, device="cuda")
    status, message = raw_call(sw, lev, scope, pa, pb, [on_device[0].data_ptr(), host[1].ctypes.data, on_device[2].data_ptr(), host[3].ctypes.data])
    assert status == "success", message
    back = on_device.cpu().numpy()
    assert_counts([back[0], host[1], back[2], host[3]], want[:700])
    strided = np.full((700, 3), 77, np.uint32)
    status, message = raw_call(sw, lev, scope, pa, pb, [strided.ctypes.data, None, strided.ctypes.data + 8, None], stride=12)
    assert status == "success", message
    assert (strided[:, 0] == want[:700, 0]).all() and (strided[:, 2] == want[:700, 2]).all() and (strided[:, 1] == 77).all()
    # device tapes; prepared tapes of either offset width, whole and as sub-views
    assert_counts(lev.partial_counts_cross(sq.to_device(scope), sc.to_device(scope), scope), want)
    pq, pc = sw.PreparedTape(scope, sq.with_offsets(np.uint32)), sw.PreparedTape(scope, sc.with_offsets(np.uint64))
    assert_counts(lev.partial_counts_cross(pq, pc, scope), want)
    part = want.reshape(37, 53, 4)[5:30, 3:].reshape(-1, 4)
    assert_counts(lev.partial_counts_cross(pq[5:30], pc[3:], scope), part)
    assert_counts(lev.partial_counts(pq[2:37], pc[2:37], scope), want.reshape(37, 53, 4)[np.arange(2, 37), np.arange(2, 37)])
    # b == NULL: the self-product; the diagonal holds L = len, window (0, len), side 0
    own = raw_outputs(0, (37, 37))
    status, message = raw_call(sw, lev, scope, sq, None, [o.ctypes.data for o in own], cross=True)
    assert status == "success", message
    x, y = expanded(queries, queries)
    assert_counts(own, expected(x, y))
    lengths = sq.lengths
    assert (np.diagonal(own[0]) == lengths).all() and (np.diagonal(own[1]) == 0).all() and (np.diagonal(own[2]) == lengths).all()
    assert (np.diagonal(own[3]) == 0).all() and (np.diagonal(lev.partial_ratio_cross(pq, None, scope)) == 100.0).all()
    # profiling describes the whole call
    scope.set_profiling(True)
    try:
        lev.partial_counts(pa, pb, scope)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["cells"] == sum(len(x) * len(y) for x, y in zip(a[:700], b[:700])) and timing["dominant_name"] == "partial"
    assert timing["kernels"] == 4   # the counting and the placing sizes launch, the items, the merge


@gpu
def test_cross_in_many_chunks(request, sw):
    """STRINGWARS_AMD_PARTIAL_CHUNK_PAIRS (test library) shrinks the slices of whole rows to 424 pairs, so the 37 x 53 product runs as
    four slices of eight rows and a ragged fifth of five -- each counted, laid out and cut on its own --, with the same results on
    the host and on the device."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_PARTIAL_CHUNK_PAIRS="424"), test_library=True):
        return
    import torch
    scope = sw.DeviceScope(gpu_device=0)
    lev = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = cross_batch()
    sq, sc = sw.Strs(queries), sw.Strs(candidates)
    a, b = expanded(queries, candidates)
    want = expected(a, b)
    scope.set_profiling(True)
    matrices = lev.partial_counts_cross(sq, sc, scope)
    timing = scope.last_timing()
    scope.set_profiling(False)
    assert_counts(matrices, want)
    # the whole matrix measured once, then per slice two sizes launches, the items and the merge
    assert timing["kernels"] == 1 + 4 * 5 and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    wide_d = torch.full((4, 37, 56), 77, dtype=torch.int64, device="cuda")
    status, message = raw_call(sw, lev, scope, sq, sc, [wide_d[k].data_ptr() for k in range(4)], cross=True, stride=56 * 8)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert_counts([back[k, :, :53] for k in range(4)], want); assert (back[:, :, 53:] == 77).all()
    host, on_device = raw_outputs(0, (37, 53)), torch.full((4, 37, 53), 77, dtype=torch.int64, device="cuda")   # two of each kind
    status, message = raw_call(sw, lev, scope, sq, sc, [host[0].ctypes.data, host[1].ctypes.data, on_device[2].data_ptr(), on_device[3].data_ptr()], cross=True)
    assert status == "success", message
    back = on_device.cpu().numpy()
    assert_counts([host[0], host[1], back[2], back[3]], want)
    # a slice with a long haystack needs more item scratch than the slices before it
    long_q = queries[:9] + [b"abcdefgh", b"ab"]
    long_c = candidates[:5] + [np.random.default_rng(77).integers(97, 105, 40000).astype(np.uint8).tobytes()]
    x, y = expanded(long_q[-2:], long_c[-1:])   # (the reference of the long pairs alone: the others were checked above)
    got = lev.partial_counts_cross(sw.Strs(long_q), sw.Strs(long_c), scope)
    assert_counts([g[-2:, -1] for g in got], expected(x, y))
    x, y = expanded(long_q[:9], long_c[:5])
    assert_counts([g[:9, :5] for g in got], expected(x, y))
    # a refusal still comes before the first row is written
    long_q = [b"ab"] * 300 + [b"a" * 2049]
    untouched = raw_outputs(0, (301, 3))
    status, message = raw_call(sw, lev, scope, sw.Strs(long_q), sw.Strs([b"ab", b"b" * 2049, b"c" * 3000]), [o.ctypes.data for o in untouched], cross=True)
    assert status == "unsupported_length" and "pair (300, 1)" in message and all((o == 77).all() for o in untouched), message


# ---- tape edges ---------------------------------------------------------------------------------------------------------------------
# The reader is chosen by the tape totals of the view: under 4 bytes a tape is read byte by byte, from 16 bytes on BOTH tapes the
# haystack's windows are read with 128-bit loads, in between dword by dword; code-point tapes under four symbols have a path of their own.
EDGE_SIZES = tuple(range(0, 21)) + (63, 64, 65)
EDGE_OTHERS = (3, 4, 5, 15, 16, 17)
EDGE_SYMBOLS = tuple(range(0, 9))
EDGE_SYMBOL_OTHERS = (1, 3, 4, 8)


@functools.lru_cache(maxsize=None)
def edge_sweep(kind):
    from test_tape_edges import FOUR_BYTE, LETTERS, WIDE_LETTERS, make_sweep
    if kind == "bytes":
        return make_sweep(9101, False, EDGE_SIZES, EDGE_OTHERS, LETTERS, True, (1, 4), None)
    if kind == "utf8":
        return make_sweep(9102, True, EDGE_SIZES, EDGE_OTHERS, WIDE_LETTERS, True, (1, 4), None)
    return make_sweep(9103, True, EDGE_SYMBOLS, EDGE_SYMBOL_OTHERS, FOUR_BYTE, False, (1, 4), None)


def test_edge_sweeps_hold_what_they_are_meant_to():
    for kind in ("bytes", "utf8", "symbols"):
        cases = edge_sweep(kind)
        totals = {(c.total_a, c.total_b) for c in cases}
        sizes, others = (EDGE_SYMBOLS, EDGE_SYMBOL_OTHERS) if kind == "symbols" else (EDGE_SIZES, EDGE_OTHERS)
        assert {(s, s) for s in sizes} <= totals and {(s, o) for s in sizes for o in others} <= totals and {(o, s) for s in sizes for o in others} <= totals
        assert any(c.empty_side == "a" for c in cases) and any(c.empty_side == "b" for c in cases)
        assert all(len(c.a) == len(c.b) and c.a[0] is not None for c in cases)
    assert any(len(x) == len(y) > 1 for c in edge_sweep("bytes") for x, y in zip(c.a, c.b))


@gpu
@pytest.mark.parametrize("kind", ["bytes", "utf8", "symbols"])
def test_tape_edges(sw, scope, lev, lev8, kind):
    """One call per case: the first string starts at the tape's first byte and the last ends at its last."""
    engine, utf8 = (lev, False) if kind == "bytes" else (lev8, True)
    for c in edge_sweep(kind):
        want = expected(c.a, c.b, utf8)
        got = engine.partial_counts(sw.Strs(c.a), sw.Strs(c.b), scope)
        assert_counts(got, want, lambda k: (c.total_a, c.total_b, c.trial, c.a[k], c.b[k]))
    if kind == "bytes":   # the byte engine on the multi-byte tapes too
        for c in edge_sweep("utf8")[::3]:
            x, y = [s.encode() for s in c.a], [s.encode() for s in c.b]
            assert_counts(lev.partial_counts(sw.Strs(x), sw.Strs(y), scope), expected(x, y), lambda k: (c.total_a, c.total_b, x[k], y[k]))


@gpu
def test_views_into_larger_tapes(sw, scope, lev, lev8):
    """Views of 1..3 strings into prepared tapes whose neighbours continue the string: a window that read past its view would find
    more of the needle there. The view's own totals (3, 15, 16, 17, 40 bytes or so) choose the reader."""
    rng = np.random.default_rng(78)
    for engine, utf8, alphabet in ((lev, False, "abc"), (lev8, True, "abé中")):
        word = "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), 400))
        cuts = np.sort(rng.integers(0, 401, 70))
        hay = [word[i:j] for i, j in zip(np.r_[0, cuts], np.r_[cuts, 400])]           # neighbours continue each other
        needles = [word[max(0, i - 2):i + int(rng.integers(0, 7))] for i in np.r_[0, cuts]]
        items = lambda strs: list(strs) if utf8 else [s.encode() for s in strs]
        pa = sw.PreparedTape(scope, sw.Strs(items(needles)), utf8=utf8)
        pb = sw.PreparedTape(scope, sw.Strs(items(hay)), utf8=utf8)
        want = expected(items(needles), items(hay), utf8)
        assert_counts(engine.partial_counts(pa, pb, scope), want)
        for first in range(0, 71):
            for count in (1, 2, 3):
                if first + count <= 71:
                    got = engine.partial_counts(pa[first:first + count], pb[first:first + count], scope)
                    assert_counts(got, want[first:first + count], lambda k: (first, count, needles[first + k], hay[first + k]))
                    got = engine.partial_counts(pb[first:first + count], pa[first:first + count], scope)   # the needle on side b
                    flipped = want[first:first + count].copy()
                    unequal = np.array([len(needles[first + k]) != len(hay[first + k]) for k in range(count)])
                    assert_counts([g[unequal] for g in got[:3]] + [got[3][unequal]], np.c_[flipped[unequal, :3], 1 - flipped[unequal, 3]])
