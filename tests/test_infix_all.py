"""Infix search for every occurrence within a bound (swh_levenshtein_infix_all_*): the ends of a text at which its pattern occurs
within `bound` edits, as CSR rows, under the three selects (all, best, minima).

The reference is numpy and test_infix's: D, the bottom row of the semi-global Wagner-Fischer matrix, is `last_row(p, t, anchored=False)`;
the selects are applied to it as the header defines them; the start of a hit that ends at e is e - the first column whose value is
D(e) in `last_row` of the reversed pattern against the reversed t[:e]. Where a row has many hits those last rows are computed for all
its ends in one sweep (`last_rows`: the same recurrence with one text per matrix row), which a CPU test holds to `last_row` itself.
A brute force over every substring pins all of it on the tiny cases."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from test_infix import golden_lines, last_row, mutated, py_levenshtein, rand_bytes, reference_infix, symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PACKAGE = os.path.join(ROOT, "stringwars_amd")
SELECTS = ("all", "best", "minima")
SELECT_ID = {"all": 0, "best": 1, "minima": 2}
SENTINEL = 0xA5A5A5A5
WIDE = "aж中\U0001F600"   # 1-, 2-, 3- and 4-byte code points


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def last_rows(p: np.ndarray, texts: np.ndarray) -> np.ndarray:
    """`last_row(p, texts[k], anchored=True)` for every row k of `texts` at once (symbols < 0 match nothing: padding)."""
    count, n = texts.shape
    ar = np.arange(n + 1, dtype=np.int32)
    row = np.tile(ar, (count, 1))
    tmp = np.empty((count, n + 1), dtype=np.int32)
    for i in range(1, len(p) + 1):
        tmp[:, 0] = i
        np.minimum(row[:, :-1] + (texts != p[i - 1]), row[:, 1:] + 1, out=tmp[:, 1:])
        row = np.minimum.accumulate(tmp - ar, axis=1) + ar
    return row


def select_ends(D: np.ndarray, bound, select: str) -> list:
    """The ends e = 0 .. n that are hits, as the header defines them."""
    n = len(D) - 1
    within = (lambda e: True) if bound is None else (lambda e: int(D[e]) <= bound)
    if select == "all":
        return [e for e in range(n + 1) if within(e)]
    if select == "best":
        return [e for e in range(n + 1) if D[e] == D.min() and within(e)]
    ends = []
    for e in range(n + 1):
        if not within(e) or (e > 0 and D[e - 1] <= D[e]):
            continue
        later = [int(D[f]) for f in range(e + 1, n + 1) if D[f] != D[e]]
        if not later or later[0] > D[e]:
            ends.append(e)
    return ends


_ROWS = {}   # (pattern, text, utf8) -> [symbols of p, symbols of t, D, {end: start}]: computed once, shared by every test


def reference_hits(p, t, bound, select, utf8=False) -> list:
    """[(start, end, d)] of one pair, ascending by end."""
    key = (p, t, utf8)
    if key not in _ROWS:
        ps, ts = symbols(p, utf8), symbols(t, utf8)
        _ROWS[key] = [ps, ts, last_row(ps, ts, anchored=False), {}]
    ps, ts, D, starts = _ROWS[key]
    ends = select_ends(D, bound, select)
    missing = [e for e in ends if e not in starts]
    if len(missing) == 1:
        e = missing[0]
        back = last_row(ps[::-1], ts[:e][::-1], anchored=True)
        starts[e] = e - int(np.nonzero(back == D[e])[0][0])
    elif missing:
        reversed_prefixes = np.full((len(missing), max(missing)), -1, dtype=np.int64)
        for k, e in enumerate(missing):
            reversed_prefixes[k, :e] = ts[:e][::-1]
        back = last_rows(ps[::-1], reversed_prefixes)
        for k, e in enumerate(missing):
            starts[e] = e - int(np.nonzero(back[k, :e + 1] == D[e])[0][0])
    return [(starts[e], e, int(D[e])) for e in ends]


def expected_csr(patterns, texts, bound, select, utf8=False):
    """(offsets u64, starts, ends, distances u32) of a batch."""
    rows = [reference_hits(p, t, bound, select, utf8) for p, t in zip(patterns, texts)]
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    flat = np.array([h for r in rows for h in r], dtype=np.int64).reshape(-1, 3)
    return (offsets,) + tuple(flat[:, k].astype(np.uint32) for k in range(3))


def brute_hits(p, t, bound, select) -> list:
    """The definition, over every substring: D(e) and the largest start that reaches it, then the select rules with +inf at both ends."""
    n, inf = len(t), float("inf")
    table = [[py_levenshtein(p, t[s:e]) for s in range(e + 1)] for e in range(n + 1)]
    D = [min(row) for row in table]
    start = [max(s for s in range(e + 1) if table[e][s] == D[e]) for e in range(n + 1)]
    hits = []
    for e in range(n + 1):
        if D[e] > bound:
            continue
        if select == "best" and D[e] != min(D):
            continue
        if select == "minima":
            before = D[e - 1] if e > 0 else inf
            after = next((D[f] for f in range(e + 1, n + 1) if D[f] != D[e]), inf)
            if not (before > D[e] and after > D[e]):
                continue
        hits.append((start[e], e, D[e]))
    return hits


EXAMPLES = [
    ("abc", "xxabcxx", 1, "all", [(2, 4, 1), (2, 5, 0), (2, 6, 1)]), ("abc", "xxabcxx", 1, "best", [(2, 5, 0)]), ("abc", "xxabcxx", 1, "minima", [(2, 5, 0)]),
    ("lawn", "flaw in law", 1, "all", [(1, 4, 1), (1, 5, 1), (8, 11, 1)]), ("lawn", "flaw in law", 1, "minima", [(1, 4, 1), (8, 11, 1)]),
    ("ab", "abab", 0, "all", [(0, 2, 0), (2, 4, 0)]), ("ab", "abab", 0, "best", [(0, 2, 0), (2, 4, 0)]), ("ab", "abab", 0, "minima", [(0, 2, 0), (2, 4, 0)]),
    ("ab", "ba", 1, "all", [(0, 1, 1), (1, 2, 1)]),
    ("aaa", "bbb", 2, "all", []), ("aaa", "bbb", 2, "best", []), ("aaa", "bbb", 2, "minima", []),
    ("aaa", "bbb", 3, "all", [(0, 0, 3), (1, 1, 3), (2, 2, 3), (3, 3, 3)]), ("aaa", "bbb", 3, "minima", [(0, 0, 3)]),
    ("", "abc", 0, "all", [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0)]), ("", "abc", 0, "minima", [(0, 0, 0)]),
    ("abc", "", 3, "all", [(0, 0, 3)]), ("abc", "", 3, "best", [(0, 0, 3)]), ("abc", "", 3, "minima", [(0, 0, 3)]),
    ("abc", "", 2, "all", []), ("abc", "", 2, "best", []), ("abc", "", 2, "minima", []),
]


def all_strings(alphabet, upto):
    return ["".join(x) for n in range(upto + 1) for x in itertools.product(alphabet, repeat=n)]


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_reference_equals_brute_force():
    pairs = [(p, t) for p in all_strings("ab", 3) for t in all_strings("ab", 5)]
    assert len(pairs) == 945
    wrong = [(p, t, bound, select) for p, t in pairs for bound in range(4) for select in SELECTS
             if reference_hits(p, t, bound, select) != brute_hits(p, t, bound, select)]
    assert not wrong, wrong[:5]


def test_reference_examples():
    for p, t, bound, select, want in EXAMPLES:
        assert reference_hits(p, t, bound, select) == want == brute_hits(p, t, bound, select), (p, t, bound, select)


def test_batched_last_rows_equal_last_row():
    rng = np.random.default_rng(3)
    for _ in range(40):
        p = symbols(rand_bytes(rng, rng.integers(0, 40), 3, 97))
        texts = [symbols(rand_bytes(rng, rng.integers(0, 50), 3, 97)) for _ in range(5)]
        padded = np.full((5, max(map(len, texts))), -1, dtype=np.int64)
        for k, t in enumerate(texts):
            padded[k, :len(t)] = t
        rows = last_rows(p, padded)
        for k, t in enumerate(texts):
            assert (rows[k, :len(t) + 1] == last_row(p, t, anchored=True)).all()


def test_best_row_begins_with_the_infix_occurrence():
    rng = np.random.default_rng(7)
    hits = 0
    for i in range(300):
        p = rand_bytes(rng, rng.integers(0, 30), 3, 97)
        t = rand_bytes(rng, rng.integers(0, 80), 3, 97)
        d, s, e = reference_infix(p, t)
        for bound in (None, d, d - 1):
            row = reference_hits(p, t, bound, "best")
            if bound is not None and d > bound:
                assert row == []
            else:
                assert row[0] == (s, e, d) and all(h[2] == d for h in row), (i, bound)
                hits += len(row)
    assert hits > 600


def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in ("swh_levenshtein_infix_all_u64tape", "swh_levenshtein_utf8_infix_all_u64tape", "swh_levenshtein_infix_all_prepared"):
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert callable(sw.LevenshteinDistances.infix_all) and sw.LevenshteinDistancesUTF8.infix_all is sw.LevenshteinDistances.infix_all
    header = open(os.path.join(INCLUDE, "stringwars_amd.h")).read()
    for name, value in (("ALL", 0), ("BEST", 1), ("MINIMA", 2)):
        assert "#define SWH_INFIX_SELECT_%s %du" % (name, value) in header and getattr(N, "INFIX_SELECT_" + name) == value
    got = sw.InfixOccurrences(np.array([0, 2, 2, 3], np.uint64), np.array([1, 1, 8], np.uint32), np.array([4, 5, 11], np.uint32), np.array([1, 1, 1], np.uint32))
    assert len(got) == 3 and got[0] == [(1, 1, 4), (1, 1, 5)] and got[1] == [] and got[-1] == [(1, 8, 11)] and got.counts.tolist() == [2, 0, 1]
    assert [x.tolist() for x in got.row(2)] == [[8], [11], [1]]
    bare = sw.InfixOccurrences(np.array([0, 1], np.uint64), None, np.array([4], np.uint32), np.array([1], np.uint32))
    assert bare.starts is None and bare[0] == [(1, None, 4)] and bare.row(0)[0] is None
    counted = sw.InfixOccurrences(np.array([0, 5], np.uint64), None, None, None)
    assert counted.counts.tolist() == [5]
    with pytest.raises(ValueError):
        counted.row(0)
    with pytest.raises(IndexError):
        got[3]
    with pytest.raises(ValueError):
        sw.InfixOccurrences(np.array([0, 1], np.uint64), None, np.array([4], np.uint32), None)


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    tp, _, keep_p = sw.engines._c_tape(sw.Strs([b"abc"]), want64=True)
    tt, _, keep_t = sw.engines._c_tape(sw.Strs([b"xxabcxx"]), want64=True)
    offsets = np.full(2, 77, np.uint64)
    outs = [np.full(4, 77, np.uint32) for _ in range(3)]
    tail = [1, 0, C.c_void_p(offsets.ctypes.data), *(C.c_void_p(o.ctypes.data) for o in outs), 4]
    for name in ("swh_levenshtein_infix_all_u64tape", "swh_levenshtein_utf8_infix_all_u64tape"):
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, C.byref(tp), C.byref(tt), *tail, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    view = N.PreparedView(None, 0, 1)
    err = C.c_char_p()
    status = N.lib.swh_levenshtein_infix_all_prepared(None, None, C.byref(view), C.byref(view), *tail, C.byref(err))
    assert N.STATUS_NAMES[status] == "no_device" and err.value
    assert (offsets == 77).all() and all((o == 77).all() for o in outs)
    with pytest.raises(sw.StringWarsError, match="no_device"):
        sw.DeviceScope(gpu_device=0)


# ---- the C++ wrappers: a program of their own -------------------------------------------------------------------------------------------
def build_check_infix_all(tmp_path):
    """tests/bindings/check_infix_all.cpp against include/stringwars_amd.hpp and the shipped library."""
    binary = tmp_path / "check_infix_all"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "tests", "bindings", "check_infix_all.cpp"),
                    "-o", str(binary), "-L", PACKAGE, "-lstringwars_amd", f"-Wl,-rpath,{PACKAGE}", "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True, text=True, timeout=300)
    return binary


def write_program_case(path, utf8, patterns, texts, requests):
    """The case file of check_infix_all.cpp; `requests`: (prepared, with starts, bound, select id)."""
    with open(path, "wb") as out:
        out.write(struct.pack("<i", int(utf8)))
        for side in (patterns, texts):
            items = [s.encode() if isinstance(s, str) else bytes(s) for s in side]
            offsets = np.zeros(len(items) + 1, dtype=np.uint64)
            np.cumsum([len(s) for s in items], out=offsets[1:])
            out.write(struct.pack("<Q", len(items)) + offsets.tobytes() + b"".join(items))
        out.write(struct.pack("<I", len(requests)))
        for prepared, with_starts, bound, select in requests:
            out.write(struct.pack("<iiII", int(prepared), int(with_starts), bound, select))


def test_cpp_program_builds_and_fails_loudly_without_a_device(tmp_path):
    """The wrappers' program compiles against the header with warnings as errors; where no device is visible it ends with the
    library's status (no_device) on stderr and writes no result."""
    import torch
    binary = build_check_infix_all(tmp_path)
    if torch.cuda.is_available():
        return   # (with a device the program is run by test_binding_programs)
    write_program_case(tmp_path / "tiny.case", False, ["abc"], ["xxabcxx"], [(0, 1, 1, 0)])
    done = subprocess.run([str(binary), str(tmp_path / "tiny.case"), str(tmp_path / "tiny.out")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2 and "status 5" in done.stderr, (done.returncode, done.stderr)
    assert os.path.getsize(tmp_path / "tiny.out") == 0


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


def assert_csr(got, want, what):
    """`got`: an InfixOccurrences or (offsets, starts, ends, distances); `want`: expected_csr's. Exact, array by array."""
    if not isinstance(got, tuple):
        got = (got.offsets, got.starts, got.ends, got.distances)
    got = tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in got)   # (device tensors of an out= call)
    offsets = np.asarray(got[0], dtype=np.uint64)
    assert np.array_equal(offsets, want[0]), (what, "offsets", np.flatnonzero(np.diff(offsets.astype(np.int64)) != np.diff(want[0].astype(np.int64)))[:5])
    for name, have, expected in zip(("starts", "ends", "distances"), got[1:], want[1:]):
        if have is None:
            continue
        have = np.asarray(have, dtype=np.uint32)[:len(expected)]
        differs = np.flatnonzero(have != expected)
        if len(differs):
            h = int(differs[0])
            row = int(np.searchsorted(want[0], h, side="right")) - 1
            raise AssertionError((what, name, "hit", h, "row", row, "got", int(have[h]), "want", int(expected[h]), len(differs), "differ"))


def check_batch(sw, engine, scope, patterns, texts, bound, select, utf8=False, what=""):
    got = engine.infix_all(sw.Strs(patterns), sw.Strs(texts), scope, bound=bound, select=select)
    want = expected_csr(patterns, texts, bound, select, utf8)
    assert len(got.ends) == len(got.starts) == len(got.distances) == int(want[0][-1]), (what, bound, select, len(got.ends), int(want[0][-1]))
    assert_csr(got, want, (what, bound, select))
    return got, want


@pytest.mark.gpu
def test_examples(sw, scope, lev):
    for p, t, bound, select, want in EXAMPLES:
        got = lev.infix_all(sw.Strs([p]), sw.Strs([t]), scope, bound=bound, select=select)
        assert got[0] == [(d, s, e) for s, e, d in want], (p, t, bound, select, got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "code_points"])
def test_exhaustive_small_cases(sw, scope, lev, lev8, utf8):
    """Every pattern of up to 3 symbols against every text of up to 6 over two symbols, one batch per (bound, select). The code-point
    batch spells pair k's two symbols with two of the four letters of WIDE, so every UTF-8 width takes its turn."""
    pairs = [(p, t) for p in all_strings("ab", 3) for t in all_strings("ab", 6)]
    assert len(pairs) == 15 * 127
    if utf8:
        spell = lambda s, k: s.translate({ord("a"): WIDE[k % 4], ord("b"): WIDE[(k + 1 + k // 4 % 3) % 4]})
        pairs = [(spell(p, k), spell(t, k)) for k, (p, t) in enumerate(pairs)]
    patterns, texts = [p for p, _ in pairs], [t for _, t in pairs]
    totals = {}
    for bound in range(4):
        for select in SELECTS:
            _, want = check_batch(sw, lev8 if utf8 else lev, scope, patterns, texts, bound, select, utf8, "exhaustive")
            totals[bound, select] = int(want[0][-1])
    assert totals[3, "all"] == sum(len(t) + 1 for t in texts) and 0 < totals[0, "minima"] <= totals[0, "best"] <= totals[0, "all"] < totals[1, "all"]


EDGE_M = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 2047, 2048)
EDGE_N = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200)


def planted_text(rng, p, n):
    """n symbols: filler, a mutated copy of p written over its very start and another over its very end -- one over the other where
    the text is shorter than both, cut where it is shorter than one."""
    letter = lambda: int(rng.integers(97, 101))
    text = bytearray(rand_bytes(rng, n, 4, 97))
    first, second = (bytes(mutated(rng, p, int(rng.integers(0, 3)), letter)) for _ in range(2))
    text[:len(first)] = first[:n]
    if n:
        tail = second[-n:]
        text[n - len(tail):] = tail
    assert len(text) == n
    return bytes(text)


def edge_batch():
    rng = np.random.default_rng(51)
    patterns, texts = [], []
    for m in EDGE_M:
        p = rand_bytes(rng, m, 4, 97)
        for n in EDGE_N:
            patterns.append(p); texts.append(planted_text(rng, p, n))
    return patterns, texts


@pytest.mark.gpu
@pytest.mark.parametrize("select", SELECTS)
def test_block_and_step_edges(sw, scope, lev, select):
    """The score bit and the hand-over between blocks (m around multiples of 32, one lane to all 64) against the 16-symbol super-step
    (n around multiples of 16), with occurrences that touch both ends of the text. bound = m admits every column, e = 0 included."""
    patterns, texts = edge_batch()
    for bound in (0, 2):
        _, want = check_batch(sw, lev, scope, patterns, texts, bound, select, what="edges")
        assert int(want[0][-1]) > 100 and (np.diff(want[0].astype(np.int64)) == 0).any()
    for k, m in enumerate(EDGE_M):
        rows = slice(k * len(EDGE_N), (k + 1) * len(EDGE_N))
        _, want = check_batch(sw, lev, scope, patterns[rows], texts[rows], m, select, what=("edges", m))
        if select == "all":
            assert np.diff(want[0].astype(np.int64)).tolist() == [n + 1 for n in EDGE_N] and (want[2][want[0][:-1].astype(np.int64)] == 0).all()


@pytest.mark.gpu
def test_mixed_items(sw, scope, lev):
    """One run of 64 pairs whose patterns take 1, 2, 5 and 64 lanes in turn: items of several pairs with idle lanes beside items of one.
    Every other row is empty (a text over other letters), the first and the last among them."""
    rng = np.random.default_rng(52)
    patterns, texts = [], []
    for i in range(64):
        m = (20, 50, 150, 2048)[i % 4]
        p = rand_bytes(rng, m, 4, 97)
        if i % 2 == 0 or i == 63:
            t = rand_bytes(rng, rng.integers(0, 120), 4, 65)   # A..D: nothing within the bound
        else:
            t = rand_bytes(rng, rng.integers(0, 40), 4, 97) + p + rand_bytes(rng, 30, 4, 97)
            if m < 2048:   # (one copy in the long rows: the numpy reference stays in seconds)
                t += bytes(mutated(rng, p, 2, lambda: int(rng.integers(97, 101))))
        patterns.append(p); texts.append(t)
    for select in SELECTS:
        _, want = check_batch(sw, lev, scope, patterns, texts, 3, select, what="mixed")
        counts = np.diff(want[0].astype(np.int64))
        assert counts[0] == counts[-1] == 0 and (counts[::2] == 0).all() and (counts[1:63:2] > 0).all()


@pytest.mark.gpu
def test_text_tape_under_16_bytes(sw, scope, lev):
    """The forward walk reads a text tape of under 16 bytes word by word and a longer one with 128-bit loads."""
    patterns = [b"ab", b"", b"abc", b"b"]
    narrow, wide = [b"abab", b"xyz", b"", b"abcb"], [b"abab", b"xyz", b"", b"abcbabcabcab"]
    assert sum(map(len, narrow)) < 16 <= sum(map(len, wide))
    for texts in (narrow, wide):
        for select in SELECTS:
            check_batch(sw, lev, scope, patterns, texts, 1, select, what=("tape", sum(map(len, texts))))


@pytest.mark.gpu
def test_scan_tiles(sw, scope, lev):
    """9,000 rows: more than two tiles of the offsets scan and many waves of the walks; offsets and every hit compared."""
    rng = np.random.default_rng(53)
    words = [rand_bytes(rng, rng.integers(0, 9), 3, 97) for _ in range(300)]
    lines = [rand_bytes(rng, rng.integers(0, 25), 3, 97) for _ in range(400)]
    picks = rng.integers(0, 300, 9000), rng.integers(0, 400, 9000)
    patterns, texts = [words[i] for i in picks[0]], [lines[i] for i in picks[1]]
    got, want = check_batch(sw, lev, scope, patterns, texts, 1, "all", what="scan")
    assert int(want[0][-1]) > 3 * 4096 and (got.counts == 0).any()


@pytest.mark.gpu
def test_start_pass(sw, scope, lev):
    """Ends in front of the pattern's length, ends at exactly m + d, texts far longer than m + d; many rows' hits in one item of the
    start pass beside rows whose every hit takes a wave (2048 symbols); three planted occurrences in each of the long rows."""
    rng = np.random.default_rng(54)
    letter = lambda: int(rng.integers(97, 101))
    patterns, texts = [b"abcdef", b"abcdef", b"aaaa", b"abcabc"], [b"cdefxx", b"abcdefabcdefx", b"baaaaaab", b"abc"]
    for m in (33, 2048):
        for _ in range(2):
            p = rand_bytes(rng, m, 4, 97)
            copies = [bytes(mutated(rng, p, edits, letter)) for edits in (0, 1, 2)]
            patterns.append(p); texts.append(copies[0] + rand_bytes(rng, 700, 4, 97) + copies[1] + rand_bytes(rng, 5, 4, 97) + copies[2])
    for i in range(120):   # short rows with a few hits each: their hits share items
        p = rand_bytes(rng, rng.integers(1, 40), 3, 97)
        patterns.append(p); texts.append(rand_bytes(rng, rng.integers(0, 30), 3, 97) + p[:len(p) // 2] + rand_bytes(rng, rng.integers(0, 30), 3, 97) + p)
    for select in SELECTS:
        _, want = check_batch(sw, lev, scope, patterns, texts, 2, select, what="starts")
        starts, ends, distances = (x.astype(np.int64) for x in want[1:])
        rows = np.repeat(np.arange(len(patterns)), np.diff(want[0].astype(np.int64)))
        m = np.array([len(p) for p in patterns])[rows]
        assert (ends < m).any() and (ends == m + distances).any() and (ends > 4 * m).any()   # the pass runs min(e, m + d) columns
        assert all(int(want[0][r + 1] - want[0][r]) >= (1 if select == "best" else 3) for r in range(4, 8))


def raw_all(sw, engine, scope, patterns, texts, bound, select, outs, capacity, utf8=False):
    """The C ABI itself: raw u64 tapes, or prepared views where `patterns` is a PreparedTape. `outs`: four addresses (or None).
    Returns (status name, message)."""
    from stringwars_amd import _native as N
    if isinstance(patterns, sw.PreparedTape):
        vp, vt = patterns.view(), texts.view()
        fn, sides = N.lib.swh_levenshtein_infix_all_prepared, (C.byref(vp), C.byref(vt))
    else:
        tp, _, keep_p = sw.engines._c_tape(patterns, want64=True)
        tt, _, keep_t = sw.engines._c_tape(texts, want64=True)
        fn = N.lib.swh_levenshtein_utf8_infix_all_u64tape if utf8 else N.lib.swh_levenshtein_infix_all_u64tape
        sides = (C.byref(tp), C.byref(tt))
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, *sides, N.UNBOUNDED if bound is None else bound, SELECT_ID.get(select, select),
                *(C.c_void_p(o) for o in outs), capacity, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def protocol_batch():
    rng = np.random.default_rng(55)
    patterns, texts = [], []
    for i in range(240):
        p = rand_bytes(rng, rng.integers(0, 70), 4, 97)
        t = rand_bytes(rng, rng.integers(0, 200), 4, 97)
        if i % 2:
            at = int(rng.integers(0, len(t) + 1))
            t = t[:at] + bytes(mutated(rng, p, int(rng.integers(0, 3)), lambda: int(rng.integers(97, 101)))) + t[at:]
        patterns.append(p); texts.append(t)
    return patterns, texts


@pytest.mark.gpu
def test_counting_protocol_and_output_placement(sw, scope, lev):
    import torch
    patterns, texts = protocol_batch()
    sp, st = sw.Strs(patterns), sw.Strs(texts)
    count, bound = len(patterns), 2
    for select in SELECTS:
        want = expected_csr(patterns, texts, bound, select)
        total = int(want[0][-1])
        assert total > 50
        # the counting call: the offsets alone
        offsets = np.full(count + 1, SENTINEL, np.uint64)
        assert raw_all(sw, lev, scope, sp, st, bound, select, [offsets.ctypes.data, None, None, None], 0)[0] == "success"
        assert np.array_equal(offsets, want[0])
        counted = lev.infix_all(sp, st, scope, bound=bound, select=select, out=(np.zeros(count + 1, np.uint64), None, None, None))
        assert counted.ends is None and np.array_equal(counted.offsets, want[0])
        # exact capacity, then one short: offsets written, arrays untouched, success
        for room in (total, total - 1):
            offsets = np.full(count + 1, SENTINEL, np.uint64)
            arrays = [np.full(total + 1, SENTINEL, np.uint32) for _ in range(3)]
            status, message = raw_all(sw, lev, scope, sp, st, bound, select, [offsets.ctypes.data] + [a.ctypes.data for a in arrays], room)
            assert status == "success", message
            assert np.array_equal(offsets, want[0])
            if room == total:
                assert_csr((offsets, *arrays), want, ("exact", select))
                assert all(a[total] == SENTINEL for a in arrays)
            else:
                assert all((a == SENTINEL).all() for a in arrays)
        # starts = NULL: the start pass is skipped, ends and distances are the same
        offsets, ends, distances = np.zeros(count + 1, np.uint64), np.full(total, SENTINEL, np.uint32), np.full(total, SENTINEL, np.uint32)
        assert raw_all(sw, lev, scope, sp, st, bound, select, [offsets.ctypes.data, None, ends.ctypes.data, distances.ctypes.data], total)[0] == "success"
        assert_csr((offsets, None, ends, distances), want, ("no starts", select))
        bare = lev.infix_all(sp, st, scope, bound=bound, select=select, starts=False)
        assert bare.starts is None and bare[1] == [(d, None, e) for _, e, d in reference_hits(patterns[1], texts[1], bound, select)]
        assert_csr(bare, want, ("starts=False", select))
        # every output on the device; then offsets and ends on the device, starts and distances on the host
        device = [torch.zeros(count + 1, dtype=torch.int64, device="cuda")] + [torch.zeros(total, dtype=torch.int32, device="cuda") for _ in range(3)]
        assert raw_all(sw, lev, scope, sp, st, bound, select, [x.data_ptr() for x in device], total)[0] == "success"
        assert_csr(tuple(x.cpu().numpy() for x in device), want, ("device", select))
        filled = lev.infix_all(sp, st, scope, bound=bound, select=select, out=tuple(torch.zeros_like(x) for x in device))
        assert_csr(filled, want, ("out= tensors", select))
        assert filled[1] == [(d, s, e) for s, e, d in reference_hits(patterns[1], texts[1], bound, select)]
        d_offsets, d_ends = torch.zeros(count + 1, dtype=torch.int64, device="cuda"), torch.zeros(total, dtype=torch.int32, device="cuda")
        h_starts, h_distances = np.zeros(total, np.uint32), np.zeros(total, np.uint32)
        assert raw_all(sw, lev, scope, sp, st, bound, select, [d_offsets.data_ptr(), h_starts.ctypes.data, d_ends.data_ptr(), h_distances.ctypes.data],
                       total)[0] == "success"
        assert_csr((d_offsets.cpu().numpy(), h_starts, d_ends.cpu().numpy(), h_distances), want, ("mixed", select))
        # the Python call grows its arrays when the first room is too small
        assert_csr(lev.infix_all(sp, st, scope, bound=bound, select=select, capacity=3), want, ("capacity=3", select))
    # raw device tapes; prepared tapes in all four offset-width mixes, whole and as sub-views
    want = expected_csr(patterns, texts, bound, "all")
    assert_csr(lev.infix_all(sp.to_device(scope), st.to_device(scope), scope, bound=bound), want, "device tapes")
    tapes = {(w, name): sw.PreparedTape(scope, sw.Strs(items).with_offsets(w)) for w in (np.uint32, np.uint64) for name, items in (("p", patterns), ("t", texts))}
    sub = expected_csr(patterns[37:201], texts[37:201], bound, "all")
    for wp, wt in itertools.product((np.uint32, np.uint64), repeat=2):
        assert_csr(lev.infix_all(tapes[wp, "p"], tapes[wt, "t"], scope, bound=bound), want, ("prepared", wp, wt))
        assert_csr(lev.infix_all(tapes[wp, "p"][37:201], tapes[wt, "t"][37:201], scope, bound=bound), sub, ("sub-view", wp, wt))
    # bound = None: no cutoff, every column of every text under "all"
    unbounded = lev.infix_all(sp, st, scope, select="all", starts=False)
    assert unbounded.counts.tolist() == [len(t) + 1 for t in texts]
    # count == 0: row_offsets[0] = 0 and nothing else
    offsets, arrays = np.full(2, SENTINEL, np.uint64), [np.full(2, SENTINEL, np.uint32) for _ in range(3)]
    assert raw_all(sw, lev, scope, sw.Strs([]), sw.Strs([]), 1, "all", [offsets.ctypes.data] + [a.ctypes.data for a in arrays], 2)[0] == "success"
    assert offsets.tolist() == [0, SENTINEL] and all((a == SENTINEL).all() for a in arrays)
    empty = lev.infix_all(sw.Strs([]), sw.Strs([]), scope, bound=1)
    assert len(empty) == 0 and len(empty.ends) == 0
    # profiling: cells counted once, the stamps named after the walks
    scope.set_profiling(True)
    try:
        lev.infix_all(sp, st, scope, bound=bound)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["cells"] == int((sp.lengths * st.lengths).sum()) and timing["kernels"] >= 5   # sizes, two walks, the scan, the start pass


@pytest.mark.gpu
def test_refusals(sw, scope, lev, lev8):
    rng = np.random.default_rng(56)
    offsets, arrays = np.full(8, SENTINEL, np.uint64), [np.full(64, SENTINEL, np.uint32) for _ in range(3)]
    pointers = [offsets.ctypes.data] + [a.ctypes.data for a in arrays]
    untouched = lambda: (offsets == SENTINEL).all() and all((a == SENTINEL).all() for a in arrays)
    good_p, good_t = sw.Strs([b"abc", b"b"]), sw.Strs([b"xxabcxx", b"abab"])
    # NULL mixes and a bad select: invalid_argument, nothing written
    s, e, d = pointers[1:]
    for outs, capacity in (([None, s, e, d], 64), ([pointers[0], s, None, d], 64), ([pointers[0], s, e, None], 64), ([pointers[0], s, None, None], 0),
                           ([pointers[0], None, None, None], 64)):
        status, message = raw_all(sw, lev, scope, good_p, good_t, 1, "all", outs, capacity)
        assert status == "invalid_argument" and message and untouched(), (outs, status)
    assert raw_all(sw, lev, scope, good_p, good_t, 1, 3, pointers, 64)[0] == "invalid_argument" and untouched()
    with pytest.raises(ValueError):
        lev.infix_all(good_p, good_t, scope, bound=1, select="first")
    # an oversize pattern: before any output, naming its pair
    patterns = [b"abc", rand_bytes(rng, 2048, 4, 97), rand_bytes(rng, 2049, 4, 97), b"abc", rand_bytes(rng, 3000, 4, 97)]
    texts = [b"xxabcxx", rand_bytes(rng, 100, 4, 97), rand_bytes(rng, 100, 4, 97), b"", b"abc"]
    status, message = raw_all(sw, lev, scope, sw.Strs(patterns), sw.Strs(texts), 1, "all", pointers, 64)
    assert status == "unsupported_length" and "pair 2" in message and "2049" in message and untouched(), message
    with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
        lev.infix_all(sw.Strs(patterns), sw.Strs(texts), scope, bound=1)
    assert "pair 2" in str(info.value)
    check_batch(sw, lev, scope, patterns[:2], texts[:2], 1, "all", what="2048 symbols are accepted")
    # count mismatch, costs, UTF-8, tapes of two kinds
    assert raw_all(sw, lev, scope, sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), 1, "all", pointers, 64)[0] == "invalid_argument" and untouched()
    with pytest.raises(ValueError):
        lev.infix_all(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope, bound=1)
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    assert raw_all(sw, costly, scope, good_p, good_t, 1, "all", pointers, 64)[0] == "not_implemented" and untouched()
    for bad_p, bad_t in (([b"ok", b"\xff\xfe"], [b"ok", b"x"]), ([b"ok", b"x"], [b"ok", b"\xc3"])):
        assert raw_all(sw, lev8, scope, sw.Strs(bad_p), sw.Strs(bad_t), 1, "all", pointers, 64, utf8=True)[0] == "invalid_utf8" and untouched()
    as_bytes, as_utf8 = sw.PreparedTape(scope, good_p), sw.PreparedTape(scope, good_t, utf8=True)
    assert raw_all(sw, lev, scope, as_bytes, as_utf8, 1, "all", pointers, 64)[0] == "invalid_argument" and untouched()
    with pytest.raises(ValueError):
        lev.infix_all(as_bytes, as_utf8, scope, bound=1)
    # null handles where a device is visible
    from stringwars_amd import _native as N
    tp, _, keep_p = sw.engines._c_tape(good_p, want64=True)
    err = C.c_char_p()
    status = N.lib.swh_levenshtein_infix_all_u64tape(None, None, C.byref(tp), C.byref(tp), 1, 0, *(C.c_void_p(x) for x in pointers), 64, C.byref(err))
    assert N.STATUS_NAMES[status] == "invalid_argument" and err.value and untouched()


@pytest.mark.gpu
def test_determinism(sw, scope, lev):
    patterns, texts = protocol_batch()
    tp, tt = sw.PreparedTape(scope, sw.Strs(patterns)), sw.PreparedTape(scope, sw.Strs(texts))
    for select in SELECTS:
        first, second = (lev.infix_all(tp, tt, scope, bound=3, select=select) for _ in range(2))
        assert len(first.ends) > 50
        assert all(getattr(first, name).tobytes() == getattr(second, name).tobytes() for name in ("offsets", "starts", "ends", "distances")), select


@pytest.mark.gpu
def test_consistency_with_infix_and_between_selects(sw, scope, lev):
    rng = np.random.default_rng(57)
    patterns, texts = [], []
    for i in range(2000):
        p = rand_bytes(rng, rng.integers(0, 100), 4, 97)
        t = rand_bytes(rng, rng.integers(0, 400), 4, 97)
        if i % 2:
            at = int(rng.integers(0, len(t) + 1))
            t = t[:at] + bytes(mutated(rng, p, int(rng.integers(0, 5)), lambda: int(rng.integers(97, 101)))) + t[at:]
        patterns.append(p); texts.append(t)
    tp, tt = sw.PreparedTape(scope, sw.Strs(patterns)), sw.PreparedTape(scope, sw.Strs(texts))
    bound = 6
    single = lev.infix(tp, tt, scope, bound=bound)
    rows = {select: lev.infix_all(tp, tt, scope, bound=bound, select=select) for select in SELECTS}
    found = 0
    for i in range(2000):
        every, best, minima = (rows[select][i] for select in SELECTS)
        assert set(best) <= set(every) and set(minima) <= set(every), i
        assert [h[2] for h in every] == sorted({h[2] for h in every}), i   # ascending ends, each once
        if single[i] is None:
            assert best == [] and every == [] and minima == [], i
        else:
            assert best[0] == single[i] and best == [h for h in every if h[0] == best[0][0]], i
            assert min(h[0] for h in every) == best[0][0] and [h for h in minima if h[0] == best[0][0]][0] == best[0], i
            found += 1
    assert 500 < found < 2000


@pytest.mark.gpu
def test_utf8_lines(sw, scope, lev8):
    """A word of every golden line searched in its line, positions in code points."""
    rng = np.random.default_rng(58)
    patterns, texts = [], []
    for line in golden_lines():
        words = [w for w in line.split() if len(w) >= 2]
        for k, w in enumerate(words[3::max(1, len(words) // 8)][:8]):
            patterns.append("".join(mutated(rng, w, k % 2, lambda: line[int(rng.integers(0, len(line)))]))); texts.append(line)
    assert len(patterns) >= 100 and any(len(t.encode()) > len(t) for t in texts)
    for bound in (0, 1):
        for select in SELECTS:
            _, want = check_batch(sw, lev8, scope, patterns, texts, bound, select, utf8=True, what="utf8")
            assert int(want[0][-1]) >= 50
    prepared = lev8.infix_all(sw.PreparedTape(scope, sw.Strs(patterns), utf8=True), sw.PreparedTape(scope, sw.Strs(texts), utf8=True), scope, bound=1)
    assert_csr(prepared, expected_csr(patterns, texts, 1, "all", True), "utf8 prepared")


@pytest.mark.gpu
def test_seeded_random_round(sw, scope, lev):
    """3,000 pairs in three batches of a random select each; bound = m // 4 is a value of the pair, so each batch runs per bound."""
    rng = np.random.default_rng(2028)
    count = 3000
    rows = rng.integers(1, 301, size=count)
    columns = (1501 * rng.random(count) ** 4).astype(np.int64)   # 0 .. 1500, most of them short: the numpy reference stays in seconds
    selects = [SELECTS[int(k)] for k in rng.integers(0, 3, size=3)]
    patterns = [rand_bytes(rng, m, 4, 97) for m in rows]
    texts = [rand_bytes(rng, n, 4, 97) for n in columns]
    assert rows.min() == 1 and rows.max() == 300 and columns.min() == 0 and columns.max() > 1200
    # every random number is drawn: the device comes now
    hits_under_all = 0
    for batch, select in enumerate(selects):
        members = np.arange(batch * 1000, (batch + 1) * 1000)
        for bound in np.unique(rows[members] // 4):
            chosen = [int(i) for i in members if rows[i] // 4 == bound]
            check_batch(sw, lev, scope, [patterns[i] for i in chosen], [texts[i] for i in chosen], int(bound), select, what=("random", batch))
    for i in range(count):
        hits_under_all += len(select_ends(_ROWS[patterns[i], texts[i], False][2], int(rows[i]) // 4, "all"))
    total_columns = int(columns.sum()) + count
    assert 0 < hits_under_all < 0.05 * total_columns, (hits_under_all, total_columns)


@pytest.mark.gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_binding_programs(tmp_path, utf8):
    """Both overloads of LevenshteinDistances::infix_all (stringwars_amd.hpp) from a C++ program -- raw tape views and prepared tapes, the
    three selects, with and without starts: a counting call, then a filled call with exactly that room -- and check_c's lines for the
    three exports. What the C++ program writes equals the reference exactly."""
    binary = build_check_infix_all(tmp_path)
    patterns, texts = protocol_batch()
    if utf8:
        spell = lambda s: bytes(s).decode().translate({97 + k: WIDE[k] for k in range(4)})
        patterns, texts = [spell(p) for p in patterns[:120]], [spell(t) for t in texts[:120]]
    requests = [(prepared, with_starts, 2, SELECT_ID[select]) for prepared in (0, 1) for select in SELECTS for with_starts in (1, 0)]
    write_program_case(tmp_path / "batch.case", utf8, patterns, texts, requests)
    done = subprocess.run([str(binary), str(tmp_path / "batch.case"), str(tmp_path / "batch.out")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    raw = open(tmp_path / "batch.out", "rb").read()
    at = 0
    for prepared, with_starts, bound, select in requests:
        want = expected_csr(patterns, texts, bound, SELECTS[select], utf8)
        total = int(want[0][-1])
        arrays = []
        for dtype, entries in [(np.uint64, len(patterns) + 1)] * 2 + [(np.uint32, total)] * (3 if with_starts else 2):
            arrays.append(np.frombuffer(raw, dtype=dtype, count=entries, offset=at))
            at += arrays[-1].nbytes
        assert np.array_equal(arrays[0], want[0]), ("the counting call", prepared, select)
        got = (arrays[1], arrays[2] if with_starts else None, arrays[-2], arrays[-1])
        assert_csr(got, want, ("C++ infix_all", utf8, prepared, with_starts, select))
    assert at == len(raw)
    if not utf8:
        from test_bindings import CHECK_C, run_program, the_case, write_case   # (the case is computed once per session and shared)
        write_case(tmp_path / "bindings.case", the_case())
        done, lines = run_program(CHECK_C, tmp_path / "bindings.case")
        assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
        for name in ("swh_levenshtein_infix_all_u64tape", "swh_levenshtein_utf8_infix_all_u64tape", "swh_levenshtein_infix_all_prepared"):
            assert lines.get("nodevice." + name) == "ok", (name, lines.get("nodevice." + name))
