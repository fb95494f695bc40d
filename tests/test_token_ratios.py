"""Token-sorted tapes, token_sort_ratio and token_set_ratio (swh_tape_token_sort, swh_prepared_read, swh_levenshtein_token_set_pairs_*):
rapidfuzz's fuzz.token_sort_ratio and fuzz.token_set_ratio.

The contract is include/stringwars_amd.h's. Tokens are what Python's split() returns -- bytes.split() on a byte tape, str.split() on
a UTF-8 tape --, their order is sorted()'s, the two normal forms are " ".join(sorted(s.split())) and " ".join(sorted(set(s.split()))),
and token_set_ratio is evaluated on the host from four integers: the symbols s, x, y of the joined intersection and differences of
the two token sets and L = LCS(X, Y).

The reference lives here and is Python's own split(), sorted() and set(), test_lcs.py's numpy LCS table and the score expressions
written operation by operation. It is pinned on the header's worked rows. Every comparison is exact: the derived tapes' bytes and
offsets, the counts as integers, the float64 scores bit for bit. No rapidfuzz exists where these tests run."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV
from test_lcs import reference_lcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE, PACKAGE = os.path.join(ROOT, "include"), os.path.join(ROOT, "stringwars_amd")
gpu = pytest.mark.gpu

TOKEN_SYMBOLS = ("swh_tape_token_sort", "swh_prepared_read", "swh_levenshtein_token_set_pairs_u64tape",
                 "swh_levenshtein_utf8_token_set_pairs_u64tape", "swh_levenshtein_token_set_pairs_prepared")
TOKEN_SET_SYMBOLS = TOKEN_SYMBOLS[2:]
METHODS = ("token_sort_ratio", "token_sort_ratio_cross", "token_set_counts", "token_set_ratio", "_token_set_score")
# a, b, token_sort_ratio, (s, x, y, L), token_set_ratio: the worked rows of include/stringwars_amd.h, the floats as the issue printed them
ROWS = [("fuzzy was a bear", "fuzzy fuzzy was a bear", 84.21052631578948, (16, 0, 0, 0), 100.0),
        ("mariners vs angels", "los angeles angels of anaheim at seattle mariners", 50.74626865671642, (15, 2, 33, 1), 90.9090909090909),
        ("york new", "new jersey", 33.333333333333336, (3, 4, 6, 1), 55.55555555555556),
        ("a a b", "b c", 25.0, (1, 1, 1, 0), 66.66666666666667),
        ("  b  a ", "a\tb\n", 100.0, (3, 0, 0, 0), 100.0),
        ("", "", 100.0, (0, 0, 0, 0), 0.0),
        ("   ", "a", 0.0, (0, 0, 1, 0), 0.0)]
# str.isspace(), as the header lists it, and its UTF-8 sequences
SPACES = set(range(0x09, 0x0E)) | set(range(0x1C, 0x21)) | {0x85, 0xA0, 0x1680} | set(range(0x2000, 0x200B)) | {0x2028, 0x2029, 0x202F, 0x205F, 0x3000}
SPACE_SEQUENCES = ([bytes([c]) for c in range(0x09, 0x0E)] + [bytes([c]) for c in range(0x1C, 0x21)] + [b"\xC2\x85", b"\xC2\xA0", b"\xE1\x9A\x80"] +
                   [bytes([0xE2, 0x80, c]) for c in range(0x80, 0x8B)] + [b"\xE2\x80\xA8", b"\xE2\x80\xA9", b"\xE2\x80\xAF", b"\xE2\x81\x9F", b"\xE3\x80\x80"])
BYTE_SPACES = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20}
LOOK_ALIKES = ("\u200b", "\u180e", "\ufeff", "\u0084", "\u00a1")


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def joined(tokens):
    """One 0x20 between the tokens (of bytes or of str)."""
    tokens = list(tokens)
    return (b" " if tokens and isinstance(tokens[0], bytes) else " ").join(tokens) if tokens else None


def normal_form(s, unique):
    tokens = s.split()
    out = joined(sorted(set(tokens)) if unique else sorted(tokens))
    return out if out is not None else s[:0]


def ratio_of(m, n, lcs) -> float:
    """engine.ratio's expression: 200 L / (d + 2 L) with d = m + n - 2 L, 100 for two empty strings."""
    twice = 2.0 * float(lcs)
    total = float(m + n - 2 * lcs) + twice
    return 100.0 * twice / total if total > 0 else 100.0


def q(d, t) -> float:
    return 100.0 * float(t - d) / float(t) if t > 0 else 100.0


def set_score(s, x, y, L) -> float:
    """The header's definition, operation by operation."""
    if s == 0 and (x == 0 or y == 0):
        return 0.0
    if s > 0 and (x == 0 or y == 0):
        return 100.0
    e = 1 if s > 0 else 0
    sab, sba = s + e + x, s + e + y
    r = q(x + y - 2 * L, sab + sba)
    return r if s == 0 else max(r, q(e + x, s + sab), q(e + y, s + sba))


def set_parts(a, b):
    """S, X, Y of one pair: the joined sorted A & B, A - B and B - A."""
    A, B = set(a.split()), set(b.split())
    empty = a[:0]
    return tuple(joined(sorted(part)) or empty for part in (A & B, A - B, B - A))


def reference(a, b, utf8, sort=True):
    """(token_sort_ratio, counts (n, 4), token_set_ratio) of the pairs; the items are str with utf8, else bytes. Without `sort` the
    first is None."""
    sort_ratio = None
    if sort:
        sa, sb = [normal_form(x, False) for x in a], [normal_form(x, False) for x in b]
        lcs = reference_lcs(sa, sb, utf8)
        sort_ratio = np.array([ratio_of(len(x), len(y), int(l)) for x, y, l in zip(sa, sb, lcs)], dtype=np.float64)
    parts = [set_parts(x, y) for x, y in zip(a, b)]
    L = reference_lcs([p[1] for p in parts], [p[2] for p in parts], utf8) if parts else np.zeros(0, np.int64)
    counts = np.array([[len(p[0]), len(p[1]), len(p[2]), int(l)] for p, l in zip(parts, L)], dtype=np.int64).reshape(len(parts), 4)
    set_ratio = np.array([set_score(*(int(v) for v in row)) for row in counts], dtype=np.float64)
    return sort_ratio, counts, set_ratio


def as_items(strings, utf8):
    """The test's strings (str) as the mode takes them: str on a UTF-8 tape, their UTF-8 bytes on a byte tape."""
    return [s if utf8 or isinstance(s, bytes) else s.encode() for s in strings]


def raw(items):
    return [x.encode() if isinstance(x, str) else bytes(x) for x in items]


def same_bits(got, want):
    return got.dtype == np.float64 and got.shape == want.shape and (got.view(np.uint64) == want.view(np.uint64)).all()


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in TOKEN_SYMBOLS:
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    for name in METHODS:
        assert callable(getattr(sw.LevenshteinDistances, name)), name
        assert getattr(sw.LevenshteinDistancesUTF8, name) is getattr(sw.LevenshteinDistances, name), name
    assert callable(sw.PreparedTape.token_sorted) and callable(sw.PreparedTape.to_strs)
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_TOKEN_MAX_BYTES 4096u", header) and N.TOKEN_MAX_BYTES == 4096 == sw.TOKEN_MAX_BYTES
    assert re.search(r"#define SWH_TOKENS_SORTED 0\b", header) and re.search(r"#define SWH_TOKENS_UNIQUE 1\b", header)
    assert (N.TOKENS_SORTED, N.TOKENS_UNIQUE) == (0, 1)
    test_library = C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    assert all(hasattr(test_library, name) for name in TOKEN_SYMBOLS)
    rust = open(os.path.join(ROOT, "stringwars_amd", "rust", "src", "lib.rs")).read()
    cxx = open(os.path.join(ROOT, "include", "stringwars_amd.hpp")).read()
    assert all("fn %s(" % name in rust and name in cxx for name in TOKEN_SYMBOLS)
    assert "token_set_score" in cxx and "TokenSetCounts" in cxx and "fn token_set_score" in rust


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        return   # (with a device the refusals are test_length_cap_and_refusals')
    ta, _, keep_a = sw.engines._c_tape(sw.Strs([b"b a"]), want64=True)
    tb, _, keep_b = sw.engines._c_tape(sw.Strs([b"a b"]), want64=True)
    out = np.full(4, 77, np.uint32)
    view = N.PreparedView(None, 0, 1)
    for name in TOKEN_SET_SYMBOLS:
        sides = (C.byref(view), C.byref(view)) if name.endswith("_prepared") else (C.byref(ta), C.byref(tb))
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, *sides, *(C.c_void_p(out[k:].ctypes.data) for k in range(4)), 0, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    handle, err = C.c_void_p(), C.c_char_p()
    assert N.STATUS_NAMES[N.lib.swh_tape_token_sort(None, C.byref(view), 0, C.byref(handle), C.byref(err))] == "no_device" and not handle.value
    offsets, err = np.full(2, 77, np.uint64), C.c_char_p()
    assert N.STATUS_NAMES[N.lib.swh_prepared_read(None, None, None, C.c_void_p(offsets.ctypes.data), C.byref(err))] == "no_device" and err.value
    assert (out == 77).all() and (offsets == 77).all()
    engine = object.__new__(sw.LevenshteinDistances)
    for method in ("token_sort_ratio", "token_sort_ratio_cross", "token_set_counts", "token_set_ratio"):
        with pytest.raises(ValueError):   # the Python front end asks for a scope before anything else
            getattr(engine, method)([b"a"], [b"b"], None)


def test_reference_reproduces_the_worked_rows():
    for utf8 in (False, True):
        a, b = as_items([r[0] for r in ROWS], utf8), as_items([r[1] for r in ROWS], utf8)
        sort_ratio, counts, set_ratio = reference(a, b, utf8)
        assert same_bits(sort_ratio, np.array([r[2] for r in ROWS]))
        assert counts.tolist() == [list(r[3]) for r in ROWS]
        assert same_bits(set_ratio, np.array([r[4] for r in ROWS]))
    assert normal_form(b"  b  a b ", False) == b"a b b" and normal_form("  b  a b ", True) == "a b" and normal_form(b" \t", True) == b""


def test_whitespace_sets_are_pythons():
    assert {c for c in range(0x110000) if chr(c).isspace()} == SPACES and len(SPACES) == 29
    assert sorted(SPACE_SEQUENCES) == sorted(chr(c).encode() for c in SPACES)
    assert {c for c in range(256) if bytes([c]).split() == []} == BYTE_SPACES
    for look_alike in LOOK_ALIKES:
        assert ("a" + look_alike + "b").split() == ["a" + look_alike + "b"]
    for byte in (0x1C, 0x1D, 0x1E, 0x1F, 0x85, 0xA0):
        assert (b"a" + bytes([byte]) + b"b").split() == [b"a" + bytes([byte]) + b"b"]


def test_host_score_equals_the_definition(sw):
    cases = [(s, x, y, L) for s, x, y in itertools.product(range(7), repeat=3) for L in range(min(x, y) + 1)]
    columns = [np.array([c[k] for c in cases], dtype=np.uint32) for k in range(4)]
    got = sw.LevenshteinDistances._token_set_score(*columns)
    assert same_bits(got, np.array([set_score(*c) for c in cases], dtype=np.float64))


def build_check_tokens(tmp_path):
    """tests/bindings/check_tokens.cpp against include/stringwars_amd.hpp and the shipped library."""
    binary = tmp_path / "check_tokens"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "tests", "bindings", "check_tokens.cpp"),
                    "-o", str(binary), "-L", PACKAGE, "-lstringwars_amd", f"-Wl,-rpath,{PACKAGE}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True, timeout=300)
    return binary


def write_case(path, utf8, a, b):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", int(utf8)))
        for strs in (a, b):
            items = raw(strs)
            offsets = np.cumsum([0] + [len(x) for x in items]).astype("<u8")
            f.write(struct.pack("<Q", len(items)) + offsets.tobytes() + b"".join(items))


def test_cpp_wrappers_build_and_refuse_without_device(tmp_path):
    import torch
    binary = build_check_tokens(tmp_path)
    if torch.cuda.is_available():
        return   # (run on the device by test_cpp_wrappers)
    write_case(tmp_path / "case", False, [b"b a"], [b"a b"])
    done = subprocess.run([str(binary), str(tmp_path / "case"), str(tmp_path / "result")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2 and "status" in done.stderr, (done.returncode, done.stderr)


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


def assert_tape(strs, want_items):
    """A Strs read back from the device holds exactly these strings: the bytes, and the offsets from 0."""
    want = raw(want_items)
    assert strs.offsets.dtype == np.uint64 and strs.offsets.tolist() == np.cumsum([0] + [len(x) for x in want]).tolist()
    assert strs.data.tobytes() == b"".join(want)


def check_derived(sw, scope, items, utf8, source=None):
    """Both normal forms of the items, derived on the device from `source` (default: a tape prepared from them), against Python."""
    tape = source if source is not None else sw.PreparedTape(scope, sw.Strs(items), utf8=utf8)
    for unique in (False, True):
        derived = tape.token_sorted(unique=unique)
        assert isinstance(derived, sw.PreparedTape) and len(derived) == len(items) and derived.utf8 == utf8
        want = [normal_form(x, unique) for x in items]
        assert_tape(derived.to_strs(), want)
        info = derived.info
        assert info["count"] == len(items) and info["bytes"] == sum(len(x) for x in raw(want)) and info["utf8"] == utf8
        assert info["symbols"] == sum(len(x) for x in want) and info["longest"] == max([len(x) for x in want], default=0)
        derived.free()


def check_scores(engine, scope, a, b, utf8, sort=True, want=None):
    """token_sort_ratio (with `sort`), token_set_counts and token_set_ratio of the pairs against the reference (`want`: computed
    already); returns the counts."""
    sort_ratio, counts, set_ratio = want if want is not None else reference(a, b, utf8, sort)
    if sort:
        assert same_bits(engine.token_sort_ratio(a, b, scope), sort_ratio)
    got = engine.token_set_counts(a, b, scope)
    assert all(g.dtype == np.uint32 for g in got) and np.array_equal(np.stack(got, axis=1).astype(np.int64).reshape(len(a), 4), counts)
    assert same_bits(engine.token_set_ratio(a, b, scope), set_ratio)
    return counts


@gpu
def test_worked_rows(sw, scope, lev, lev8):
    for utf8, engine in ((False, lev), (True, lev8)):
        a, b = as_items([r[0] for r in ROWS], utf8), as_items([r[1] for r in ROWS], utf8)
        check_derived(sw, scope, a + b, utf8)
        assert same_bits(engine.token_sort_ratio(a, b, scope), np.array([r[2] for r in ROWS]))
        assert np.array_equal(np.stack(engine.token_set_counts(a, b, scope), axis=1), np.array([r[3] for r in ROWS], dtype=np.uint32))
        assert same_bits(engine.token_set_ratio(a, b, scope), np.array([r[4] for r in ROWS]))
        check_scores(engine, scope, a, b, utf8)


@gpu
def test_exhaustive_small_strings(sw, scope, lev, lev8):
    """Every string over {a, b, space, tab} of up to 7 symbols through both forms; all ordered pairs of those up to 4 through the split."""
    strings = ["".join(t) for n in range(8) for t in itertools.product("ab \t", repeat=n)]
    assert len(strings) == 21845
    short = [s for s in strings if len(s) <= 4]
    a, b = [x for x in short for _ in short], [y for _ in short for y in short]
    want = reference(a, b, True, sort=False)   # (ASCII: the same counts in both modes)
    for utf8, engine in ((False, lev), (True, lev8)):
        check_derived(sw, scope, as_items(strings, utf8), utf8)
        check_scores(engine, scope, as_items(a, utf8), as_items(b, utf8), utf8, sort=False, want=want)


def token_count_cases(rng):
    """Strings of 0 .. 2048 tokens and the orders and ties that the sort and the dedupe can get wrong; small: those of at most 256 bytes."""
    letters = [chr(c) for c in range(ord("a"), ord("z") + 1)]
    cases = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 2048):   # one-byte tokens, one space: 2048 of them are 4095 bytes
        cases.append(" ".join(letters[int(k)] for k in rng.integers(0, 26, n)))
    pairs = [x + y for x in letters for y in letters]
    cases.append(" ".join(pairs[int(k)] for k in rng.integers(0, len(pairs), 1024)))   # 1024 tokens, most of them repeated somewhere
    cases.append(" ".join(pairs[int(k)] for k in rng.permutation(len(pairs))[:100]) + "\t")
    prefixes = ["abcdefghij"[:k] for k in range(1, 11)] + ["ab", "abc", "b", "ba"]
    cases.append(" ".join(prefixes[int(k)] for k in rng.permutation(len(prefixes))))
    cases.append(" ".join(["x" * 64 + "b", "x" * 64 + "a", "x" * 64, "x" * 70, "x" * 64 + "a", "x" * 63, "x" * 64 + "ab"]))
    cases.append(" ".join(["dup"] * 300 + ["d", "dupe"] + ["dup"] * 40 + ["a"]))
    cases.append(" ".join(["same"] * 50))
    ordered = sorted(pairs[:200])
    cases += [" ".join(ordered), " ".join(reversed(ordered)), "  ".join(ordered[:80]), "\n".join(reversed(ordered[:80]))]
    cases.append("y" * 4096)
    cases.append("é z 中 \U0001d11e \uff5e é é a \U00010000")   # byte order is code-point order
    return cases


@gpu
def test_token_count_edges(sw, scope, lev, lev8):
    rng = np.random.default_rng(17)
    cases = token_count_cases(rng)
    assert max(len(c.encode()) for c in cases) == 4096 and max(len(c.split()) for c in cases) == 2048
    small = [c for c in cases if len(c.encode()) <= 256]
    assert {len(c.split()) for c in small} >= {0, 1, 2, 63, 64, 65, 127, 128}
    for utf8, engine in ((False, lev), (True, lev8)):
        check_derived(sw, scope, as_items(small, utf8), utf8)    # the launch for short strings
        check_derived(sw, scope, as_items(cases, utf8), utf8)    # ... and for long ones
        # every case against a part of itself with a few tokens of its own: sets of up to 676 tokens, shared and not
        others = []
        for c in cases:
            tokens = c.split()
            keep = [t for k, t in enumerate(tokens) if k % 3 != 1][:600]
            extra = ["new", "x" * 64 + "a", "zz"]
            others.append(" ".join(keep + extra if len(" ".join(keep + extra).encode()) <= 4096 else extra))
        for a, b in ((cases, others), (small, list(reversed(small)))):
            assert all(min(len(normal_form(x, True)), len(normal_form(y, True))) <= 2048 for x, y in zip(a, b))
            check_scores(engine, scope, as_items(a, utf8), as_items(b, utf8), utf8, sort=False)


def chunk_edge_cases(offsets):
    """Whitespace runs, two- and three-byte spaces, token boundaries and the look-alikes laid at every one of the byte offsets."""
    features = ["  \t ", " ", "\u0085", "\u00a0", "\u1680", "\u2000", "\u2003", "\u200a", "\u2028", "\u2029", "\u202f", "\u205f", "\u3000",
                "\u00a0\u3000", "\x1c", "\x1f"]
    cases = []
    for k in offsets:
        for f in features:
            cases.append("b" * k + f + "ab" + f + "a")
            cases.append("c" * (k - 1) + " " + f + "a" + f)
        for f in LOOK_ALIKES:
            cases.append("b" * k + f + "a b" + f)
        cases.append("b" * (k - 2) + "é" + "\u3000" + "é")
    return cases


@gpu
@pytest.mark.parametrize("offsets", [range(60, 69), range(252, 261)], ids=["64", "256"])
def test_chunk_edges(sw, scope, lev, lev8, offsets):
    cases = chunk_edge_cases(offsets)
    others = [c[::-1] if c.isascii() else c[1:] + " b" for c in cases]
    for utf8, engine in ((False, lev), (True, lev8)):
        a, b = as_items(cases, utf8), as_items(others, utf8)
        if not utf8:   # raw bytes that are whitespace only as code points, or never: they stay inside their tokens
            for k in offsets:
                a += [b"b" * k + bytes([byte]) + b"a b" for byte in (0x1C, 0x1F, 0x85, 0xA0, 0xC2, 0xE2)]
                a += [b"b" * k + b"\x0b" + b"a" + b"\x0c\r" + b"a"]
            b += a[len(b):][::-1]
        check_derived(sw, scope, a, utf8)
        check_scores(engine, scope, a, b, utf8)


@gpu
@pytest.mark.parametrize("count", [4095, 4096, 4097, 8193])
def test_scan_tile_edges(sw, scope, count):
    """Tapes of as many strings as the offsets scan's tile of 4096 values holds, one less, one more, and one more than two tiles: the
    lengths of the normal forms are its only u32 input scanned without a second copy of the starts. One to three short tokens a string,
    some repeated, every seventh string empty or blank; both forms in full against Python."""
    rng = np.random.default_rng(count)
    words = ["a", "b", "ab", "ba", "abc", "zz", "é", "中"]
    items = []
    for i in range(count):
        tokens = [words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(1, 4)))]
        items.append(("", " ", "\t ")[i % 3] if i % 7 == 3 else (" ", "  ", "\n")[i % 3].join(tokens) + ("", " ")[i % 2])
    assert {len(s.split()) for s in items} == {0, 1, 2, 3}
    for utf8 in (False, True):
        check_derived(sw, scope, as_items(items, utf8), utf8)


@gpu
def test_length_cap_and_refusals(sw, scope, lev, lev8):
    from stringwars_amd import _native as N
    fits, over = b"ab " * 1365 + b"a", b"ab " * 1365 + b"ab"
    assert (len(fits), len(over)) == (4096, 4097)
    check_derived(sw, scope, [b"a", fits], False)
    tape = sw.PreparedTape(scope, sw.Strs([b"b a", fits, over, b"x" * 5000]))
    for form in (N.TOKENS_SORTED, N.TOKENS_UNIQUE):
        handle, err, view = C.c_void_p(), C.c_char_p(), tape.view()
        status = N.lib.swh_tape_token_sort(scope.handle, C.byref(view), form, C.byref(handle), C.byref(err))
        assert N.STATUS_NAMES[status] == "unsupported_length" and not handle.value
        assert b"string 2" in err.value and b"4097" in err.value
    view = tape[3:4].view()   # the index is the view's
    assert N.STATUS_NAMES[N.lib.swh_tape_token_sort(scope.handle, C.byref(view), 0, C.byref(handle), C.byref(err))] == "unsupported_length"
    assert b"string 0" in err.value and b"5000" in err.value and not handle.value
    assert_tape(tape[0:2].token_sorted().to_strs(), [b"a b", normal_form(fits, False)])
    view = tape[0:1].view()
    assert N.STATUS_NAMES[N.lib.swh_tape_token_sort(scope.handle, C.byref(view), 2, C.byref(handle), C.byref(err))] == "invalid_argument"
    with pytest.raises(sw.StringWarsError) as info:
        lev.token_sort_ratio([b"a", over], [b"a", b"b"], scope)
    assert info.value.status == "unsupported_length" and "string 1" in str(info.value)

    # token_set: the shorter NORMAL FORM over SWH_LCS_MAX_SHORTER symbols is refused, with nothing written
    a, b = [b"b a", b"a" * 3000, b"c"], [b"a b", b"b" * 2500, b"c"]
    outs = [np.full(3, 77, np.uint32) for _ in range(4)]
    with pytest.raises(sw.StringWarsError) as info:
        lev.token_set_counts(a, b, scope, out=outs)
    assert info.value.status == "unsupported_length" and "pair 1" in str(info.value) and "3000 x 2500" in str(info.value)
    assert all((o == 77).all() for o in outs)
    with pytest.raises(sw.StringWarsError) as info:
        lev8.token_set_counts(["b a", "é" * 2047 + " a", "c"], ["a b", "é" * 2047 + " b", "c"], scope, out=outs)
    assert info.value.status == "unsupported_length" and "pair 1" in str(info.value) and "2049 x 2049" in str(info.value)
    assert all((o == 77).all() for o in outs)
    # ... while a long normal form beside a short one is scored, and so are 2048 symbols exactly (repeated tokens do not count)
    a = [b"a" * 4000, b"ab " * 1365, b"q" * 2048 + b" " + b"q" * 2047, "é".encode() * 2048]
    b = [b"a" * 100 + b" b", b"ab", b"q" * 2048, "é".encode() * 2047 + b" z"]
    check_scores(lev, scope, a[:3], b[:3], False)   # (the last pair is 2048 x 2049 code points, and 4096 x 4096 bytes)
    check_scores(lev8, scope, [x.decode() for x in a], [x.decode() for x in b], True)
    # the conventions of the pairwise calls
    with pytest.raises(ValueError):
        lev.token_set_counts([b"a"], [b"a", b"b"], scope)
    with pytest.raises(sw.StringWarsError) as info:
        lev.token_set_counts([b"a"], [b"a"], scope, out=(None, None, None, None))
    assert info.value.status == "invalid_argument"
    with pytest.raises(sw.StringWarsError) as info:
        sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope).token_set_counts([b"a"], [b"a"], scope)
    assert info.value.status == "not_implemented"
    with pytest.raises(sw.StringWarsError) as info:
        lev8.token_set_counts([b"a \xff"], [b"a"], scope)
    assert info.value.status == "invalid_utf8"
    assert all(len(o) == 0 for o in lev.token_set_counts([], [], scope))


@gpu
def test_tape_forms(sw, scope, lev, lev8):
    rng = np.random.default_rng(23)
    words = ["new", "york", "mets", "vs", "atlanta", "braves", "a", "ab", "été", "中文", "of", "the"]
    names = [" ".join(words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(0, 9)))) for _ in range(40)]
    names[5], names[6], names[7] = "", " \t\n ", "\u3000\u00a0"
    for utf8, engine in ((False, lev), (True, lev8)):
        items = as_items(names, utf8)
        whole = sw.Strs(items)
        for dtype in (np.uint32, np.uint64):   # both offset widths; the derived tape keeps the source's
            check_derived(sw, scope, items, utf8, source=sw.PreparedTape(scope, whole.with_offsets(dtype), utf8=utf8))
        # a window of a larger buffer (offsets[0] != 0), and a sub-view of it that does not begin at its first string
        window = whole.subview(4, 37)
        assert int(window.offsets[0]) != 0
        for source in (window, window.to_device(scope), window.with_offsets(np.uint32).to_device(scope)):
            tape = sw.PreparedTape(scope, source, utf8=utf8)
            check_derived(sw, scope, items[4:37], utf8, source=tape)
            check_derived(sw, scope, items[9:30], utf8, source=tape[5:26])
            empty = tape[7:7].token_sorted(unique=True)
            assert len(empty) == 0 and empty.info["count"] == 0 and empty.to_strs().offsets.tolist() == [0] and len(empty.to_strs().data) == 0
            # to_strs reads any prepared tape, also one that was not derived
            assert_tape(tape[5:26].to_strs(), items[9:30])
        # the derived tape owns its memory: the source is freed before it is used
        source = sw.PreparedTape(scope, whole, utf8=utf8)
        sorted_a, unique_a = source.token_sorted(), source.token_sorted(unique=True)
        source.free()
        other = list(reversed(items))
        sorted_b = sw.PreparedTape(scope, sw.Strs([normal_form(x, False) for x in other]), utf8=utf8)
        sort_ratio, counts, set_ratio = reference(items, other, utf8)
        assert same_bits(engine.ratio(sorted_a, sorted_b, scope), sort_ratio)
        assert_tape(unique_a.to_strs(), [normal_form(x, True) for x in items])
        # strided, missing and device outputs of the split; raw, prepared and already unique sides
        prepared_b = sw.PreparedTape(scope, sw.Strs(other), utf8=utf8)
        matrix = np.full((len(items), 4), 77, dtype=np.uint32)
        engine.token_set_counts(items, other, scope, out=[matrix[:, k] for k in range(4)])
        assert np.array_equal(matrix.astype(np.int64), counts)
        wide = np.full((len(items), 6), 77, dtype=np.uint32)
        engine.token_set_counts(unique_a, prepared_b, scope, out=(None, wide[:, 1], None, wide[:, 3]))
        assert np.array_equal(wide[:, [1, 3]].astype(np.int64), counts[:, [1, 3]]) and (wide[:, [0, 2, 4, 5]] == 77).all()
        sect, ba = engine.token_set_counts(unique_a[3:20], prepared_b[3:20], scope, out=(True, None, True, None))[::2]
        assert np.array_equal(sect, counts[3:20, 0]) and np.array_equal(ba, counts[3:20, 2])
        import torch
        device = [torch.full((len(items),), 77, dtype=torch.int32, device="cuda") for _ in range(4)]
        engine.token_set_counts(unique_a, prepared_b, scope, out=device)
        assert np.array_equal(np.stack([d.cpu().numpy() for d in device], axis=1).astype(np.int64), counts)
        assert same_bits(engine.token_set_ratio(unique_a, prepared_b, scope), set_ratio)


def shuffled_names(rng, count, utf8):
    words = ["new", "york", "mets", "vs", "atlanta", "braves", "los", "angeles", "angels", "of", "anaheim", "at", "seattle", "mariners", "st", "louis",
             "cardinals", "étoile", "münchen", "東京", "fc", "united", "city", "real"]
    names = []
    for _ in range(count):
        picked = [words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(1, 7)))]
        names.append((" " if rng.integers(0, 4) else "  ").join(picked))
    return as_items(names, utf8)


@gpu
def test_composition_with_the_other_calls(sw, scope, lev, lev8):
    """A derived tape is a prepared tape: the dense, the search and the partial calls on derived tapes give what they give on tapes
    prepared from the strings Python normalised."""
    rng = np.random.default_rng(29)
    for utf8, engine in ((False, lev), (True, lev8)):
        queries, candidates = shuffled_names(rng, 200, utf8), shuffled_names(rng, 300, utf8)
        pq, pc = sw.PreparedTape(scope, sw.Strs(queries), utf8=utf8), sw.PreparedTape(scope, sw.Strs(candidates), utf8=utf8)
        dq, dc = pq.token_sorted(), pc.token_sorted()
        rq = sw.PreparedTape(scope, sw.Strs([normal_form(x, False) for x in queries]), utf8=utf8)
        rc = sw.PreparedTape(scope, sw.Strs([normal_form(x, False) for x in candidates]), utf8=utf8)
        want = engine.ratio_cross(rq, rc, scope)
        assert same_bits(engine.ratio_cross(dq, dc, scope), want) and same_bits(engine.token_sort_ratio_cross(queries, candidates, scope), want)
        assert same_bits(engine.token_sort_ratio_cross(pq, None, scope), engine.ratio_cross(rq, None, scope))
        got, ref = engine.extract(dq, dc, scope, scorer="ratio", k=5), engine.extract(rq, rc, scope, scorer="ratio", k=5)
        assert np.array_equal(got[0], ref[0]) and same_bits(got[1], ref[1])
        got = engine.extract_within(dq, dc, scope, scorer="ratio", cutoff=60.0)
        ref = engine.extract_within(rq, rc, scope, scorer="ratio", cutoff=60.0)
        assert np.array_equal(got.offsets, ref.offsets) and np.array_equal(got.indices, ref.indices) and len(ref.indices) > 0
        assert same_bits(getattr(got, got._values), getattr(ref, ref._values))
        assert same_bits(engine.partial_ratio(dq, dc[:200], scope), engine.partial_ratio(rq, rc[:200], scope))
        uq, uc = pq.token_sorted(unique=True), pc[:200].token_sorted(unique=True)
        on_raw = engine.token_set_counts(queries, candidates[:200], scope)
        for sides in ((uq, uc), (pq, pc[:200]), (uq, pc[:200])):
            assert all(np.array_equal(g, w) for g, w in zip(engine.token_set_counts(*sides, scope), on_raw))


def mutated_pairs(rng, count, utf8):
    vocabulary = ["a", "b", "ab", "ba", "abc", "new", "york", "jersey", "x", "é", "été", "中", "nu", "ny"]
    spaces = [" ", " ", "  ", "\t", "\n ", "\u00a0", "\u2003"]
    a, b = [], []
    for _ in range(count):
        tokens = [vocabulary[int(k)] for k in rng.integers(0, len(vocabulary), int(rng.integers(1, 13)))]
        other = list(tokens)
        for _ in range(int(rng.integers(0, 4))):
            kind, at = int(rng.integers(0, 4)), int(rng.integers(0, len(other)))
            if kind == 0 and len(other) > 1:
                del other[at]
            elif kind == 1:
                other.insert(at, vocabulary[int(rng.integers(0, len(vocabulary)))])
            elif kind == 2:
                other[at] = other[at] + "z"
            else:
                other = [other[int(k)] for k in rng.permutation(len(other))]
        a.append("".join(t + spaces[int(rng.integers(0, len(spaces)))] for t in tokens))
        b.append(spaces[int(rng.integers(0, len(spaces)))].join(other))
    return as_items(a, utf8), as_items(b, utf8)


@gpu
def test_random_round(sw, scope, lev, lev8):
    rng = np.random.default_rng(31)
    for utf8, engine in ((False, lev), (True, lev8)):
        a, b = mutated_pairs(rng, 2000, utf8)
        counts = check_scores(engine, scope, a, b, utf8)
        assert (counts[:, 0] > 0).sum() > 500 and (counts[:, 3] > 0).sum() > 200 and ((counts[:, 1] == 0) | (counts[:, 2] == 0)).sum() > 50


@gpu
def test_cpp_wrappers(tmp_path):
    """PreparedTape::token_sorted and ::read, LevenshteinDistances::token_set on raw and prepared tapes, token_set_score."""
    binary = build_check_tokens(tmp_path)
    rng = np.random.default_rng(37)
    for utf8 in (False, True):
        a, b = mutated_pairs(rng, 60, utf8)
        a, b = as_items([r[0] for r in ROWS], utf8) + a, as_items([r[1] for r in ROWS], utf8) + b
        write_case(tmp_path / "case", utf8, a, b)
        done = subprocess.run([str(binary), str(tmp_path / "case"), str(tmp_path / "result")], capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stderr
        blob, count, at = open(tmp_path / "result", "rb").read(), len(a), 0
        for items, unique in ((a, False), (b, False), (a, True)):
            want = raw([normal_form(x, unique) for x in items])
            offsets = np.frombuffer(blob[at:at + 8 * (count + 1)], dtype="<u8")
            at += 8 * (count + 1)
            assert offsets.tolist() == np.cumsum([0] + [len(x) for x in want]).tolist()
            assert blob[at:at + int(offsets[-1])] == b"".join(want)
            at += int(offsets[-1])
        sort_ratio, counts, set_ratio = reference(a, b, utf8)
        indel, lcs = (np.frombuffer(blob[at + k * 4 * count:at + (k + 1) * 4 * count], dtype="<u4").astype(np.int64) for k in range(2))
        at += 8 * count
        twice = 2.0 * lcs.astype(np.float64)
        total = indel.astype(np.float64) + twice
        assert same_bits(np.where(total > 0, 100.0 * twice / np.where(total > 0, total, 1.0), 100.0), sort_ratio)
        for _ in range(2):
            got = np.stack([np.frombuffer(blob[at + k * 4 * count:at + (k + 1) * 4 * count], dtype="<u4") for k in range(4)], axis=1)
            assert np.array_equal(got.astype(np.int64), counts)
            at += 16 * count
        assert same_bits(np.frombuffer(blob[at:at + 8 * count], dtype="<f8"), set_ratio)
        assert at + 8 * count == len(blob)
