"""Jaro and Jaro-Winkler counts and similarities (swh_levenshtein_jaro_*): rapidfuzz's distance.Jaro / distance.JaroWinkler.

Two references, both here and in pure Python: R1 is the definition's loop (a's symbols in order, the first free equal symbol of b
within the search range), R2 an independent formulation on Python's big integers (a match mask per symbol of b, the lowest set bit
of mask & window & ~flags), which is what the long strings use. The header's worked examples pin R1, R1 pins R2 on all pairs of
short strings and on random ones, all on the CPU; only then are they held against the GPU: the counts exactly, the similarities with
== against the header's expressions evaluated in Python on the reference's counts."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# a, b, M, t, jaro, jaro_winkler at p = 0.1: the worked examples of include/stringwars_amd.h
EXAMPLES = [("MARTHA", "MARHTA", 6, 1, 0.9444444444444445, 0.9611111111111111),
            ("DWAYNE", "DUANE", 4, 0, 0.8222222222222223, 0.8400000000000001),
            ("DIXON", "DICKSONX", 4, 0, 0.7666666666666666, 0.8133333333333332),
            ("CRATE", "TRACE", 3, 0, 0.7333333333333334, 0.7333333333333334),
            ("JELLYFISH", "SMELLYFISH", 8, 0, 0.8962962962962964, 0.8962962962962964),
            ("ab", "ba", 0, 0, 0.0, 0.0), ("a", "a", 1, 0, 1.0, 1.0), ("a", "b", 0, 0, 0.0, 0.0), ("", "", 0, 0, 1.0, 1.0)]
JARO_SYMBOLS = ("swh_levenshtein_jaro_pairs_u64tape", "swh_levenshtein_utf8_jaro_pairs_u64tape", "swh_levenshtein_jaro_pairs_prepared",
                "swh_levenshtein_jaro_cross_u64tape", "swh_levenshtein_utf8_jaro_cross_u64tape", "swh_levenshtein_jaro_cross_prepared")
METHODS = ("jaro_counts", "jaro_counts_cross", "jaro", "jaro_winkler", "jaro_cross", "jaro_winkler_cross")


# ---- the references -----------------------------------------------------------------------------------------------------------------
def symbols(s, utf8=False):
    if isinstance(s, str):
        return [ord(c) for c in s] if utf8 else list(s.encode())
    return list(bytes(s))


def common_prefix(a, b):
    size = 0
    while size < min(len(a), len(b), 4) and a[size] == b[size]:
        size += 1
    return size


def r1(a, b):
    """(M, t, prefix) by the definition's loop: a drives, b is flagged."""
    m, n = len(a), len(b)
    R = max(0, max(m, n) // 2 - 1)
    flagged, from_a = [False] * n, []
    for i in range(m):
        for j in range(max(0, i - R), min(n - 1, i + R) + 1):
            if b[j] == a[i] and not flagged[j]:
                flagged[j] = True
                from_a.append(a[i])
                break
    from_b = [b[j] for j in range(n) if flagged[j]]
    h = sum(x != y for x, y in zip(from_a, from_b))
    return len(from_a), h // 2, common_prefix(a, b)


def r2(a, b):
    """(M, t, prefix) on big integers: w = pm[c] & window & ~flags; flags |= w & -w; then the two matched sequences are compared."""
    m, n = len(a), len(b)
    R = max(0, max(m, n) // 2 - 1)
    pm = {}
    for j, c in enumerate(b):
        pm[c] = pm.get(c, 0) | (1 << j)
    everything = (1 << n) - 1
    flags, from_a = 0, []
    for i, c in enumerate(a):
        low = i - R
        window = (everything & ((1 << (i + R + 1)) - 1)) >> max(low, 0) << max(low, 0)
        w = pm.get(c, 0) & window & ~flags
        if w:
            flags |= w & -w
            from_a.append(c)
    from_b = [b[j] for j in range(n) if (flags >> j) & 1]
    assert len(from_a) == len(from_b)
    h = sum(x != y for x, y in zip(from_a, from_b))
    return len(from_a), h // 2, common_prefix(a, b)


def jaro_of(M, t, m, n):
    if m == 0 and n == 0:
        return 1.0
    if M == 0:
        return 0.0
    return (M / m + M / n + (M - t) / M) / 3.0


def winkler_of(jaro, prefix, p=0.1):
    return jaro + prefix * p * (1.0 - jaro) if jaro > 0.7 else jaro


def reference(a, b, utf8=False, ref=r2) -> np.ndarray:
    """The (count, 3) array of M, t, prefix of the pairs (a[k], b[k])."""
    return np.array([ref(symbols(x, utf8), symbols(y, utf8)) for x, y in zip(a, b)], dtype=np.int64).reshape(len(a), 3)


def similarities(a, b, counts, utf8=False, p=0.1):
    """jaro and jaro_winkler of the pairs as float64 arrays, by the header's expressions on `counts`."""
    jaro = [jaro_of(int(c[0]), int(c[1]), len(symbols(x, utf8)), len(symbols(y, utf8))) for x, y, c in zip(a, b, counts)]
    return np.array(jaro, dtype=np.float64), np.array([winkler_of(j, int(c[2]), p) for j, c in zip(jaro, counts)], dtype=np.float64)


def rand_bytes(rng, n, alphabet, base=97):
    return bytes((rng.integers(0, alphabet, size=int(n)) + base).astype(np.uint8))


def mutated(rng, s, edits, draw):
    """`edits` random edits of s: substitutions, insertions and deletions."""
    s = list(s)
    for _ in range(edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(0, max(len(s), 1)))
        if op == 0 and s:
            s[at] = draw()
        elif op == 1:
            s.insert(at, draw())
        elif op == 2 and s:
            del s[at]
    return s


def all_strings(alphabet, upto):
    return ["".join(x) for n in range(upto + 1) for x in itertools.product(alphabet, repeat=n)]


def expanded(queries, candidates):
    return [q for q in queries for _ in candidates], [c for _ in queries for c in candidates]


def raw_pairs(sw, engine, scope, a, b, matches, transpositions, prefix, stride=0, utf8=False):
    """The C ABI itself on raw u64 tapes; the outputs are pointers (host or device) or None. Returns (status name, message)."""
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True)
    fn = N.lib.swh_levenshtein_utf8_jaro_pairs_u64tape if utf8 else N.lib.swh_levenshtein_jaro_pairs_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb), C.c_void_p(matches), C.c_void_p(transpositions), C.c_void_p(prefix),
                stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def raw_cross(sw, engine, scope, a, b, matches, transpositions, prefix, stride=0, utf8=False):
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True) if b is not None else (None, None, None)
    fn = N.lib.swh_levenshtein_utf8_jaro_cross_u64tape if utf8 else N.lib.swh_levenshtein_jaro_cross_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb) if tb is not None else None, C.c_void_p(matches),
                C.c_void_p(transpositions), C.c_void_p(prefix), stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def assert_same(got, want, describe=lambda k: int(k)):
    got, want = np.asarray(got).astype(np.int64).ravel(), np.asarray(want).astype(np.int64).ravel()
    assert got.shape == want.shape
    wrong = np.nonzero(got != want)[0]
    assert not len(wrong), [(describe(k), int(got[k]), int(want[k])) for k in wrong[:5]]


def assert_counts(got, want, describe=lambda k: int(k)):
    """`got`: the three arrays of a call; `want`: the reference's (count, 3) array."""
    assert len(got) == 3
    for column, name in enumerate(("matches", "transpositions", "prefix")):
        assert_same(got[column], want[:, column], lambda k: (name, describe(k)))


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in JARO_SYMBOLS:
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "jaro" in sw.capabilities().split(",")
    for name in METHODS:
        assert callable(getattr(sw.LevenshteinDistances, name)), name
        assert getattr(sw.LevenshteinDistancesUTF8, name) is getattr(sw.LevenshteinDistances, name), name
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_JARO_MAX_LENGTH 2048u", header) and N.JARO_MAX_LENGTH == 2048 == sw.JARO_MAX_LENGTH
    test_library = C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    assert all(hasattr(test_library, name) for name in JARO_SYMBOLS)


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    ta, _, keep_a = sw.engines._c_tape(sw.Strs([b"ab"]), want64=True)
    tb, _, keep_b = sw.engines._c_tape(sw.Strs([b"ba"]), want64=True)
    out32, out64 = np.full(3, 77, np.uint32), np.full(3, 77, np.uint64)
    view = N.PreparedView(None, 0, 1)
    for name in JARO_SYMBOLS:
        cross, prepared = "_cross_" in name, name.endswith("_prepared")
        sides = (C.byref(view), C.byref(view)) if prepared else (C.byref(ta), C.byref(tb))
        out = out64 if cross else out32
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, *sides, C.c_void_p(out.ctypes.data), C.c_void_p(out[1:].ctypes.data),
                                      C.c_void_p(out[2:].ctypes.data), 0, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    assert (out32 == 77).all() and (out64 == 77).all()


def test_definition_reproduces_the_worked_examples():
    for a, b, M, t, jaro, winkler in EXAMPLES:
        x, y = symbols(a), symbols(b)
        got = r1(x, y)
        assert got[:2] == (M, t), (a, b, got)
        assert jaro_of(got[0], got[1], len(x), len(y)) == jaro, (a, b)
        assert winkler_of(jaro_of(got[0], got[1], len(x), len(y)), got[2]) == winkler, (a, b)
    assert r1(symbols("JELLYFISH"), symbols("SMELLYFISH"))[2] == 0 and r1(symbols("MARTHA"), symbols("MARHTA"))[2] == 3
    # h can be odd: a's matched symbols are b c a, b's flagged ones c a b -- three differing ranks, halved and floored
    assert r1(symbols("bbcaba"), symbols("cab")) == (3, 1, 0)
    # code points, not bytes: é and è share their first byte, and with m = n = 2 the range is 0
    assert r1(symbols("é", True), symbols("è", True))[0] == 0 and r1(symbols("é"), symbols("è"))[0] == 1
    assert r2(symbols("é", True), symbols("è", True))[0] == 0 and r2(symbols("é"), symbols("è"))[0] == 1


def test_the_two_references_agree():
    for alphabet, upto, count in (("ab", 6, 127), ("abc", 4, 121)):
        strs = [symbols(s) for s in all_strings(alphabet, upto)]
        assert len(strs) == count
        for x in strs:
            for y in strs:
                assert r1(x, y) == r2(x, y), (x, y)
    rng = np.random.default_rng(70)
    for i in range(3000):
        alphabet = int(rng.integers(2, 27))
        x = list(rand_bytes(rng, rng.integers(0, 151), alphabet))
        y = mutated(rng, x, int(rng.integers(0, 12)), lambda: int(rng.integers(97, 97 + alphabet)))[:150] if i % 2 else \
            list(rand_bytes(rng, rng.integers(0, 151), alphabet))
        assert r1(x, y) == r2(x, y), (x, y)


def test_no_short_pair_depends_on_which_side_drives():
    """An observation, not a theorem: on the two exhaustive sets swapping the sides changes neither M nor t. The self-product test
    relies on it when it asks for a symmetric matrix."""
    for alphabet, upto in (("ab", 6), ("abc", 4)):
        strs = [symbols(s) for s in all_strings(alphabet, upto)]
        for x in strs:
            for y in strs:
                assert r1(x, y) == r1(y, x), (x, y)


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


@pytest.mark.gpu
def test_examples_and_exhaustive(sw, scope, lev, lev8):
    a, b = sw.Strs([e[0] for e in EXAMPLES]), sw.Strs([e[1] for e in EXAMPLES])
    for engine in (lev, lev8):
        got = engine.jaro_counts(a, b, scope)
        assert all(x.dtype == np.uint32 for x in got)
        assert got[0].tolist() == [e[2] for e in EXAMPLES] and got[1].tolist() == [e[3] for e in EXAMPLES]
        assert got[2].tolist() == [common_prefix(e[0], e[1]) for e in EXAMPLES]
        got = engine.jaro(a, b, scope)
        assert got.dtype == np.float64 and got.tolist() == [e[4] for e in EXAMPLES]
        got = engine.jaro_winkler(a, b, scope)
        assert got.dtype == np.float64 and got.tolist() == [e[5] for e in EXAMPLES]
        assert engine.jaro([b"MARTHA"], [b"MARHTA"], scope)[0] == 0.9444444444444445    # lists are accepted
        assert engine.jaro_winkler([b"MARTHA"], [b"MARHTA"], scope, prefix_weight=0.25)[0] == winkler_of(0.9444444444444445, 3, 0.25)
    for alphabet, engine, utf8 in (("ab", lev, False), ("aé", lev8, True)):
        strs = all_strings(alphabet, 6)
        assert len(strs) == 127
        x, y = expanded(strs, strs)
        want = reference(x, y, utf8=utf8, ref=r1)
        describe = lambda k: (x[k], y[k])
        got = engine.jaro_counts_cross(sw.Strs(strs), sw.Strs(strs), scope)
        assert all(g.dtype == np.uint64 and g.shape == (127, 127) for g in got)
        assert_counts(got, want, describe)
        jaro, winkler = similarities(x, y, want, utf8=utf8)
        assert (engine.jaro_cross(sw.Strs(strs), sw.Strs(strs), scope).ravel() == jaro).all()
        assert (engine.jaro_winkler_cross(sw.Strs(strs), sw.Strs(strs), scope).ravel() == winkler).all()
        # the self-product: the same matrices, symmetric (on these strings: see the CPU test), the diagonal M = len, t = 0, l = min(len, 4)
        own = engine.jaro_counts_cross(sw.Strs(strs), None, scope)
        lengths = np.array([len(s) for s in strs])
        for g, o in zip(got, own):
            assert (g == o).all() and (o == o.T).all()
        assert (np.diagonal(own[0]) == lengths).all() and (np.diagonal(own[1]) == 0).all()
        assert (np.diagonal(own[2]) == np.minimum(lengths, 4)).all()
        assert (engine.jaro_winkler_cross(sw.Strs(strs), None, scope).ravel() == winkler).all()


BLOCK_N = (1, 31, 32, 33, 63, 64, 65, 96, 97, 2047, 2048)


def block_edge_cases():
    """(n, kind, a, b, known (M, t) or None): b holds n symbols. The fillers y (of a) and z (of b) match nothing."""
    rng = np.random.default_rng(71)
    cases = []
    for n in BLOCK_N:
        for m in sorted({n, n + 1, n // 2} - {0}):
            if m <= 2048:   # every column finds its match in a different block: the found bit must stop every block above
                cases.append((n, "one symbol", b"a" * m, b"a" * n, (min(m, n), 0)))
        R = max(0, n // 2 - 1)   # of the window cases: m = n
        if R >= 1:
            for at, M in ((R, 1), (R + 1, 0)):
                far = bytearray(b"z" * n)
                far[at] = ord("x")
                cases.append((n, "window: x at b[%d]" % at, b"x" + b"y" * (n - 1), bytes(far), (M, 0)))
                far = bytearray(b"y" * n)
                far[at] = ord("x")
                cases.append((n, "window: x at a[%d]" % at, bytes(far), b"x" + b"z" * (n - 1), (M, 0)))
        if n >= 33:
            a = bytearray(b"c" * n)
            a[31], a[32] = ord("x"), ord("y")
            b = bytearray(a)
            b[31], b[32] = a[32], a[31]
            cases.append((n, "swap across rows 31 / 32", bytes(a), bytes(b), (n, 1)))
            a = bytearray(b"c" * n)
            a[30], a[31], a[32] = ord("x"), ord("y"), ord("z")
            b = bytearray(a)
            b[30], b[31], b[32] = a[31], a[32], a[30]   # h = 3
            cases.append((n, "three-cycle across rows 30 .. 32", bytes(a), bytes(b), (n, 1)))
        for alphabet in (2, 26):
            for m in (n, n + 1, 2 * n + 3):
                cases.append((n, "random %d" % alphabet, rand_bytes(rng, min(m, 2048), alphabet), rand_bytes(rng, n, alphabet), None))
    return cases


@pytest.mark.gpu
def test_block_edges(sw, scope, lev):
    cases = block_edge_cases()
    a, b = [c[2] for c in cases], [c[3] for c in cases]
    assert {len(y) for y in b} == set(BLOCK_N)
    want, swapped = reference(a, b), reference(b, a)
    for k, c in enumerate(cases):   # what the constructed cases are known to give, in either order
        if c[4] is not None:
            assert tuple(want[k, :2]) == c[4] == tuple(swapped[k, :2]), (c[0], c[1])
    describe = lambda k: (cases[k][0], cases[k][1], len(a[k]))
    sa, sb = sw.Strs(a), sw.Strs(b)
    assert_counts(lev.jaro_counts(sa, sb, scope), want, describe)
    assert_counts(lev.jaro_counts(sb, sa, scope), swapped, describe)
    jaro, winkler = similarities(a, b, want)
    assert (lev.jaro(sa, sb, scope) == jaro).all() and (lev.jaro_winkler(sa, sb, scope) == winkler).all()


@pytest.mark.gpu
def test_mixed_items(sw, scope, lev):
    """One batch whose block counts run 1..64 in shuffled order, with empty strings on either or both sides: pairs of different G
    share a wave, lanes idle past a shorter b, and the last run of 64 pairs is partial."""
    rng = np.random.default_rng(72)
    count = 64 * 3 + 5
    blocks = np.concatenate([rng.permutation(64) + 1 for _ in range(4)])[:count]
    a, b = [], []
    for i in range(count):
        n = int(blocks[i]) * 32 - int(rng.integers(0, 32))
        y = rand_bytes(rng, n, 4)
        kind = i % 7 if i >= 64 else 3   # (the first run of 64 pairs holds every block count)
        if kind == 0:
            x, y = rand_bytes(rng, rng.integers(0, 50), 4), b""
        elif kind == 1:
            x = b""
        elif kind == 2:
            x = bytes(mutated(rng, y, int(rng.integers(1, 9)), lambda: int(rng.integers(97, 101))))[:2048]
        else:
            x = rand_bytes(rng, min(2048, max(0, n - 100 + int(rng.integers(0, 200)))), 4)
        a.append(x); b.append(y)
    a[70], b[70] = b"", b""
    assert {max(1, (len(y) + 31) // 32) for y in b[:64]} == set(range(1, 65))
    want = reference(a, b)
    describe = lambda k: (int(k), len(a[k]), len(b[k]))
    assert_counts(lev.jaro_counts(sw.Strs(a), sw.Strs(b), scope), want, describe)
    order = rng.permutation(count)   # a pair's result does not depend on its neighbours
    again = lev.jaro_counts(sw.Strs([a[k] for k in order]), sw.Strs([b[k] for k in order]), scope)
    assert_counts(again, want[order])


@pytest.mark.gpu
def test_forms_and_scopes(sw, scope, lev):
    import torch
    from stringwars_amd import _native as N
    rng = np.random.default_rng(73)
    a = [rand_bytes(rng, rng.integers(0, 300), 4) for _ in range(700)]
    b = [bytes(mutated(rng, x, int(rng.integers(0, 9)), lambda: int(rng.integers(97, 101)))) if k % 2 else rand_bytes(rng, rng.integers(0, 300), 4)
         for k, x in enumerate(a)]
    sa, sb = sw.Strs(a), sw.Strs(b)
    want = reference(a, b)
    assert (want[:, 1] > 0).any() and (want[:, 2] == 4).any() and (want[:, 2] == 0).any()
    assert_counts(lev.jaro_counts(sa, sb, scope), want)
    fresh = lambda: [np.full(700, 77, np.uint32) for _ in range(3)]
    fresh_d = lambda: [torch.full((700,), 77, dtype=torch.int32, device="cuda") for _ in range(3)]
    # each output alone and all three, on the host and on the device: what is not wanted is not written
    for wanted in ((0,), (1,), (2,), (0, 1, 2)):
        host, dev = fresh(), fresh_d()
        status, message = raw_pairs(sw, lev, scope, sa, sb, *[host[k].ctypes.data if k in wanted else None for k in range(3)])
        assert status == "success", message
        status, message = raw_pairs(sw, lev, scope, sa, sb, *[dev[k].data_ptr() if k in wanted else None for k in range(3)])
        assert status == "success", message
        for k in range(3):
            if k in wanted:
                assert_same(host[k], want[:, k]); assert_same(dev[k].cpu().numpy(), want[:, k])
            else:
                assert (host[k] == 77).all() and (dev[k].cpu().numpy() == 77).all()
        partial = lev.jaro_counts(sa, sb, scope, out=tuple(True if k in wanted else None for k in range(3)))
        assert all((partial[k] is not None) == (k in wanted) for k in range(3))
    # host and device pointers mixed
    host, dev = fresh(), fresh_d()
    status, message = raw_pairs(sw, lev, scope, sa, sb, host[0].ctypes.data, dev[1].data_ptr(), host[2].ctypes.data)
    assert status == "success", message
    assert_same(host[0], want[:, 0]); assert_same(dev[1].cpu().numpy(), want[:, 1]); assert_same(host[2], want[:, 2])
    assert (host[1] == 77).all() and (dev[0].cpu().numpy() == 77).all() and (dev[2].cpu().numpy() == 77).all()
    # stride 12, host and device: the gaps stay as they were
    wide = np.full((700, 3), 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, sa, sb, wide.ctypes.data, None, wide.ctypes.data + 8, stride=12)
    assert status == "success", message
    assert_same(wide[:, 0], want[:, 0]); assert_same(wide[:, 2], want[:, 2]); assert (wide[:, 1] == 77).all()
    wide_d = torch.full((700, 3), 77, dtype=torch.int32, device="cuda")
    status, message = raw_pairs(sw, lev, scope, sa, sb, None, wide_d.data_ptr() + 4, wide_d.data_ptr() + 8, stride=12)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert_same(back[:, 1], want[:, 1]); assert_same(back[:, 2], want[:, 2]); assert (back[:, 0] == 77).all()
    wide = np.full((700, 3), 77, np.uint32)
    lev.jaro_counts(sa, sb, scope, out=(wide[:, 1], None, wide[:, 2]))
    assert_same(wide[:, 1], want[:, 0]); assert_same(wide[:, 2], want[:, 2]); assert (wide[:, 0] == 77).all()
    # raw device tapes, raw u64 tapes; prepared tapes in all four offset-width mixes, whole and as sub-views
    jaro, winkler = similarities(a, b, want)
    assert_counts(lev.jaro_counts(sa.to_device(scope), sb.to_device(scope), scope), want)
    assert (lev.jaro_winkler(sa.to_device(scope), sb.to_device(scope), scope) == winkler).all()
    da, db = sa.with_offsets(np.uint64).to_device(scope), sb.with_offsets(np.uint64).to_device(scope)
    host = fresh()
    status, message = raw_pairs(sw, lev, scope, da, db, host[0].ctypes.data, host[1].ctypes.data, None)
    assert status == "success", message
    assert_same(host[0], want[:, 0]); assert_same(host[1], want[:, 1])
    tapes = {(w, name): sw.PreparedTape(scope, sw.Strs(items).with_offsets(w)) for w in (np.uint32, np.uint64)
             for name, items in (("a", a), ("b", b))}
    for wa, wb in itertools.product((np.uint32, np.uint64), repeat=2):
        pa, pb = tapes[(wa, "a")], tapes[(wb, "b")]
        assert_counts(lev.jaro_counts(pa, pb, scope), want)
        assert_counts(lev.jaro_counts(pa[37:333], pb[37:333], scope), want[37:333])
        on_device = torch.zeros(296, dtype=torch.int32, device="cuda")
        lev.jaro_counts(pa[37:333], pb[37:333], scope, out=(None, on_device, None))
        assert_same(on_device.cpu().numpy(), want[37:333, 1])
        assert (lev.jaro(pa[37:333], pb[37:333], scope) == jaro[37:333]).all()
    assert (lev.jaro_winkler(tapes[(np.uint32, "a")], tapes[(np.uint64, "b")], scope) == winkler).all()
    # tapes of two kinds: refused by the C ABI, nothing written
    as_utf8 = sw.PreparedTape(scope, sb, utf8=True)
    va, vb, err = tapes[(np.uint64, "a")].view(), as_utf8.view(), C.c_char_p()
    untouched = np.full(700, 77, np.uint32)
    status = N.lib.swh_levenshtein_jaro_pairs_prepared(lev._handle, scope.handle, C.byref(va), C.byref(vb), C.c_void_p(untouched.ctypes.data),
                                                       None, None, 0, C.byref(err))
    assert N.STATUS_NAMES[status] == "invalid_argument" and (untouched == 77).all()
    # a caller-stream scope -- synchronous, then asynchronous, then pipelined: the results are visible when the call returns
    other = sw.DeviceScope(gpu_device=0, stream=torch.cuda.current_stream().cuda_stream)
    engine = sw.LevenshteinDistances(capabilities=other)
    assert_counts(engine.jaro_counts(sa, sb, other), want)
    for mode in ("async", "pipelined"):
        if mode == "async":
            other.set_async(True)
        else:
            other.set_async(False)
            other.set_pipelined(True)
        engine.pairs(sa, sb, other)   # outstanding work the call joins
        assert_counts(engine.jaro_counts(sa, sb, other), want)
        other.synchronize()
    # profiling describes the whole call: the measuring kernel and the counting one; one more of the latter with outputs of both kinds
    scope.set_profiling(True)
    try:
        lev.jaro_counts(sa, sb, scope)
        timing = scope.last_timing()
        host, dev = fresh(), fresh_d()
        assert raw_pairs(sw, lev, scope, sa, sb, host[0].ctypes.data, dev[1].data_ptr(), None)[0] == "success"
        mixed_timing = scope.last_timing()
        lev.jaro_counts_cross(sa[:60], sb[:50], scope)
        cross_timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["cells"] == int((sa.lengths * sb.lengths).sum())
    assert timing["dominant_name"] == "jaro" and timing["kernels"] == 2 and mixed_timing["kernels"] == 3
    assert cross_timing["cells"] == int(sa.lengths[:60].sum()) * int(sb.lengths[:50].sum()) and cross_timing["dominant_name"] == "jaro"


def golden_strings(name, sides):
    z = np.load(os.path.join(GOLDEN, name))
    out = []
    for side in sides:
        data, offsets = z[side + "_data"], z[side + "_offsets"].astype(np.int64)
        out.append([bytes(data[offsets[i]:offsets[i + 1]]).decode("utf-8") for i in range(len(offsets) - 1)])
    return out


@pytest.mark.gpu
def test_utf8(sw, scope, lev, lev8):
    rng = np.random.default_rng(74)
    lines_a, lines_b = golden_strings("script_lines.npz", "ab")
    queries, candidates = golden_strings("uwords.npz", "qc")
    count = min(len(queries), len(candidates), 400)
    a, b = list(lines_a[:150]) + queries[:count], list(lines_b[:150]) + candidates[:count]
    assert all(len(s) <= 2048 for s in a + b)
    # a 1- to 4-byte code-point alphabet, with the first and last code point of every length
    mixed = [0x61, 0x62, 0xE9, 0x3B1, 0x4E2D, 0x6587, 0x1F600, 0x10FFFF, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000]
    renamed = {cp: 65 + k for k, cp in enumerate(mixed)}
    first = len(a)
    for i in range(300):
        x = [int(rng.choice(mixed)) for _ in range(int(rng.integers(0, 100)))]
        y = mutated(rng, x, int(rng.integers(0, 6)), lambda: int(rng.choice(mixed)))
        a.append("".join(map(chr, x))); b.append("".join(map(chr, y)))
    a.append("é"); b.append("è")   # no code point in common; one byte in common, and in range
    assert any(len(x.encode()) > len(x) for x in a[:first])
    want = reference(a, b, utf8=True)
    got = lev8.jaro_counts(sw.Strs(a), sw.Strs(b), scope)
    assert_counts(got, want)
    jaro, winkler = similarities(a, b, want, utf8=True)
    assert (lev8.jaro(sw.Strs(a), sw.Strs(b), scope) == jaro).all()
    assert got[0][-1] == 0 and lev.jaro_counts(sw.Strs(a[-1:]), sw.Strs(b[-1:]), scope)[0][0] == 1
    # the byte call on the strings with the code points renamed to bytes
    as_bytes = lambda strs: [bytes(renamed[ord(c)] for c in s) for s in strs]
    assert_counts(lev.jaro_counts(sw.Strs(as_bytes(a[first:-1])), sw.Strs(as_bytes(b[first:-1])), scope), want[first:-1])
    pa, pb = sw.PreparedTape(scope, sw.Strs(a), utf8=True), sw.PreparedTape(scope, sw.Strs(b), utf8=True)
    assert_counts(lev8.jaro_counts(pa, pb, scope), want)
    assert (lev8.jaro_winkler(pa, pb, scope) == winkler).all()   # the lengths are code points
    some = slice(first - 20, first + 20)
    matrices = lev8.jaro_counts_cross(sw.Strs(a[some]), sw.Strs(b[some]), scope)
    assert_counts([np.diagonal(g) for g in matrices], want[some])
    scope.set_profiling(True)
    try:
        lev8.jaro_counts(sw.Strs(a), sw.Strs(b), scope)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["dominant_name"] == "jaro_u32" and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    # invalid UTF-8 in either tape: the status, and the outputs untouched
    out, matrix = np.full(2, 77, np.uint32), np.full((2, 2), 77, np.uint64)
    for bad_a, bad_b in (([b"ok", b"\xff\xfe"], [b"ok", b"x"]), ([b"ok", b"x"], [b"ok", b"\xc3"])):
        status, _ = raw_pairs(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), out.ctypes.data, None, None, utf8=True)
        assert status == "invalid_utf8" and (out == 77).all()
        status, _ = raw_cross(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), None, matrix.ctypes.data, None, utf8=True)
        assert status == "invalid_utf8" and (matrix == 77).all()


def cross_batch():
    rng = np.random.default_rng(75)
    queries = [rand_bytes(rng, rng.integers(0, 90), 4) for _ in range(37)]
    candidates = [bytes(mutated(rng, queries[k % 37], int(rng.integers(0, 5)), lambda: int(rng.integers(97, 101)))) for k in range(53)]
    return queries, candidates


@pytest.mark.gpu
def test_cross(sw, scope, lev):
    import torch
    queries, candidates = cross_batch()
    sq, sc = sw.Strs(queries), sw.Strs(candidates)
    a, b = expanded(queries, candidates)
    want = reference(a, b)
    cube = want.T.reshape(3, 37, 53)
    got = lev.jaro_counts_cross(sq, sc, scope)
    assert all(g.dtype == np.uint64 and g.shape == (37, 53) for g in got)
    assert_counts(got, want)
    jaro, winkler = similarities(a, b, want)
    assert (lev.jaro_cross(sq, sc, scope).ravel() == jaro).all() and (lev.jaro_winkler_cross(sq, sc, scope).ravel() == winkler).all()
    # a row stride wider than the row, on the host and on the device, all matrices in one call: the columns past them stay
    wide = np.full((3, 37, 56), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sq, sc, wide[0].ctypes.data, wide[1].ctypes.data, wide[2].ctypes.data, stride=56 * 8)
    assert status == "success", message
    assert_same(wide[:, :, :53], cube); assert (wide[:, :, 53:] == 77).all()
    wide_d = torch.full((3, 37, 56), 77, dtype=torch.int64, device="cuda")
    status, message = raw_cross(sw, lev, scope, sq, sc, wide_d[0].data_ptr(), wide_d[1].data_ptr(), wide_d[2].data_ptr(), stride=56 * 8)
    assert status == "success", message
    assert (wide_d.cpu().numpy() == wide.astype(np.int64)).all()
    out = np.full((37, 56), 77, np.uint64)
    lev.jaro_counts_cross(sq, sc, scope, out=(None, out[:, :53], None))
    assert_same(out[:, :53], cube[1]); assert (out[:, 53:] == 77).all()
    # device and prepared tapes, whole and as sub-views
    assert_counts(lev.jaro_counts_cross(sq.to_device(scope), sc.to_device(scope), scope), want)
    pq, pc = sw.PreparedTape(scope, sq.with_offsets(np.uint32)), sw.PreparedTape(scope, sc.with_offsets(np.uint64))
    assert_counts(lev.jaro_counts_cross(pq, pc, scope), want)
    part = lev.jaro_counts_cross(pq[5:30], pc[3:], scope)
    for k in range(3):
        assert_same(part[k], cube[k, 5:30, 3:])
    assert (lev.jaro_cross(pq[5:30], pc[3:], scope) == jaro.reshape(37, 53)[5:30, 3:]).all()
    # b == NULL: the self-product
    own = np.full((3, 37, 37), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sq, None, own[0].ctypes.data, own[1].ctypes.data, own[2].ctypes.data)
    assert status == "success", message
    a, b = expanded(queries, queries)
    assert_same(own, reference(a, b).T)
    assert (np.diagonal(own[0]) == sq.lengths).all() and (np.diagonal(own[1]) == 0).all()
    assert (np.diagonal(own[2]) == np.minimum(sq.lengths, 4)).all()
    assert all((g == o).all() for g, o in zip(lev.jaro_counts_cross(pq, None, scope), own))
    assert lev.jaro_counts_cross(sw.Strs([]), sw.Strs([b"a"]), scope)[0].shape == (0, 1)
    assert lev.jaro_cross(sw.Strs([]), sw.Strs([b"a"]), scope).shape == (0, 1)


@pytest.mark.gpu
def test_cross_in_many_chunks(request, sw):
    """STRINGWARS_AMD_JARO_CHUNK_PAIRS (test library) shrinks the slices of whole rows to 424 pairs, so the 37 x 53 product runs as
    four slices of eight rows and a ragged fifth of five, with the same results on the host and on the device."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_JARO_CHUNK_PAIRS="424"), test_library=True):
        return
    import torch
    scope = sw.DeviceScope(gpu_device=0)
    lev = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = cross_batch()
    a, b = expanded(queries, candidates)
    want = reference(a, b)
    cube = want.T.reshape(3, 37, 53)
    scope.set_profiling(True)
    got = lev.jaro_counts_cross(sw.Strs(queries), sw.Strs(candidates), scope)
    timing = scope.last_timing()
    scope.set_profiling(False)
    assert_counts(got, want)
    assert timing["kernels"] == 1 + 2 * 5 and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    wide_d = torch.full((3, 37, 56), 77, dtype=torch.int64, device="cuda")
    status, message = raw_cross(sw, lev, scope, sw.Strs(queries), sw.Strs(candidates), wide_d[0].data_ptr(), wide_d[1].data_ptr(),
                                wide_d[2].data_ptr(), stride=56 * 8)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert_same(back[:, :, :53], cube); assert (back[:, :, 53:] == 77).all()
    host, on_device = np.full((37, 53), 77, np.uint64), torch.full((37, 53), 77, dtype=torch.int64, device="cuda")   # one of each kind
    status, message = raw_cross(sw, lev, scope, sw.Strs(queries), sw.Strs(candidates), host.ctypes.data, on_device.data_ptr(), None)
    assert status == "success", message
    assert_same(host, cube[0]); assert_same(on_device.cpu().numpy(), cube[1])
    # a refusal still comes before the first row is written
    long_q = [b"ab"] * 300 + [b"a" * 2049]
    long_c = [b"ab", b"b" * 2048, b"c" * 20]
    untouched = np.full((301, 3), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sw.Strs(long_q), sw.Strs(long_c), untouched.ctypes.data, None, None)
    assert status == "unsupported_length" and "pair (300, 0)" in message and "2049 x 2" in message and (untouched == 77).all(), message


@pytest.mark.gpu
def test_refusals(sw, scope, lev):
    rng = np.random.default_rng(76)
    outs = [np.full(3, 77, np.uint32) for _ in range(3)]
    pointers = [o.ctypes.data for o in outs]
    # 2049 symbols on the a side alone, on the b side alone: each is refused, naming the pair and both lengths, nothing written
    for a, b, lengths in (([b"abc", rand_bytes(rng, 2049, 4), b"x"], [b"acb", rand_bytes(rng, 5, 4), b"x"], "2049 x 5"),
                          ([b"abc", rand_bytes(rng, 5, 4), b"x"], [b"acb", rand_bytes(rng, 2049, 4), b"x"], "5 x 2049")):
        status, message = raw_pairs(sw, lev, scope, sw.Strs(a), sw.Strs(b), *pointers)
        assert status == "unsupported_length" and "pair 1" in message and lengths in message, message
        assert all((o == 77).all() for o in outs)
        with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
            lev.jaro(sw.Strs(a), sw.Strs(b), scope)
        assert "pair 1" in str(info.value)
        matrix = np.full((3, 3), 77, np.uint64)
        status, message = raw_cross(sw, lev, scope, sw.Strs(a), sw.Strs(b), matrix.ctypes.data, None, None)
        assert status == "unsupported_length" and (matrix == 77).all(), message
        assert ("pair (1, 0)" if len(a[1]) == 2049 else "pair (0, 1)") in message, message
    # 2048 x 2048 is accepted and correct
    a, b = [rand_bytes(rng, 2048, 4), b"abc"], [rand_bytes(rng, 2048, 4), b"acb"]
    assert_counts(lev.jaro_counts(sw.Strs(a), sw.Strs(b), scope), reference(a, b))
    # a general-cost engine
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    for call in (costly.jaro_counts, costly.jaro, costly.jaro_winkler, costly.jaro_counts_cross, costly.jaro_cross, costly.jaro_winkler_cross):
        with pytest.raises(sw.StringWarsError, match="not_implemented"):
            call(sw.Strs([b"ab"]), sw.Strs([b"ba"]), scope)
    # count mismatch, all outputs null, strides that are no multiple of the element
    assert raw_pairs(sw, lev, scope, sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), *pointers)[0] == "invalid_argument"
    with pytest.raises(ValueError):
        lev.jaro_counts(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope)
    assert raw_pairs(sw, lev, scope, sw.Strs(a), sw.Strs(b), None, None, None)[0] == "invalid_argument"
    assert raw_cross(sw, lev, scope, sw.Strs(a), sw.Strs(b), None, None, None)[0] == "invalid_argument"
    for stride in (2, 6):
        assert raw_pairs(sw, lev, scope, sw.Strs(a), sw.Strs(b), *pointers, stride=stride)[0] == "invalid_argument"
    matrix = np.full((2, 3), 77, np.uint64)
    assert raw_cross(sw, lev, scope, sw.Strs(a), sw.Strs(b), matrix.ctypes.data, None, None, stride=20)[0] == "invalid_argument"
    assert raw_cross(sw, lev, scope, sw.Strs(a), sw.Strs(b), matrix.ctypes.data, None, None, stride=8)[0] == "invalid_argument"
    assert all((o == 77).all() for o in outs) and (matrix == 77).all()
    # count == 0: success, nothing written
    assert all(len(x) == 0 for x in lev.jaro_counts(sw.Strs([]), sw.Strs([]), scope)) and len(lev.jaro_winkler(sw.Strs([]), sw.Strs([]), scope)) == 0
    status, _ = raw_pairs(sw, lev, scope, sw.Strs([]), sw.Strs([]), *pointers)
    assert status == "success" and all((o == 77).all() for o in outs)
    # the prefix weight lies in [0, 0.25]
    for call in (lev.jaro_winkler, lev.jaro_winkler_cross):
        with pytest.raises(ValueError):
            call(sw.Strs([b"ab"]), sw.Strs([b"ab"]), scope, prefix_weight=0.3)
        with pytest.raises(ValueError):
            call(sw.Strs([b"ab"]), sw.Strs([b"ab"]), scope, prefix_weight=-0.1)
    assert lev.jaro_winkler([b"abcd"], [b"abcx"], scope, prefix_weight=0.25)[0] == winkler_of(jaro_of(3, 0, 4, 4), 3, 0.25)


LENGTH_CLASSES = ((0, 16, 0.40), (17, 64, 0.30), (65, 300, 0.2925), (301, 2048, 0.0075))


@pytest.mark.gpu
def test_seeded_random_round(sw, scope, lev):
    """20 000 pairs over all length classes and alphabets 2 / 4 / 26 / 256, two thirds of them mutated copies, and a 150 x 150
    self-product."""
    rng = np.random.default_rng(2030)
    count = 20000
    kinds = rng.choice(len(LENGTH_CLASSES), size=count, p=[c[2] for c in LENGTH_CLASSES])
    alphabets = np.array([2, 4, 26, 256])[rng.integers(0, 4, size=count)]
    related, edits = rng.integers(0, 3, size=count), rng.integers(0, 12, size=count)
    a, b = [], []
    for i in range(count):
        low, high, _ = LENGTH_CLASSES[kinds[i]]
        alphabet, base = int(alphabets[i]), 0 if alphabets[i] == 256 else 97
        x = rand_bytes(rng, rng.integers(low, high + 1), alphabet, base)
        if related[i]:
            y = bytes(mutated(rng, x, int(edits[i]), lambda: base + int(rng.integers(0, alphabet))))[:2048]
        else:
            other = LENGTH_CLASSES[int(rng.integers(0, kinds[i] + 1))]
            y = rand_bytes(rng, rng.integers(other[0], other[1] + 1), alphabet, base)
        if i % 2:
            x, y = y, x
        a.append(x); b.append(y)
    assert (kinds == 3).sum() >= 100
    want = reference(a, b)
    jaro, winkler = similarities(a, b, want)
    queries = [rand_bytes(rng, rng.integers(0, 120), (2, 4, 26)[k % 3]) for k in range(150)]
    qa, qb = expanded(queries, queries)
    want_cross = reference(qa, qb)
    # every random number is drawn and the references are computed: the device comes now
    describe = lambda k: (int(k), len(a[k]), len(b[k]))
    sa, sb = sw.Strs(a), sw.Strs(b)
    assert_counts(lev.jaro_counts(sa, sb, scope), want, describe)
    assert (lev.jaro(sa, sb, scope) == jaro).all() and (lev.jaro_winkler(sa, sb, scope) == winkler).all()
    assert_counts(lev.jaro_counts_cross(sw.Strs(queries), None, scope), want_cross)
