"""LCS lengths, Indel distances and ratios (swh_levenshtein_lcs_*): rapidfuzz's distance.LCSseq, distance.Indel and fuzz.ratio.

The reference is computed here with numpy: the LCS table row by row, for a whole batch of pairs at once (the pairs are padded to one
shape with symbols that match nothing; pair k's length is read at row m_k, column n_k). A by-definition LCS (every subsequence of
one string looked for in the other) pins it on all pairs of short strings, the header's worked examples and the oracle's general-cost
Levenshtein distance at (0, 2, 1, 1) pin it further, all on the CPU; only then is it held against the GPU, exactly."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# a, b, LCS, indel, ratio: the worked examples of include/stringwars_amd.h
EXAMPLES = [("kitten", "sitting", 4, 5, 200 * 4 / 13), ("ab", "ba", 1, 2, 50.0), ("abc", "abc", 3, 0, 100.0), ("", "", 0, 0, 100.0),
            ("abc", "", 0, 3, 0.0)]
LCS_SYMBOLS = ("swh_levenshtein_lcs_pairs_u64tape", "swh_levenshtein_utf8_lcs_pairs_u64tape", "swh_levenshtein_lcs_pairs_prepared",
               "swh_levenshtein_lcs_cross_u64tape", "swh_levenshtein_utf8_lcs_cross_u64tape", "swh_levenshtein_lcs_cross_prepared")
METHODS = ("lcs", "indel", "ratio", "lcs_cross", "indel_cross", "ratio_cross")


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def symbols(s, utf8=False) -> np.ndarray:
    if isinstance(s, str):
        return np.array([ord(c) for c in s], dtype=np.int64) if utf8 else np.frombuffer(s.encode(), dtype=np.uint8).astype(np.int64)
    return np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64)


def _lcs_batch(rows, columns) -> np.ndarray:
    """LCS lengths of rows[k] against columns[k] (lists of int64 arrays), all pairs advancing through one padded table."""
    count = len(rows)
    ms, ns = np.array([len(x) for x in rows]), np.array([len(x) for x in columns])
    M, N = int(ms.max(initial=0)), int(ns.max(initial=0))
    A, B = np.full((count, M), -1, dtype=np.int32), np.full((count, N), -2, dtype=np.int32)
    for k in range(count):
        A[k, :ms[k]] = rows[k]
        B[k, :ns[k]] = columns[k]
    out = np.zeros(count, dtype=np.int64)
    row = np.zeros((count, N + 1), dtype=np.int32)
    tmp = np.zeros((count, N + 1), dtype=np.int32)
    for i in range(1, M + 1):   # L[i][j] = max(L[i-1][j-1] + [a_i = b_j], L[i-1][j], L[i][j-1]): the last term is a running maximum
        np.maximum(row[:, :-1] + (B == A[:, i - 1:i]), row[:, 1:], out=tmp[:, 1:])
        row = np.maximum.accumulate(tmp, axis=1)
        done = np.nonzero(ms == i)[0]
        out[done] = row[done, ns[done]]
    return out


def reference_lcs(a, b, utf8=False, chunk=256) -> np.ndarray:
    """LCS lengths of the pairs (a[k], b[k]); the shorter string of a pair gives the rows, and the pairs are grouped by size so that
    the padding stays small."""
    rows, columns = [symbols(x, utf8) for x in a], [symbols(x, utf8) for x in b]
    for k in range(len(rows)):
        if len(rows[k]) > len(columns[k]):
            rows[k], columns[k] = columns[k], rows[k]
    order = sorted(range(len(rows)), key=lambda k: (len(rows[k]), len(columns[k])))
    out = np.zeros(len(rows), dtype=np.int64)
    at = 0
    while at < len(order):   # a group ends where the rows have grown to twice its first pair's
        end = at + 1
        while end < len(order) and end - at < chunk and len(rows[order[end]]) <= 2 * len(rows[order[at]]) + 16:
            end += 1
        part = order[at:end]
        out[part] = _lcs_batch([rows[k] for k in part], [columns[k] for k in part])
        at = end
    return out


def lengths_of(strs, utf8=False) -> np.ndarray:
    return np.array([len(symbols(x, utf8)) for x in strs], dtype=np.int64)


def reference_indel(a, b, utf8=False, lcs=None) -> np.ndarray:
    lcs = reference_lcs(a, b, utf8) if lcs is None else lcs
    return lengths_of(a, utf8) + lengths_of(b, utf8) - 2 * lcs


def reference_ratio(a, b, utf8=False, lcs=None) -> np.ndarray:
    lcs = reference_lcs(a, b, utf8) if lcs is None else lcs
    total = lengths_of(a, utf8) + lengths_of(b, utf8)
    return np.where(total > 0, 200.0 * lcs / np.maximum(total, 1), 100.0)


def is_subsequence(x, y) -> bool:
    rest = iter(y)
    return all(c in rest for c in x)


def lcs_by_definition(a, b) -> int:
    """The longest subsequence of a that is a subsequence of b, every subsequence of a tried."""
    for size in range(len(a), 0, -1):
        if any(is_subsequence(x, b) for x in set(itertools.combinations(a, size))):
            return size
    return 0


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


def raw_pairs(sw, engine, scope, a, b, indel, lcs, bound=None, stride=0, utf8=False):
    """The C ABI itself on raw u64 tapes; `indel` / `lcs` are pointers (host or device) or None. Returns (status name, message)."""
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True)
    fn = N.lib.swh_levenshtein_utf8_lcs_pairs_u64tape if utf8 else N.lib.swh_levenshtein_lcs_pairs_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb), N.UNBOUNDED if bound is None else bound, C.c_void_p(indel),
                C.c_void_p(lcs), stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def raw_cross(sw, engine, scope, a, b, indel, lcs, stride=0, utf8=False):
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True) if b is not None else (None, None, None)
    fn = N.lib.swh_levenshtein_utf8_lcs_cross_u64tape if utf8 else N.lib.swh_levenshtein_lcs_cross_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb) if tb is not None else None, C.c_void_p(indel), C.c_void_p(lcs),
                stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def assert_same(got, want, describe=lambda k: int(k)):
    got, want = np.asarray(got).astype(np.int64).ravel(), np.asarray(want).astype(np.int64).ravel()
    assert got.shape == want.shape
    wrong = np.nonzero(got != want)[0]
    assert not len(wrong), [(describe(k), int(got[k]), int(want[k])) for k in wrong[:5]]


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in LCS_SYMBOLS:
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "lcs" in sw.capabilities().split(",")
    for name in METHODS:
        assert callable(getattr(sw.LevenshteinDistances, name)), name
        assert getattr(sw.LevenshteinDistancesUTF8, name) is getattr(sw.LevenshteinDistances, name), name
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_LCS_MAX_SHORTER 2048u", header) and N.LCS_MAX_SHORTER == 2048 == sw.LCS_MAX_SHORTER
    test_library = C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    assert all(hasattr(test_library, name) for name in LCS_SYMBOLS)


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    ta, _, keep_a = sw.engines._c_tape(sw.Strs([b"ab"]), want64=True)
    tb, _, keep_b = sw.engines._c_tape(sw.Strs([b"ba"]), want64=True)
    out32, out64 = np.full(2, 77, np.uint32), np.full(2, 77, np.uint64)
    view = N.PreparedView(None, 0, 1)
    for name in LCS_SYMBOLS:
        cross, prepared = "_cross_" in name, name.endswith("_prepared")
        sides = (C.byref(view), C.byref(view)) if prepared else (C.byref(ta), C.byref(tb))
        extra = () if cross else (N.UNBOUNDED,)
        out = out64 if cross else out32
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, *sides, *extra, C.c_void_p(out.ctypes.data), C.c_void_p(out[1:].ctypes.data), 0, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    assert (out32 == 77).all() and (out64 == 77).all()


def test_reference_equals_the_definition():
    for alphabet, upto, count in (("ab", 6, 127), ("abc", 4, 121)):
        strs = all_strings(alphabet, upto)
        assert len(strs) == count
        a, b = expanded(strs, strs)
        got = reference_lcs(a, b, chunk=4096)
        by_definition = {}
        for x, y, g in zip(a, b, got):
            if (y, x) in by_definition:   # the definition is symmetric; the reference is held to that too
                want = by_definition[(y, x)]
            else:
                want = by_definition[(x, y)] = lcs_by_definition(x, y)
            assert g == want, (x, y, int(g), want)


def test_reference_worked_examples():
    a, b = [e[0] for e in EXAMPLES], [e[1] for e in EXAMPLES]
    assert reference_lcs(a, b).tolist() == [e[2] for e in EXAMPLES] == [lcs_by_definition(x, y) for x, y in zip(a, b)]
    assert reference_indel(a, b).tolist() == [e[3] for e in EXAMPLES]
    assert np.allclose(reference_ratio(a, b), [e[4] for e in EXAMPLES], rtol=0, atol=1e-12)
    assert abs(reference_ratio(["kitten"], ["sitting"])[0] - 61.53846153846154) < 1e-12   # 100 (1 - 5 / 13), what fuzz.ratio gives
    # the utf8 switch counts code points, not bytes: é and è share their first byte
    assert reference_lcs(["é"], ["è"], utf8=True).tolist() == [0] and reference_lcs(["é"], ["è"]).tolist() == [1]


def test_reference_against_oracle_general_costs(orc, sw):
    rng = np.random.default_rng(60)
    a, b = [], []
    for i in range(2000):
        alphabet = int(rng.integers(2, 27))
        x = rand_bytes(rng, rng.integers(0, 301), alphabet)
        if i % 2:
            y = bytes(mutated(rng, x, int(rng.integers(0, 12)), lambda: int(rng.integers(97, 97 + alphabet))))[:300]
        else:
            y = rand_bytes(rng, rng.integers(0, 301), alphabet)
        a.append(x); b.append(y)
    want = np.asarray(orc.levenshtein_costs_pairs(sw.Strs(a), sw.Strs(b), 0, 2, 1, 1)).astype(np.int64)
    assert_same(reference_indel(a, b), want)


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
        got = engine.lcs(a, b, scope)
        assert got.dtype == np.uint32 and got.tolist() == [e[2] for e in EXAMPLES]
        got = engine.indel(a, b, scope)
        assert got.dtype == np.uint32 and got.tolist() == [e[3] for e in EXAMPLES]
        got = engine.ratio(a, b, scope)
        assert got.dtype == np.float64 and got.tolist() == [e[4] for e in EXAMPLES]   # 200.0 * L / (d + 2 L), the same expression
        assert engine.ratio([b"kitten"], [b"sitting"], scope)[0] == 200.0 * 4 / 13    # lists are accepted
    for alphabet, engine, utf8 in (("ab", lev, False), ("aé", lev8, True)):
        strs = all_strings(alphabet, 6)
        assert len(strs) == 127
        x, y = expanded(strs, strs)
        want = reference_lcs(x, y, utf8=utf8, chunk=4096)
        matrix = engine.lcs_cross(sw.Strs(strs), sw.Strs(strs), scope)
        assert matrix.dtype == np.uint64 and matrix.shape == (127, 127)
        assert_same(matrix, want, lambda k: (x[k], y[k]))
        assert_same(engine.indel_cross(sw.Strs(strs), sw.Strs(strs), scope), reference_indel(x, y, utf8, lcs=want))
        ratios = engine.ratio_cross(sw.Strs(strs), None, scope)
        assert ratios.dtype == np.float64 and (ratios.ravel() == reference_ratio(x, y, utf8, lcs=want)).all()


BLOCK_M = (1, 31, 32, 33, 63, 64, 65, 96, 97, 2047, 2048)


def block_edge_cases():
    """(m, kind, shorter, longer) for every shorter length m against n = m, m + 1 and 2 m + 3."""
    rng = np.random.default_rng(61)
    cases = []
    for m in BLOCK_M:
        ripple = b"a" + b"b" * (m - 1)   # its one match is in row 0: the carry of that addition ripples through every block, one hop per step
        cases += [(m, "ripple/a", ripple, b"a"), (m, "ripple/ab", ripple, b"ab")]
        for n in (m, m + 1, 2 * m + 3):
            cases.append((m, "one symbol", b"a" * m, b"a" * n))   # a carry out of every block in every column
            cases.append((m, "ripple/a*n", ripple, b"a" * n))
            for alphabet in (2, 26):
                cases.append((m, "random %d" % alphabet, rand_bytes(rng, m, alphabet), rand_bytes(rng, n, alphabet)))
            base = rand_bytes(rng, m, 4)
            copy = mutated(rng, base, 1 + m // 16, lambda: int(rng.integers(97, 101)))
            while len(copy) < n:
                copy.insert(int(rng.integers(0, len(copy) + 1)), int(rng.integers(97, 101)))
            cases.append((m, "mutated", base, bytes(copy[:max(n, m)])))
    return cases


@pytest.mark.gpu
def test_block_edges_and_carries(sw, scope, lev):
    cases = block_edge_cases()
    a, b = [c[2] for c in cases], [c[3] for c in cases]
    assert {len(x) for x in a} == set(BLOCK_M)
    want = reference_lcs(a, b, chunk=16)
    for k, c in enumerate(cases):   # what the constructed cases are known to give
        if c[1] == "one symbol":
            assert want[k] == c[0]
        elif c[1].startswith("ripple"):
            assert want[k] == (1 if c[1] != "ripple/ab" or c[0] == 1 else 2)
    describe = lambda k: (cases[k][0], cases[k][1], len(b[k]))
    sa, sb = sw.Strs(a), sw.Strs(b)
    assert_same(lev.lcs(sa, sb, scope), want, describe)     # a is the rows' string (but for the ripple against a / ab)
    assert_same(lev.lcs(sb, sa, scope), want, describe)     # b is
    assert_same(lev.indel(sa, sb, scope), reference_indel(a, b, lcs=want), describe)


@pytest.mark.gpu
def test_mixed_items(sw, scope, lev):
    """One batch whose block counts run 1..64 in shuffled order, with empty strings on either or both sides: pairs of different G
    share a wave, lanes idle past a shorter string, and the last run of 64 pairs is partial."""
    rng = np.random.default_rng(62)
    count = 64 * 3 + 5
    blocks = np.concatenate([rng.permutation(64) + 1 for _ in range(4)])[:count]
    a, b = [], []
    for i in range(count):
        m = int(blocks[i]) * 32 - int(rng.integers(0, 32))
        x = rand_bytes(rng, m, 4)
        kind = i % 7 if i >= 64 else 3   # (the first run of 64 pairs holds every block count)
        if kind == 0:
            x, y = b"", rand_bytes(rng, rng.integers(0, 50), 4)   # an empty shorter string, of either side
        elif kind == 1:
            y = b""
        elif kind == 2:
            y = bytes(mutated(rng, x, int(rng.integers(1, 9)), lambda: int(rng.integers(97, 101))))
        else:
            y = rand_bytes(rng, m + int(rng.integers(0, 200)), 4)
        if i % 2:
            x, y = y, x
        a.append(x); b.append(y)
    a[5], b[5] = b"", b""
    assert {max(1, (min(len(x), len(y)) + 31) // 32) for x, y in zip(a, b)} == set(range(1, 65))
    want = reference_lcs(a, b, chunk=16)
    describe = lambda k: (int(k), len(a[k]), len(b[k]))
    assert_same(lev.lcs(sw.Strs(a), sw.Strs(b), scope), want, describe)
    assert_same(lev.indel(sw.Strs(a), sw.Strs(b), scope), reference_indel(a, b, lcs=want), describe)
    order = rng.permutation(count)   # a pair's result does not depend on its neighbours
    again = lev.lcs(sw.Strs([a[k] for k in order]), sw.Strs([b[k] for k in order]), scope)
    assert_same(again, want[order])


@pytest.mark.gpu
def test_bounds(sw, scope, lev):
    rng = np.random.default_rng(63)
    a = [rand_bytes(rng, rng.integers(0, 150), 6) for _ in range(600)]
    b = [bytes(mutated(rng, x, k % 12, lambda: int(rng.integers(97, 103)))) for k, x in enumerate(a)]
    for d in (16, 17, 18, 19, 40):   # a copy with d symbols appended is at distance d exactly: both sides of every bound below
        a.append(a[d]); b.append(a[d] + rand_bytes(rng, d, 6))
    count = len(a)
    lcs = reference_lcs(a, b)
    want = reference_indel(a, b, lcs=lcs)
    assert want[-5:].tolist() == [16, 17, 18, 19, 40] and {0, 1, 2, 17, 18, 19} <= set(want.tolist())
    sa, sb = sw.Strs(a), sw.Strs(b)
    from stringwars_amd import _native as N
    for bound in (0, 1, 17, int(want.max()) + 1, None):
        clamped = want if bound is None else np.minimum(want, bound + 1)
        assert_same(lev.indel(sa, sb, scope, bound=bound), clamped)
        indel, length = np.zeros(count, np.uint32), np.zeros(count, np.uint32)   # the bound leaves the LCS length alone
        status, message = raw_pairs(sw, lev, scope, sa, sb, indel.ctypes.data, length.ctypes.data, bound=bound)
        assert status == "success", message
        assert_same(indel, clamped)
        assert_same(length, lcs)


@pytest.mark.gpu
def test_forms_and_scopes(sw, scope, lev):
    import torch
    from stringwars_amd import _native as N
    rng = np.random.default_rng(64)
    a = [rand_bytes(rng, rng.integers(0, 300), 4) for _ in range(700)]
    b = [bytes(mutated(rng, x, int(rng.integers(0, 9)), lambda: int(rng.integers(97, 101)))) if k % 2 else rand_bytes(rng, rng.integers(0, 300), 4)
         for k, x in enumerate(a)]
    sa, sb = sw.Strs(a), sw.Strs(b)
    lcs = reference_lcs(a, b)
    indel = np.minimum(reference_indel(a, b, lcs=lcs), 21)
    assert (indel == 21).any() and (indel < 21).any()
    # only indel, only lcs, both -- on the host
    assert_same(lev.indel(sa, sb, scope, bound=20), indel)
    assert_same(lev.lcs(sa, sb, scope), lcs)
    h_indel, h_lcs = np.full(700, 77, np.uint32), np.full(700, 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, sa, sb, h_indel.ctypes.data, h_lcs.ctypes.data, bound=20)
    assert status == "success", message
    assert_same(h_indel, indel); assert_same(h_lcs, lcs)
    # device outputs: both, each alone, and one of each kind
    d_indel, d_lcs = (torch.full((700,), 77, dtype=torch.int32, device="cuda") for _ in range(2))
    status, message = raw_pairs(sw, lev, scope, sa, sb, d_indel.data_ptr(), d_lcs.data_ptr(), bound=20)
    assert status == "success", message
    assert_same(d_indel.cpu().numpy(), indel); assert_same(d_lcs.cpu().numpy(), lcs)
    d_indel.fill_(77); d_lcs.fill_(77)
    assert raw_pairs(sw, lev, scope, sa, sb, d_indel.data_ptr(), None, bound=20)[0] == "success"
    assert_same(d_indel.cpu().numpy(), indel); assert (d_lcs.cpu().numpy() == 77).all()
    d_indel.fill_(77)
    assert raw_pairs(sw, lev, scope, sa, sb, None, d_lcs.data_ptr(), bound=20)[0] == "success"
    assert_same(d_lcs.cpu().numpy(), lcs); assert (d_indel.cpu().numpy() == 77).all()
    h_indel.fill(77); d_lcs.fill_(77)
    assert raw_pairs(sw, lev, scope, sa, sb, h_indel.ctypes.data, d_lcs.data_ptr(), bound=20)[0] == "success"
    assert_same(h_indel, indel); assert_same(d_lcs.cpu().numpy(), lcs)
    # stride 12, host and device: the gaps stay as they were
    wide = np.full((700, 3), 77, np.uint32)
    assert lev.indel(sa, sb, scope, bound=20, out=wide[:, 1]) is not None and lev.lcs(sa, sb, scope, out=wide[:, 2]) is not None
    assert_same(wide[:, 1], indel); assert_same(wide[:, 2], lcs); assert (wide[:, 0] == 77).all()
    wide = np.full((700, 3), 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, sa, sb, wide.ctypes.data, wide.ctypes.data + 8, bound=20, stride=12)
    assert status == "success", message
    assert_same(wide[:, 0], indel); assert_same(wide[:, 2], lcs); assert (wide[:, 1] == 77).all()
    wide_d = torch.full((700, 3), 77, dtype=torch.int32, device="cuda")
    status, message = raw_pairs(sw, lev, scope, sa, sb, wide_d.data_ptr() + 4, wide_d.data_ptr() + 8, bound=20, stride=12)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert_same(back[:, 1], indel); assert_same(back[:, 2], lcs); assert (back[:, 0] == 77).all()
    # raw device tapes, raw u64 tapes; prepared tapes in all four offset-width mixes, whole and as sub-views
    assert_same(lev.indel(sa.to_device(scope), sb.to_device(scope), scope, bound=20), indel)
    da, db = sa.with_offsets(np.uint64).to_device(scope), sb.with_offsets(np.uint64).to_device(scope)
    host = np.full(700, 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, da, db, None, host.ctypes.data)
    assert status == "success", message
    assert_same(host, lcs)
    tapes = {(w, name): sw.PreparedTape(scope, sw.Strs(items).with_offsets(w)) for w in (np.uint32, np.uint64)
             for name, items in (("a", a), ("b", b))}
    for wa, wb in itertools.product((np.uint32, np.uint64), repeat=2):
        pa, pb = tapes[(wa, "a")], tapes[(wb, "b")]
        assert_same(lev.indel(pa, pb, scope, bound=20), indel)
        assert_same(lev.lcs(pa[37:333], pb[37:333], scope), lcs[37:333])
        on_device = torch.zeros(296, dtype=torch.int32, device="cuda")
        lev.indel(pa[37:333], pb[37:333], scope, bound=20, out=on_device)
        assert_same(on_device.cpu().numpy(), indel[37:333])
    assert (lev.ratio(tapes[(np.uint32, "a")], tapes[(np.uint64, "b")], scope) == reference_ratio(a, b, lcs=lcs)).all()
    # tapes of two kinds: refused by the C ABI, nothing written
    as_utf8 = sw.PreparedTape(scope, sb, utf8=True)
    va, vb, err = tapes[(np.uint64, "a")].view(), as_utf8.view(), C.c_char_p()
    untouched = np.full(700, 77, np.uint32)
    status = N.lib.swh_levenshtein_lcs_pairs_prepared(lev._handle, scope.handle, C.byref(va), C.byref(vb), N.UNBOUNDED,
                                                      C.c_void_p(untouched.ctypes.data), None, 0, C.byref(err))
    assert N.STATUS_NAMES[status] == "invalid_argument" and (untouched == 77).all()
    # a caller-stream scope -- synchronous, then asynchronous, then pipelined: the results are visible when the call returns
    other = sw.DeviceScope(gpu_device=0, stream=torch.cuda.current_stream().cuda_stream)
    engine = sw.LevenshteinDistances(capabilities=other)
    assert_same(engine.indel(sa, sb, other, bound=20), indel)
    for mode in ("async", "pipelined"):
        if mode == "async":
            other.set_async(True)
        else:
            other.set_async(False)
            other.set_pipelined(True)
        engine.pairs(sa, sb, other)   # outstanding work the call joins
        assert_same(engine.lcs(sa, sb, other), lcs)
        other.synchronize()
    # profiling describes the whole call
    scope.set_profiling(True)
    try:
        lev.indel(sa, sb, scope)
        timing = scope.last_timing()
        lev.lcs_cross(sa[:60], sb[:50], scope)
        cross_timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["cells"] == int((sa.lengths * sb.lengths).sum())
    assert timing["dominant_name"] == "lcs" and timing["kernels"] == 2
    assert cross_timing["cells"] == int(sa.lengths[:60].sum()) * int(sb.lengths[:50].sum()) and cross_timing["dominant_name"] == "lcs"


def golden_strings(name, sides):
    z = np.load(os.path.join(GOLDEN, name))
    out = []
    for side in sides:
        data, offsets = z[side + "_data"], z[side + "_offsets"].astype(np.int64)
        out.append([bytes(data[offsets[i]:offsets[i + 1]]).decode("utf-8") for i in range(len(offsets) - 1)])
    return out


@pytest.mark.gpu
def test_utf8(sw, scope, lev, lev8):
    rng = np.random.default_rng(65)
    lines_a, lines_b = golden_strings("script_lines.npz", "ab")
    queries, candidates = golden_strings("uwords.npz", "qc")
    count = min(len(queries), len(candidates), 400)
    a, b = list(lines_a[:150]) + queries[:count], list(lines_b[:150]) + candidates[:count]
    # a 1- to 4-byte code-point alphabet, with the first and last code point of every length
    mixed = [0x61, 0x62, 0xE9, 0x3B1, 0x4E2D, 0x6587, 0x1F600, 0x10FFFF, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000]
    renamed = {cp: 65 + k for k, cp in enumerate(mixed)}
    first = len(a)
    for i in range(300):
        x = [int(rng.choice(mixed)) for _ in range(int(rng.integers(0, 100)))]
        y = mutated(rng, x, int(rng.integers(0, 6)), lambda: int(rng.choice(mixed)))
        a.append("".join(map(chr, x))); b.append("".join(map(chr, y)))
    a.append("é"); b.append("è")   # no code point in common, one byte in common
    assert any(len(x.encode()) > len(x) for x in a[:first])
    want = reference_lcs(a, b, utf8=True)
    got = lev8.lcs(sw.Strs(a), sw.Strs(b), scope)
    assert_same(got, want)
    assert_same(lev8.indel(sw.Strs(a), sw.Strs(b), scope), reference_indel(a, b, utf8=True, lcs=want))
    assert got[-1] == 0 and lev.lcs(sw.Strs(a[-1:]), sw.Strs(b[-1:]), scope)[0] == 1
    # the byte call on the strings with the code points renamed to bytes
    as_bytes = lambda strs: [bytes(renamed[ord(c)] for c in s) for s in strs]
    assert_same(lev.lcs(sw.Strs(as_bytes(a[first:-1])), sw.Strs(as_bytes(b[first:-1])), scope), got[first:-1])
    prepared = lev8.lcs(sw.PreparedTape(scope, sw.Strs(a), utf8=True), sw.PreparedTape(scope, sw.Strs(b), utf8=True), scope)
    assert (prepared == got).all()
    some = slice(first - 20, first + 20)
    matrix = lev8.lcs_cross(sw.Strs(a[some]), sw.Strs(b[some]), scope)
    assert_same(np.diagonal(matrix), want[some])
    scope.set_profiling(True)
    try:
        lev8.lcs(sw.Strs(a), sw.Strs(b), scope)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["dominant_name"] == "lcs_u32" and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    # invalid UTF-8 in either tape: the status, and the outputs untouched
    out, matrix = np.full(2, 77, np.uint32), np.full((2, 2), 77, np.uint64)
    for bad_a, bad_b in (([b"ok", b"\xff\xfe"], [b"ok", b"x"]), ([b"ok", b"x"], [b"ok", b"\xc3"])):
        status, _ = raw_pairs(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), out.ctypes.data, None, utf8=True)
        assert status == "invalid_utf8" and (out == 77).all()
        status, _ = raw_cross(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), None, matrix.ctypes.data, utf8=True)
        assert status == "invalid_utf8" and (matrix == 77).all()


def cross_batch():
    rng = np.random.default_rng(66)
    queries = [rand_bytes(rng, rng.integers(0, 90), 4) for _ in range(37)]
    candidates = [bytes(mutated(rng, queries[k % 37], int(rng.integers(0, 5)), lambda: int(rng.integers(97, 101)))) for k in range(53)]
    return queries, candidates


@pytest.mark.gpu
def test_cross(sw, scope, lev):
    import torch
    queries, candidates = cross_batch()
    sq, sc = sw.Strs(queries), sw.Strs(candidates)
    a, b = expanded(queries, candidates)
    lcs = reference_lcs(a, b).reshape(37, 53)
    indel = reference_indel(a, b, lcs=lcs.ravel()).reshape(37, 53)
    matrix = lev.lcs_cross(sq, sc, scope)
    assert matrix.dtype == np.uint64 and matrix.shape == (37, 53)
    assert_same(matrix, lcs)
    assert_same(lev.indel_cross(sq, sc, scope), indel)
    assert (lev.ratio_cross(sq, sc, scope).ravel() == reference_ratio(a, b, lcs=lcs.ravel())).all()
    # a row stride wider than the row, on the host and on the device, both matrices in one call: the columns past them stay
    wide = np.full((2, 37, 56), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sq, sc, wide[0].ctypes.data, wide[1].ctypes.data, stride=56 * 8)
    assert status == "success", message
    assert_same(wide[0, :, :53], indel); assert_same(wide[1, :, :53], lcs); assert (wide[:, :, 53:] == 77).all()
    wide_d = torch.full((2, 37, 56), 77, dtype=torch.int64, device="cuda")
    status, message = raw_cross(sw, lev, scope, sq, sc, wide_d[0].data_ptr(), wide_d[1].data_ptr(), stride=56 * 8)
    assert status == "success", message
    assert (wide_d.cpu().numpy() == wide.astype(np.int64)).all()
    out = np.full((37, 56), 77, np.uint64)
    lev.lcs_cross(sq, sc, scope, out=out[:, :53])
    assert_same(out[:, :53], lcs); assert (out[:, 53:] == 77).all()
    # device and prepared tapes
    assert_same(lev.lcs_cross(sq.to_device(scope), sc.to_device(scope), scope), lcs)
    pq, pc = sw.PreparedTape(scope, sq.with_offsets(np.uint32)), sw.PreparedTape(scope, sc.with_offsets(np.uint64))
    assert_same(lev.indel_cross(pq, pc, scope), indel)
    assert_same(lev.lcs_cross(pq[5:30], pc[3:], scope), lcs[5:30, 3:])
    # b == NULL: the self-product, symmetric, the diagonal holds indel = 0 and lcs = len
    own = np.full((2, 37, 37), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sq, None, own[0].ctypes.data, own[1].ctypes.data)
    assert status == "success", message
    assert (own[0] == own[0].T).all() and (own[1] == own[1].T).all()
    assert (np.diagonal(own[0]) == 0).all() and (np.diagonal(own[1]) == sq.lengths).all()
    a, b = expanded(queries, queries)
    assert_same(own[1], reference_lcs(a, b))
    assert (lev.lcs_cross(sq, None, scope) == own[1]).all() and (lev.indel_cross(pq, None, scope) == own[0]).all()
    assert lev.lcs_cross(sw.Strs([]), sw.Strs([b"a"]), scope).shape == (0, 1)


@pytest.mark.gpu
def test_cross_in_many_chunks(request, sw):
    """STRINGWARS_AMD_LCS_CHUNK_PAIRS (test library) shrinks the slices of whole rows to 424 pairs, so the 37 x 53 product runs as
    four slices of eight rows and a ragged fifth of five, with the same results on the host and on the device."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_LCS_CHUNK_PAIRS="424"), test_library=True):
        return
    import torch
    scope = sw.DeviceScope(gpu_device=0)
    lev = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = cross_batch()
    a, b = expanded(queries, candidates)
    lcs = reference_lcs(a, b).reshape(37, 53)
    indel = reference_indel(a, b, lcs=lcs.ravel()).reshape(37, 53)
    scope.set_profiling(True)
    matrix = lev.lcs_cross(sw.Strs(queries), sw.Strs(candidates), scope)
    timing = scope.last_timing()
    scope.set_profiling(False)
    assert_same(matrix, lcs)
    assert timing["kernels"] == 1 + 2 * 5 and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    wide_d = torch.full((2, 37, 56), 77, dtype=torch.int64, device="cuda")
    status, message = raw_cross(sw, lev, scope, sw.Strs(queries), sw.Strs(candidates), wide_d[0].data_ptr(), wide_d[1].data_ptr(), stride=56 * 8)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert_same(back[0, :, :53], indel); assert_same(back[1, :, :53], lcs); assert (back[:, :, 53:] == 77).all()
    host, on_device = np.full((37, 53), 77, np.uint64), torch.full((37, 53), 77, dtype=torch.int64, device="cuda")   # one of each kind
    status, message = raw_cross(sw, lev, scope, sw.Strs(queries), sw.Strs(candidates), host.ctypes.data, on_device.data_ptr())
    assert status == "success", message
    assert_same(host, indel); assert_same(on_device.cpu().numpy(), lcs)
    # a refusal still comes before the first row is written
    long_q = [b"ab"] * 300 + [b"a" * 2049]
    long_c = [b"ab", b"b" * 2049, b"c" * 3000]
    untouched = np.full((301, 3), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sw.Strs(long_q), sw.Strs(long_c), untouched.ctypes.data, None)
    assert status == "unsupported_length" and "pair (300, 1)" in message and (untouched == 77).all(), message


@pytest.mark.gpu
def test_refusals(sw, scope, lev):
    rng = np.random.default_rng(67)
    a = [b"abc", rand_bytes(rng, 2048, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 3000, 4)]
    b = [b"acb", rand_bytes(rng, 2048, 4), rand_bytes(rng, 5, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 4000, 4)]
    indel, lcs = np.full(5, 77, np.uint32), np.full(5, 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, sw.Strs(a), sw.Strs(b), indel.ctypes.data, lcs.ctypes.data)
    assert status == "unsupported_length" and "pair 3" in message and "2049" in message, message
    assert (indel == 77).all() and (lcs == 77).all()
    with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
        lev.lcs(sw.Strs(a), sw.Strs(b), scope)
    assert "pair 3" in str(info.value)
    matrix = np.full((5, 5), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sw.Strs(a), sw.Strs(b), matrix.ctypes.data, None)
    assert status == "unsupported_length" and "pair (2, 3)" in message and (matrix == 77).all(), message
    assert_same(lev.lcs(sw.Strs(a[:3]), sw.Strs(b[:3]), scope), reference_lcs(a[:3], b[:3]))   # 2048 x 2048 and 2049 x 5 are accepted
    # a general-cost engine
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    for call in (costly.lcs, costly.indel, costly.ratio, costly.lcs_cross, costly.indel_cross, costly.ratio_cross):
        with pytest.raises(sw.StringWarsError, match="not_implemented"):
            call(sw.Strs([b"ab"]), sw.Strs([b"ba"]), scope)
    # count mismatch, both outputs null, stride 2
    status, _ = raw_pairs(sw, lev, scope, sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), indel.ctypes.data, lcs.ctypes.data)
    assert status == "invalid_argument"
    with pytest.raises(ValueError):
        lev.lcs(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope)
    assert raw_pairs(sw, lev, scope, sw.Strs(a[:2]), sw.Strs(b[:2]), None, None)[0] == "invalid_argument"
    assert raw_cross(sw, lev, scope, sw.Strs(a[:2]), sw.Strs(b[:2]), None, None)[0] == "invalid_argument"
    assert raw_pairs(sw, lev, scope, sw.Strs(a[:2]), sw.Strs(b[:2]), indel.ctypes.data, lcs.ctypes.data, stride=2)[0] == "invalid_argument"
    assert (indel == 77).all() and (lcs == 77).all()
    # count == 0: success, nothing written
    assert len(lev.lcs(sw.Strs([]), sw.Strs([]), scope)) == 0 and len(lev.ratio(sw.Strs([]), sw.Strs([]), scope)) == 0
    status, _ = raw_pairs(sw, lev, scope, sw.Strs([]), sw.Strs([]), indel.ctypes.data, lcs.ctypes.data)
    assert status == "success" and (indel == 77).all() and (lcs == 77).all()


@pytest.mark.gpu
def test_against_the_general_cost_route(sw, scope, lev):
    """Two unrelated kernels, one answer: the wavefront kernel at costs (0, 2, 1, 1) scores cell by cell what k_lcs scores in words."""
    rng = np.random.default_rng(68)
    a, b = [], []
    for i in range(1500):
        alphabet = (2, 4, 26)[i % 3]
        x = rand_bytes(rng, rng.integers(0, 301), alphabet)
        if i % 2:
            y = bytes(mutated(rng, x, int(rng.integers(0, 12)), lambda: int(rng.integers(97, 97 + alphabet))))
        else:
            y = rand_bytes(rng, rng.integers(0, 301), alphabet)
        a.append(x); b.append(y)
    sa, sb = sw.Strs(a), sw.Strs(b)
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    assert_same(lev.indel(sa, sb, scope), costly.pairs(sa, sb, scope))
    bounded = costly.pairs(sa, sb, scope, bound=9)
    assert (bounded == 10).any() and (bounded < 10).any()
    assert_same(lev.indel(sa, sb, scope, bound=9), bounded)


LENGTH_CLASSES = ((0, 16, 0.40), (17, 64, 0.30), (65, 300, 0.2925), (301, 2048, 0.0075))


@pytest.mark.gpu
def test_seeded_random_round(sw, scope, lev):
    """20 000 pairs over all length classes and alphabets 2 / 4 / 26 / 256 (the long class is drawn rarely: it holds most of the
    reference's cells), and a 150 x 150 cross-product."""
    rng = np.random.default_rng(2029)
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
            y = bytes(mutated(rng, x, int(edits[i]), lambda: base + int(rng.integers(0, alphabet))))
        else:
            other = LENGTH_CLASSES[int(rng.integers(0, kinds[i] + 1))]
            y = rand_bytes(rng, rng.integers(other[0], other[1] + 1), alphabet, base)
        if i % 2:
            x, y = y, x
        a.append(x); b.append(y)
    assert (kinds == 3).sum() >= 100
    want = reference_lcs(a, b)
    queries = [rand_bytes(rng, rng.integers(0, 120), (2, 4, 26)[k % 3]) for k in range(150)]
    qa, qb = expanded(queries, queries)
    want_cross = reference_lcs(qa, qb, chunk=1024)
    # every random number is drawn and the references are computed: the device comes now
    describe = lambda k: (int(k), len(a[k]), len(b[k]))
    sa, sb = sw.Strs(a), sw.Strs(b)
    assert_same(lev.lcs(sa, sb, scope), want, describe)
    assert_same(lev.indel(sa, sb, scope), reference_indel(a, b, lcs=want), describe)
    assert (lev.ratio(sa, sb, scope) == reference_ratio(a, b, lcs=want)).all()
    assert_same(lev.lcs_cross(sw.Strs(queries), None, scope), want_cross)
    assert_same(lev.indel_cross(sw.Strs(queries), sw.Strs(queries), scope), reference_indel(qa, qb, lcs=want_cross))
