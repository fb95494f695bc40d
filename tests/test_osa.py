"""Damerau-Levenshtein distances in the optimal-string-alignment form (swh_levenshtein_osa_*): a swap of two neighbouring symbols costs
one edit, no substring is edited twice.

The reference is computed here with numpy: the Wagner-Fischer matrix with the transposition case, row by row and for a whole batch of
pairs at once (the pairs are padded to one shape with symbols that match nothing; pair k's distance is read at row m_k, column n_k).
A recursive definition pins it on every pair of short strings, the known values and the oracle's plain Levenshtein distance pin it
further, all on the CPU; only then is it held against the GPU, exactly."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KNOWN = [("ab", "ba", 1), ("abcd", "acbd", 1), ("ca", "abc", 3), ("kitten", "sitting", 3)]


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def symbols(s, utf8=False) -> np.ndarray:
    if isinstance(s, str):
        return np.array([ord(c) for c in s], dtype=np.int64) if utf8 else np.frombuffer(s.encode(), dtype=np.uint8).astype(np.int64)
    return np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64)


def _osa_batch(rows, columns) -> np.ndarray:
    """OSA distances of rows[k] against columns[k] (lists of int64 arrays), all pairs advancing through one padded matrix."""
    count = len(rows)
    ms, ns = np.array([len(x) for x in rows]), np.array([len(x) for x in columns])
    M, N = int(ms.max(initial=0)), int(ns.max(initial=0))
    A, B = np.full((count, M), -1, dtype=np.int32), np.full((count, N), -2, dtype=np.int32)
    for k in range(count):
        A[k, :ms[k]] = rows[k]
        B[k, :ns[k]] = columns[k]
    ar = np.arange(N + 1, dtype=np.int32)
    out = np.zeros(count, dtype=np.int64)
    out[ms == 0] = ns[ms == 0]
    before, row = None, np.broadcast_to(ar, (count, N + 1)).copy()
    tmp = np.empty((count, N + 1), dtype=np.int32)
    for i in range(1, M + 1):
        ai = A[:, i - 1:i]
        tmp[:, 0] = i
        np.minimum(row[:, :-1] + (B != ai), row[:, 1:] + 1, out=tmp[:, 1:])
        if i >= 2 and N >= 2:   # column j >= 2: a[i-1] = b[j-2] and a[i-2] = b[j-1] -> D[i-2][j-2] + 1
            swapped = (B[:, :-1] == ai) & (B[:, 1:] == A[:, i - 2:i - 1])
            np.minimum(tmp[:, 2:], np.where(swapped, before[:, :-2] + 1, np.int32(1 << 30)), out=tmp[:, 2:])
        before, row = row, np.minimum.accumulate(tmp - ar, axis=1) + ar
        done = np.nonzero(ms == i)[0]
        out[done] = row[done, ns[done]]
    return out


def reference_osa(a, b, utf8=False, chunk=256) -> np.ndarray:
    """OSA distances of the pairs (a[k], b[k]); the pairs are grouped by size so that the padding stays small."""
    rows, columns = [symbols(x, utf8) for x in a], [symbols(x, utf8) for x in b]
    order = sorted(range(len(rows)), key=lambda k: (len(rows[k]), len(columns[k])))
    out = np.zeros(len(rows), dtype=np.int64)
    at = 0
    while at < len(order):   # a group ends where the rows have grown to twice its first pair's
        end = at + 1
        while end < len(order) and end - at < chunk and len(rows[order[end]]) <= 2 * len(rows[order[at]]) + 16:
            end += 1
        part = order[at:end]
        out[part] = _osa_batch([rows[k] for k in part], [columns[k] for k in part])
        at = end
    return out


def osa_by_definition(a, b) -> int:
    """The recursive definition, memoised: D over prefixes, with the transposition case."""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        best = min(d(i - 1, j - 1) + (a[i - 1] != b[j - 1]), d(i - 1, j) + 1, d(i, j - 1) + 1)
        if i >= 2 and j >= 2 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
            best = min(best, d(i - 2, j - 2) + 1)
        return best
    return d(len(a), len(b))


def has_swapped_neighbours(a, b) -> bool:
    """Two adjacent distinct symbols of one string occur swapped in the other."""
    forward = {(a[i], a[i + 1]) for i in range(len(a) - 1) if a[i] != a[i + 1]}
    return any((b[j + 1], b[j]) in forward for j in range(len(b) - 1))


def rand_bytes(rng, n, alphabet, base=97):
    return bytes((rng.integers(0, alphabet, size=int(n)) + base).astype(np.uint8))


def mutated(rng, s, edits, draw):
    """`edits` random edits of s: substitutions, insertions, deletions and swaps of neighbours."""
    s = list(s)
    for _ in range(edits):
        op, at = int(rng.integers(0, 4)), int(rng.integers(0, max(len(s), 1)))
        if op == 0 and s:
            s[at] = draw()
        elif op == 1:
            s.insert(at, draw())
        elif op == 2 and s:
            del s[at]
        elif op == 3 and at + 1 < len(s):
            s[at], s[at + 1] = s[at + 1], s[at]
    return s


def all_strings(alphabet, upto):
    return ["".join(x) for n in range(upto + 1) for x in itertools.product(alphabet, repeat=n)]


def raw_pairs(sw, engine, scope, a, b, out, bound=None, stride=0, utf8=False):
    """The C ABI itself on raw u64 tapes; `out` is a pointer (host or device). Returns (status name, message)."""
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True)
    fn = N.lib.swh_levenshtein_utf8_osa_pairs_u64tape if utf8 else N.lib.swh_levenshtein_osa_pairs_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb), N.UNBOUNDED if bound is None else bound, C.c_void_p(out), stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


def raw_cross(sw, engine, scope, a, b, out, stride=0, utf8=False):
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(a, want64=True)
    tb, _, keep_b = sw.engines._c_tape(b, want64=True) if b is not None else (None, None, None)
    fn = N.lib.swh_levenshtein_utf8_osa_cross_u64tape if utf8 else N.lib.swh_levenshtein_osa_cross_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(ta), C.byref(tb) if tb is not None else None, C.c_void_p(out), stride, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


OSA_SYMBOLS = ("swh_levenshtein_osa_pairs_u64tape", "swh_levenshtein_utf8_osa_pairs_u64tape", "swh_levenshtein_osa_pairs_prepared",
               "swh_levenshtein_osa_cross_u64tape", "swh_levenshtein_utf8_osa_cross_u64tape", "swh_levenshtein_osa_cross_prepared")


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in OSA_SYMBOLS:
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "osa" in sw.capabilities().split(",")
    assert callable(sw.LevenshteinDistances.osa) and sw.LevenshteinDistancesUTF8.osa is sw.LevenshteinDistances.osa
    assert callable(sw.LevenshteinDistances.osa_cross) and sw.LevenshteinDistancesUTF8.osa_cross is sw.LevenshteinDistances.osa_cross
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_OSA_MAX_SHORTER 2048u", header) and N.OSA_MAX_SHORTER == 2048 == sw.OSA_MAX_SHORTER
    test_library = C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    assert all(hasattr(test_library, name) for name in OSA_SYMBOLS)


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    ta, _, keep_a = sw.engines._c_tape(sw.Strs([b"ab"]), want64=True)
    tb, _, keep_b = sw.engines._c_tape(sw.Strs([b"ba"]), want64=True)
    out32, out64 = np.full(1, 77, np.uint32), np.full(1, 77, np.uint64)
    view = N.PreparedView(None, 0, 1)
    for name in OSA_SYMBOLS:
        cross, prepared = "_cross_" in name, name.endswith("_prepared")
        sides = (C.byref(view), C.byref(view)) if prepared else (C.byref(ta), C.byref(tb))
        extra = () if cross else (N.UNBOUNDED,)
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, *sides, *extra, C.c_void_p((out64 if cross else out32).ctypes.data), 0, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    assert out32[0] == 77 and out64[0] == 77


def test_reference_equals_the_definition():
    strs = all_strings("abc", 4)
    pairs = [(a, b) for a in strs for b in strs]
    assert len(pairs) == 121 * 121
    got = reference_osa([a for a, _ in pairs], [b for _, b in pairs])
    mismatches = [(a, b, int(g)) for (a, b), g in zip(pairs, got) if g != osa_by_definition(a, b)]
    assert not mismatches, mismatches[:5]


def test_reference_known_values_and_symmetry():
    for a, b, want in KNOWN:
        assert osa_by_definition(a, b) == want and list(reference_osa([a, b], [b, a])) == [want, want], (a, b)
    rng = np.random.default_rng(50)
    a = [rand_bytes(rng, rng.integers(0, 80), 3) for _ in range(300)]
    b = [bytes(mutated(rng, x, int(rng.integers(0, 6)), lambda: int(rng.integers(97, 100)))) for x in a]
    assert (reference_osa(a, b) == reference_osa(b, a)).all()
    # the utf8 switch counts code points, not bytes
    assert list(reference_osa(["éa"], ["aé"], utf8=True)) == [1] and list(reference_osa(["éa"], ["aé"])) == [2]


def test_reference_against_oracle_levenshtein(orc, sw):
    rng = np.random.default_rng(51)
    a, b = [], []
    for i in range(3000):
        alphabet = (3, 8, 26)[i % 3]
        x = rand_bytes(rng, rng.integers(0, 13), alphabet)
        y = bytes(mutated(rng, x, int(rng.integers(0, 4)), lambda: int(rng.integers(97, 97 + alphabet)))) if i % 2 else rand_bytes(rng, rng.integers(0, 13), alphabet)
        a.append(x); b.append(y)
    osa = reference_osa(a, b)
    lev = np.asarray(orc.levenshtein_pairs(sw.Strs(a), sw.Strs(b), algo="wf")).astype(np.int64)
    assert (osa <= lev).all() and (lev <= 2 * osa).all()
    plain = np.array([not has_swapped_neighbours(x, y) for x, y in zip(a, b)])
    assert plain.sum() >= 300 and (~plain).sum() >= 300
    assert (osa[plain] == lev[plain]).all()
    assert (osa < lev).sum() >= 100 and not plain[osa < lev].any()


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


@pytest.mark.gpu
def test_examples_and_exhaustive(sw, scope, lev, lev8):
    got = lev.osa(sw.Strs([x[0] for x in KNOWN]), sw.Strs([x[1] for x in KNOWN]), scope)
    assert got.dtype == np.uint32 and got.tolist() == [x[2] for x in KNOWN]
    for alphabet, upto, engine, utf8 in (("ab", 7, lev, False), ("aé", 6, lev8, True)):
        strs = all_strings(alphabet, upto)
        assert len(strs) == 2 ** (upto + 1) - 1
        a, b = [x for x in strs for _ in strs], [y for _ in strs for y in strs]
        want = reference_osa(a, b, utf8=utf8, chunk=4096)
        got = engine.osa(sw.Strs(a), sw.Strs(b), scope)
        assert (got.astype(np.int64) == want).all(), np.nonzero(got != want)[0][:5]
        matrix = engine.osa_cross(sw.Strs(strs), sw.Strs(strs), scope)
        assert matrix.dtype == np.uint64 and matrix.shape == (len(strs), len(strs))
        assert (matrix.astype(np.int64).ravel() == want).all()


BLOCK_M = (31, 32, 33, 63, 64, 65, 95, 96, 97, 2047, 2048)
EDGES = (30, 31, 32, 63)   # a swap of positions p | p + 1


def block_edge_cases():
    """(m, kind, a, b): a of m symbols over 8 letters, b a copy of n = m, m + 1 or m - 1 symbols with swaps next to the block edges."""
    rng = np.random.default_rng(52)
    cases = []
    for m in BLOCK_M:
        base = list(rand_bytes(rng, m, 8))
        for p in range(m - 1):   # neighbours differ around the edges, so that every swap there changes the string
            if base[p] == base[p + 1] and min(abs(p - e) for e in EDGES + (m - 2,)) <= 3:
                base[p + 1] = 97 + (base[p] - 97 + 1 + p % 3) % 8
        for dn in (0, 1, -1):
            def sized(s):
                if dn == 1:
                    return s + [int(rng.integers(97, 105))]
                return s[:m - 1] if dn == -1 else s
            for p in EDGES + (m - 2,):   # the block edges, and the string's own last two symbols (m = 31 meets only those)
                if p + 1 < m:
                    s = list(base)
                    s[p], s[p + 1] = s[p + 1], s[p]
                    cases.append((m, "swap %d|%d" % (p, p + 1), bytes(base), bytes(sized(s))))
                q = min(p, m - 3)   # (the last symbols: the triple ends where the string does)
                if (p + 2 < m or p == m - 2) and q >= 0:   # abc -> cab: two swaps side by side, cost 2
                    s = list(base)
                    s[q:q + 3] = [s[q + 2], s[q], s[q + 1]]
                    cases.append((m, "double %d" % q, bytes(base), bytes(sized(s))))
                if p + 1 < m:
                    s = list(base)   # a swap next to an insertion
                    s[p], s[p + 1] = s[p + 1], s[p]
                    s.insert(p + 2, int(rng.integers(97, 105)))
                    cases.append((m, "swap+insert %d" % p, bytes(base), bytes(sized(s))))
    return cases


@pytest.mark.gpu
def test_block_edges(sw, orc, scope, lev):
    cases = block_edge_cases()
    a, b = [c[2] for c in cases], [c[3] for c in cases]
    assert {len(x) for x in a} == set(BLOCK_M) and all(len(y) - len(x) in (-1, 0, 1, 2) for x, y in zip(a, b))
    want = reference_osa(a, b, chunk=24)
    lev_d = np.asarray(orc.levenshtein_pairs(sw.Strs(a), sw.Strs(b), algo="wf")).astype(np.int64)
    for p in EDGES:   # a kernel that drops the transposition at this edge (inside a block or between two) cannot pass
        at = [k for k, c in enumerate(cases) if c[1] == "swap %d|%d" % (p, p + 1)]
        assert at and any(want[k] < lev_d[k] for k in at), p
    forward = lev.osa(sw.Strs(a), sw.Strs(b), scope)     # a is the shorter string, or they tie
    backward = lev.osa(sw.Strs(b), sw.Strs(a), scope)    # b is
    for got in (forward, backward):
        wrong = np.nonzero(got.astype(np.int64) != want)[0]
        assert not len(wrong), [(cases[k][0], cases[k][1], len(b[k]), int(got[k]), int(want[k])) for k in wrong[:5]]


@pytest.mark.gpu
def test_mixed_items(sw, scope, lev):
    """Consecutive pairs of changing block counts share work items (idle lanes past the shorter strings); per-pair results do not
    depend on which pairs are neighbours."""
    rng = np.random.default_rng(53)
    a, b = [], []
    for i in range(400):
        m = (20, 90, 2048, 0, 40, 33, 64, 1, 700, 0)[i % 10] if i < 40 else (5, 70, 0, 33, 200, 1)[i % 6]
        x = rand_bytes(rng, m, 4)
        kind = i % 4
        if kind == 0:
            y = x                                         # identical
        elif kind == 1:
            y = bytes(mutated(rng, x, int(rng.integers(1, 6)), lambda: int(rng.integers(97, 101))))
        elif kind == 2:
            y = rand_bytes(rng, rng.integers(0, 120), 4)
        else:
            y = b""                                       # against empty (and empty against empty)
        if i % 8 >= 4:
            x, y = y, x
        a.append(x); b.append(y)
    a += [b"b", b"a" * 2500 + b"b" + b"a" * 2499, b"x"]
    b += [b"a" * 2500 + b"b" + b"a" * 2499, b"b", rand_bytes(rng, 5000, 4)]   # one symbol against 5 000
    assert any(not x and not y for x, y in zip(a, b)) and any(x and x == y for x, y in zip(a, b))
    want = reference_osa(a, b, chunk=32)
    assert want[-3] == 4999 and want[-2] == 4999 and want[-1] == 5000
    got = lev.osa(sw.Strs(a), sw.Strs(b), scope)
    wrong = np.nonzero(got.astype(np.int64) != want)[0]
    assert not len(wrong), [(int(k), len(a[k]), len(b[k]), int(got[k]), int(want[k])) for k in wrong[:5]]
    order = rng.permutation(len(a))
    again = lev.osa(sw.Strs([a[k] for k in order]), sw.Strs([b[k] for k in order]), scope)
    assert (again == got[order]).all()


@pytest.mark.gpu
def test_bounds(sw, scope, lev):
    rng = np.random.default_rng(54)
    a = [rand_bytes(rng, rng.integers(1, 150), 6) for _ in range(600)]
    b = [bytes(mutated(rng, x, k % 12, lambda: int(rng.integers(97, 103)))) for k, x in enumerate(a)]
    want = reference_osa(a, b)
    assert set(range(8)) <= set(want.tolist())
    sa, sb = sw.Strs(a), sw.Strs(b)
    assert (lev.osa(sa, sb, scope).astype(np.int64) == want).all()
    for bound in (0, 1, 2, 3, 5, 9, 1000):
        got = lev.osa(sa, sb, scope, bound=bound).astype(np.int64)
        assert (got == np.minimum(want, bound + 1)).all(), bound
    # every pair at its own d - 1, d, d + 1: bound + 1, d, d
    for d in sorted(set(want.tolist()))[:8]:
        at = np.nonzero(want == d)[0]
        sub = lambda s: sw.Strs([s[k] for k in at])
        for bound, value in ((d - 1, d), (d, d), (d + 1, d)):
            if bound >= 0:
                assert (lev.osa(sub(a), sub(b), scope, bound=bound) == value).all(), (d, bound)


@pytest.mark.gpu
def test_forms_and_scopes(sw, scope, lev):
    import torch
    from stringwars_amd import _native as N
    rng = np.random.default_rng(55)
    a = [rand_bytes(rng, rng.integers(0, 300), 4) for _ in range(700)]
    b = [bytes(mutated(rng, x, int(rng.integers(0, 9)), lambda: int(rng.integers(97, 101)))) if k % 2 else rand_bytes(rng, rng.integers(0, 300), 4)
         for k, x in enumerate(a)]
    sa, sb = sw.Strs(a), sw.Strs(b)
    assert sa.offsets[-1] != sb.offsets[-1]
    truth = reference_osa(a, b)
    want = lev.osa(sa, sb, scope, bound=20)
    assert (want.astype(np.int64) == np.minimum(truth, 21)).all() and (want == 21).any() and (want < 21).any()
    # device output; a strided host output and a strided device output (the gaps stay as they were)
    out = torch.full((700,), 77, dtype=torch.int32, device="cuda")
    status, message = raw_pairs(sw, lev, scope, sa, sb, out.data_ptr(), bound=20)
    assert status == "success", message
    assert (out.cpu().numpy().astype(np.uint32) == want).all()
    wide = np.full((700, 3), 77, np.uint32)
    assert lev.osa(sa, sb, scope, bound=20, out=wide[:, 1]) is not None
    assert (wide[:, 1] == want).all() and (wide[:, 0] == 77).all() and (wide[:, 2] == 77).all()
    wide_d = torch.full((700, 3), 77, dtype=torch.int32, device="cuda")
    status, message = raw_pairs(sw, lev, scope, sa, sb, wide_d.data_ptr() + 4, bound=20, stride=12)
    assert status == "success", message
    back = wide_d.cpu().numpy().astype(np.uint32)
    assert (back[:, 1] == want).all() and (back[:, 0] == 77).all() and (back[:, 2] == 77).all()
    # raw device tapes; prepared tapes in all four offset-width mixes, whole and as sub-views
    assert (lev.osa(sa.to_device(scope), sb.to_device(scope), scope, bound=20) == want).all()
    da, db = sa.with_offsets(np.uint64).to_device(scope), sb.with_offsets(np.uint64).to_device(scope)
    host = np.full(700, 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, da, db, host.ctypes.data, bound=20)
    assert status == "success" and (host == want).all(), message
    tapes = {(w, name): sw.PreparedTape(scope, sw.Strs(items).with_offsets(w)) for w in (np.uint32, np.uint64)
             for name, items in (("a", a), ("b", b))}
    for wa, wb in itertools.product((np.uint32, np.uint64), repeat=2):
        pa, pb = tapes[(wa, "a")], tapes[(wb, "b")]
        assert (lev.osa(pa, pb, scope, bound=20) == want).all(), (wa, wb)
        assert (lev.osa(pa[37:333], pb[37:333], scope, bound=20) == want[37:333]).all(), (wa, wb)
        on_device = torch.zeros(296, dtype=torch.int32, device="cuda")
        lev.osa(pa[37:333], pb[37:333], scope, bound=20, out=on_device)
        assert (on_device.cpu().numpy().astype(np.uint32) == want[37:333]).all()
    # tapes of two kinds: refused by the C ABI, nothing written
    as_utf8 = sw.PreparedTape(scope, sb, utf8=True)
    va, vb, err = tapes[(np.uint64, "a")].view(), as_utf8.view(), C.c_char_p()
    untouched = np.full(700, 77, np.uint32)
    status = N.lib.swh_levenshtein_osa_pairs_prepared(lev._handle, scope.handle, C.byref(va), C.byref(vb), N.UNBOUNDED,
                                                      C.c_void_p(untouched.ctypes.data), 0, C.byref(err))
    assert N.STATUS_NAMES[status] == "invalid_argument" and (untouched == 77).all()
    # a caller-stream scope -- synchronous, then asynchronous, then pipelined: the results are visible when the call returns
    other = sw.DeviceScope(gpu_device=0, stream=torch.cuda.current_stream().cuda_stream)
    engine = sw.LevenshteinDistances(capabilities=other)
    assert (engine.osa(sa, sb, other, bound=20) == want).all()
    for mode in ("async", "pipelined"):
        if mode == "async":
            other.set_async(True)
        else:
            other.set_async(False)
            other.set_pipelined(True)
        engine.pairs(sa, sb, other)   # outstanding work the call joins
        assert (engine.osa(sa, sb, other, bound=20) == want).all(), mode
        other.synchronize()
    # count == 0: success, nothing written
    assert len(lev.osa(sw.Strs([]), sw.Strs([]), scope)) == 0
    untouched = np.full(4, 77, np.uint32)
    status, _ = raw_pairs(sw, lev, scope, sw.Strs([]), sw.Strs([]), untouched.ctypes.data)
    assert status == "success" and (untouched == 77).all()
    assert lev.osa_cross(sw.Strs([]), sw.Strs([b"a"]), scope).shape == (0, 1)
    # profiling describes the whole call
    scope.set_profiling(True)
    try:
        lev.osa(sa, sb, scope)
        timing = scope.last_timing()
        lev.osa_cross(sa[:60], sb[:50], scope)
        cross_timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["cells"] == int((sa.lengths * sb.lengths).sum())
    assert timing["dominant_name"] == "osa" and timing["kernels"] == 2
    assert cross_timing["cells"] == int(sa.lengths[:60].sum()) * int(sb.lengths[:50].sum()) and cross_timing["dominant_name"] == "osa"


def golden_strings(name, sides):
    z = np.load(os.path.join(GOLDEN, name))
    out = []
    for side in sides:
        data, offsets = z[side + "_data"], z[side + "_offsets"].astype(np.int64)
        out.append([bytes(data[offsets[i]:offsets[i + 1]]).decode("utf-8") for i in range(len(offsets) - 1)])
    return out


@pytest.mark.gpu
def test_utf8(sw, scope, lev, lev8):
    rng = np.random.default_rng(56)
    lines_a, lines_b = golden_strings("script_lines.npz", "ab")
    queries, candidates = golden_strings("uwords.npz", "qc")
    a, b = list(lines_a), list(lines_b)
    for line in lines_a:   # every line against a copy with neighbours swapped
        s = list(line)
        for _ in range(4):
            at = int(rng.integers(0, max(len(s) - 1, 1)))
            if at + 1 < len(s):
                s[at], s[at + 1] = s[at + 1], s[at]
        a.append(line); b.append("".join(s))
    count = min(len(queries), len(candidates))
    a += queries[:count]; b += candidates[:count]
    # mixed 1- to 4-byte sequences
    mixed = [0x61, 0x62, 0xE9, 0x3B1, 0x4E2D, 0x6587, 0x1F600, 0x10FFFF, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000]
    for i in range(300):
        x = [int(rng.choice(mixed)) for _ in range(int(rng.integers(0, 100)))]
        y = mutated(rng, x, int(rng.integers(0, 6)), lambda: int(rng.choice(mixed)))
        a.append("".join(map(chr, x))); b.append("".join(map(chr, y)))
    # byte OSA and code-point OSA differ: two 2-byte letters swapped are one edit in code points, two in bytes
    a.append("éè"); b.append("èé")
    assert any(len(x.encode()) > len(x) for x in a)
    want = reference_osa(a, b, utf8=True)
    got = lev8.osa(sw.Strs(a), sw.Strs(b), scope)
    wrong = np.nonzero(got.astype(np.int64) != want)[0]
    assert not len(wrong), [(int(k), int(got[k]), int(want[k])) for k in wrong[:5]]
    assert got[-1] == 1 and lev.osa(sw.Strs(a[-1:]), sw.Strs(b[-1:]), scope)[0] == 2 == reference_osa(a[-1:], b[-1:])[0]
    prepared = lev8.osa(sw.PreparedTape(scope, sw.Strs(a), utf8=True), sw.PreparedTape(scope, sw.Strs(b), utf8=True), scope)
    assert (prepared == got).all()
    some = slice(0, 40)
    matrix = lev8.osa_cross(sw.Strs(a[some]), sw.Strs(b[some]), scope)
    assert (np.diagonal(matrix).astype(np.int64) == want[some]).all()
    scope.set_profiling(True)
    try:
        lev8.osa(sw.Strs(a), sw.Strs(b), scope)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["dominant_name"] == "osa_u32" and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    # invalid UTF-8 in either tape: the status, and the outputs untouched
    out, matrix = np.full(2, 77, np.uint32), np.full((2, 2), 77, np.uint64)
    for bad_a, bad_b in (([b"ok", b"\xff\xfe"], [b"ok", b"x"]), ([b"ok", b"x"], [b"ok", b"\xc3"])):
        status, _ = raw_pairs(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), out.ctypes.data, utf8=True)
        assert status == "invalid_utf8" and (out == 77).all()
        status, _ = raw_cross(sw, lev8, scope, sw.Strs(bad_a), sw.Strs(bad_b), matrix.ctypes.data, utf8=True)
        assert status == "invalid_utf8" and (matrix == 77).all()


def cross_batch():
    rng = np.random.default_rng(57)
    queries = [rand_bytes(rng, rng.integers(0, 90), 4) for _ in range(50)]
    candidates = [bytes(mutated(rng, queries[k % 50], int(rng.integers(0, 5)), lambda: int(rng.integers(97, 101)))) for k in range(37)]
    return queries, candidates


def expanded(queries, candidates):
    return [q for q in queries for _ in candidates], [c for _ in queries for c in candidates]


@pytest.mark.gpu
def test_cross(sw, scope, lev):
    import torch
    queries, candidates = cross_batch()
    sq, sc = sw.Strs(queries), sw.Strs(candidates)
    a, b = expanded(queries, candidates)
    as_pairs = lev.osa(sw.Strs(a), sw.Strs(b), scope).reshape(50, 37)
    assert (as_pairs.astype(np.int64).ravel() == reference_osa(a, b)).all()
    matrix = lev.osa_cross(sq, sc, scope)
    assert matrix.dtype == np.uint64 and (matrix == as_pairs).all()
    # a row stride, on the host and on the device: the columns past the matrix stay as they were
    wide = np.full((50, 40), 77, np.uint64)
    lev.osa_cross(sq, sc, scope, out=wide[:, :37])
    assert (wide[:, :37] == as_pairs).all() and (wide[:, 37:] == 77).all()
    wide_d = torch.full((50, 40), 77, dtype=torch.int64, device="cuda")
    status, message = raw_cross(sw, lev, scope, sq, sc, wide_d.data_ptr(), stride=320)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert (back[:, :37] == as_pairs).all() and (back[:, 37:] == 77).all()
    # device and prepared tapes
    assert (lev.osa_cross(sq.to_device(scope), sc.to_device(scope), scope) == as_pairs).all()
    pq, pc = sw.PreparedTape(scope, sq.with_offsets(np.uint32)), sw.PreparedTape(scope, sc.with_offsets(np.uint64))
    assert (lev.osa_cross(pq, pc, scope) == as_pairs).all()
    assert (lev.osa_cross(pq[5:30], pc[3:], scope) == as_pairs[5:30, 3:]).all()
    # b == NULL: the self-product, symmetric with a zero diagonal
    own = np.full((50, 50), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sq, None, own.ctypes.data)
    assert status == "success", message
    assert (own == own.T).all() and (np.diagonal(own) == 0).all()
    a, b = expanded(queries, queries)
    assert (own.astype(np.int64).ravel() == reference_osa(a, b)).all()
    assert (lev.osa_cross(sq, None, scope) == own).all() and (lev.osa_cross(pq, None, scope) == own).all()


@pytest.mark.gpu
def test_cross_in_many_chunks(request, sw):
    """STRINGWARS_AMD_OSA_CHUNK_PAIRS (test library) shrinks the slices of whole rows to 96 pairs, so a 50 x 37 product runs as 25
    slices of two rows, with the same results on the host and on the device."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_OSA_CHUNK_PAIRS="96"), test_library=True):
        return
    import torch
    scope = sw.DeviceScope(gpu_device=0)
    lev = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = cross_batch()
    a, b = expanded(queries, candidates)
    want = reference_osa(a, b).reshape(50, 37)
    scope.set_profiling(True)
    matrix = lev.osa_cross(sw.Strs(queries), sw.Strs(candidates), scope)
    timing = scope.last_timing()
    scope.set_profiling(False)
    assert (matrix.astype(np.int64) == want).all()
    assert timing["kernels"] == 1 + 2 * 25 and timing["cells"] == sum(len(x) * len(y) for x, y in zip(a, b))
    wide_d = torch.full((50, 40), 77, dtype=torch.int64, device="cuda")
    status, message = raw_cross(sw, lev, scope, sw.Strs(queries), sw.Strs(candidates), wide_d.data_ptr(), stride=320)
    assert status == "success", message
    back = wide_d.cpu().numpy()
    assert (back[:, :37] == want).all() and (back[:, 37:] == 77).all()
    # a refusal still comes before the first row is written
    long_q = [b"ab"] * 60 + [b"a" * 2049]
    long_c = [b"ab", b"b" * 2049, b"c" * 3000]
    untouched = np.full((61, 3), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sw.Strs(long_q), sw.Strs(long_c), untouched.ctypes.data)
    assert status == "unsupported_length" and "pair (60, 1)" in message and (untouched == 77).all(), message


@pytest.mark.gpu
def test_refusals(sw, scope, lev):
    rng = np.random.default_rng(58)
    a = [b"abc", rand_bytes(rng, 2048, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 3000, 4)]
    b = [b"acb", rand_bytes(rng, 2048, 4), rand_bytes(rng, 5, 4), rand_bytes(rng, 2049, 4), rand_bytes(rng, 4000, 4)]
    out = np.full(5, 77, np.uint32)
    status, message = raw_pairs(sw, lev, scope, sw.Strs(a), sw.Strs(b), out.ctypes.data)
    assert status == "unsupported_length" and "pair 3" in message and "2049" in message, message
    assert (out == 77).all()
    with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
        lev.osa(sw.Strs(a), sw.Strs(b), scope)
    assert "pair 3" in str(info.value)
    matrix = np.full((5, 5), 77, np.uint64)
    status, message = raw_cross(sw, lev, scope, sw.Strs(a), sw.Strs(b), matrix.ctypes.data)
    assert status == "unsupported_length" and "pair (2, 3)" in message and (matrix == 77).all(), message
    got = lev.osa(sw.Strs(a[:3]), sw.Strs(b[:3]), scope)   # 2048 x 2048 and 2049 x 5 are accepted
    assert (got.astype(np.int64) == reference_osa(a[:3], b[:3])).all() and got[0] == 1
    # count mismatch
    status, _ = raw_pairs(sw, lev, scope, sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), out.ctypes.data)
    assert status == "invalid_argument" and (out == 77).all()
    with pytest.raises(ValueError):
        lev.osa(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope)
    # a general-cost engine
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    with pytest.raises(sw.StringWarsError, match="not_implemented"):
        costly.osa(sw.Strs([b"ab"]), sw.Strs([b"ba"]), scope)
    with pytest.raises(sw.StringWarsError, match="not_implemented"):
        costly.osa_cross(sw.Strs([b"ab"]), sw.Strs([b"ba"]), scope)


@pytest.mark.gpu
def test_seeded_random_round(sw, scope, lev):
    rng = np.random.default_rng(2028)
    count = 3000
    alphabets = np.array([2, 4, 26])[rng.integers(0, 3, size=count)]
    lengths, edits, related = rng.integers(0, 301, size=count), rng.integers(0, 12, size=count), rng.integers(0, 4, size=count)
    a, b = [], []
    for i in range(count):
        alphabet = int(alphabets[i])
        x = rand_bytes(rng, lengths[i], alphabet)
        if related[i]:
            y = bytes(mutated(rng, x, int(edits[i]), lambda: int(rng.integers(97, 97 + alphabet))))
        else:
            y = rand_bytes(rng, rng.integers(0, 301), alphabet)
        if i % 2:
            x, y = y, x
        a.append(x); b.append(y)
    want = reference_osa(a, b)
    # every random number is drawn and the reference is computed: the device comes now
    got = lev.osa(sw.Strs(a), sw.Strs(b), scope)
    wrong = np.nonzero(got.astype(np.int64) != want)[0]
    assert not len(wrong), [(int(k), len(a[k]), len(b[k]), int(got[k]), int(want[k])) for k in wrong[:5]]
    plain = lev.pairs(sw.Strs(a), sw.Strs(b), scope).astype(np.int64)
    assert (want <= plain).all() and (plain <= 2 * want).all() and (want < plain).sum() >= 100
