"""Levenshtein alignments (swh_levenshtein_align_*): the canonical edit script of every pair.

The reference script is computed here with numpy: the full Wagner-Fischer matrix row by row (diagonal and deletion terms in one
step, the insertion term as `minimum.accumulate(t - arange) + arange`), then the walk back from (m, n) with the rule of the C ABI:
'=' on equal symbols, else 'X' if the diagonal is optimal, else 'D' if the cell above is, else 'I'."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def symbols(s, utf8=False) -> np.ndarray:
    if isinstance(s, str):
        return np.array([ord(c) for c in s], dtype=np.int64) if utf8 else np.frombuffer(s.encode(), dtype=np.uint8).astype(np.int64)
    return np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64)


def wagner_fischer(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    m, n = len(a), len(b)
    d = np.empty((m + 1, n + 1), dtype=np.int32)
    ar = np.arange(n + 1, dtype=np.int32)
    d[0] = ar
    t = np.empty(n + 1, dtype=np.int32)
    for i in range(1, m + 1):
        prev = d[i - 1]
        t[0] = i
        np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1, out=t[1:])
        d[i] = np.minimum.accumulate(t - ar) + ar
    return d


def reference_script(a, b, utf8=False):
    """(distance, ops bytes) of the canonical script."""
    a, b = symbols(a, utf8), symbols(b, utf8)
    d = wagner_fischer(a, b)
    i, j, ops = len(a), len(b), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and a[i - 1] == b[j - 1]:
            ops.append(b"="); i -= 1; j -= 1
        elif i > 0 and j > 0 and d[i - 1, j - 1] + 1 == d[i, j]:
            ops.append(b"X"); i -= 1; j -= 1
        elif i > 0 and d[i - 1, j] + 1 == d[i, j]:
            ops.append(b"D"); i -= 1
        else:
            ops.append(b"I"); j -= 1
    return int(d[-1, -1]), b"".join(reversed(ops))


def script_errors(a, b, ops: bytes, distance: int, utf8=False):
    """Why `ops` is not a valid script of cost `distance` from a to b (None: it is)."""
    a, b = symbols(a, utf8), symbols(b, utf8)
    i = j = 0
    for op in ops:
        if op in b"=X":
            if i >= len(a) or j >= len(b) or (a[i] == b[j]) != (op == ord("=")):
                return "bad %c at (%d, %d)" % (op, i, j)
            i += 1; j += 1
        elif op == ord("D"):
            i += 1
        elif op == ord("I"):
            j += 1
        else:
            return "unknown op %r" % op
    if (i, j) != (len(a), len(b)):
        return "script ends at (%d, %d), not (%d, %d)" % (i, j, len(a), len(b))
    if sum(op != ord("=") for op in ops) != distance:
        return "cost %d, not %d" % (sum(op != ord("=") for op in ops), distance)
    return None


EXAMPLES = [("kitten", "sitting", 3, b"X===X=I"), ("flaw", "lawn", 2, b"D===I"), ("aa", "a", 1, b"D="), ("ab", "ba", 2, b"XX"),
            ("", "abc", 3, b"III"), ("abc", "", 3, b"DDD"), ("", "", 0, b"")]


def random_strs(rng, count, lo, hi, alphabet):
    lengths = rng.integers(lo, hi + 1, size=count)
    return [bytes(rng.integers(0, alphabet, size=int(n)).astype(np.uint8)) for n in lengths]


def check_exact(sw, got, a_list, b_list, utf8=False, bound=None, indices=None):
    indices = range(len(a_list)) if indices is None else indices
    for i in indices:
        d, ops = reference_script(a_list[i], b_list[i], utf8)
        if bound is not None and d > bound:
            assert int(got.distances[i]) == bound + 1 and got[i] == b"", i
            continue
        assert int(got.distances[i]) == d and got[i] == ops, (i, a_list[i][:40], b_list[i][:40], got[i][:80], ops[:80])


def check_valid_batch(a, b, got, utf8=False):
    """Vectorised validity of every pair of a batch: op counts against the lengths and the distance, '=' exactly on equal symbols.
    `a` / `b` are Strs (bytes); for utf8 the caller passes code-point arrays instead (see `code_point_tape`)."""
    sa, oa = a
    sb, ob = b
    count = len(got)
    offsets = got.offsets.astype(np.int64)
    lengths = np.diff(offsets)
    seg = np.repeat(np.arange(count), lengths)
    ops = got.ops
    assert len(ops) == offsets[-1]
    is_m, is_x, is_d, is_i = (ops == ord(c) for c in "=XDI")
    assert (is_m | is_x | is_d | is_i).all()
    cnt = lambda mask: np.bincount(seg[mask], minlength=count)
    nm, nx, nd, ni = cnt(is_m), cnt(is_x), cnt(is_d), cnt(is_i)
    la, lb = np.diff(oa.astype(np.int64)), np.diff(ob.astype(np.int64))
    assert (nm + nx + nd == la).all() and (nm + nx + ni == lb).all()
    assert (nx + nd + ni == got.distances.astype(np.int64)).all()
    # symbol positions of every op: segmented cumulative sums of the symbols each op consumes
    ca = (is_m | is_x | is_d).astype(np.int64)
    cb = (is_m | is_x | is_i).astype(np.int64)
    pa = np.cumsum(ca) - ca
    pb = np.cumsum(cb) - cb
    starts = offsets[:-1]
    pa -= np.repeat(np.where(lengths > 0, pa[np.minimum(starts, len(ops) - 1)] if len(ops) else 0, 0), lengths)
    pb -= np.repeat(np.where(lengths > 0, pb[np.minimum(starts, len(ops) - 1)] if len(ops) else 0, 0), lengths)
    both = is_m | is_x
    xa = sa[oa.astype(np.int64)[seg[both]] + pa[both]]
    xb = sb[ob.astype(np.int64)[seg[both]] + pb[both]]
    assert ((xa == xb) == is_m[both]).all()


def code_point_tape(strings):
    cps = [np.array([ord(c) for c in s], dtype=np.int64) for s in strings]
    offsets = np.zeros(len(cps) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cps], out=offsets[1:])
    return (np.concatenate(cps) if cps else np.zeros(0, np.int64)), offsets


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in ("swh_levenshtein_align_u64tape", "swh_levenshtein_utf8_align_u64tape", "swh_levenshtein_align_prepared"):
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "align" in sw.capabilities().split(",")
    assert callable(sw.LevenshteinDistances.align) and callable(sw.LevenshteinDistancesUTF8.align)
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_ALIGN_MAX_CELLS \(1ull << 30\)", header) and sw.ALIGN_MAX_CELLS == 1 << 30
    for name, value in (("MATCH", N.OP_MATCH), ("SUBST", N.OP_SUBST), ("DEL", N.OP_DEL), ("INS", N.OP_INS)):
        assert re.search(r"#define SWH_OP_%s '%s'" % (name, re.escape(chr(value))), header), name
    assert (N.OP_MATCH, N.OP_SUBST, N.OP_DEL, N.OP_INS) == tuple(map(ord, "=XDI"))


def test_reference_examples_and_validity(orc, sw):
    for a, b, d, ops in EXAMPLES:
        assert reference_script(a, b) == (d, ops), (a, b)
    rng = np.random.default_rng(7)
    for alphabet in (2, 4, 26):
        a = random_strs(rng, 100, 0, 40, alphabet)
        b = random_strs(rng, 100, 0, 40, alphabet)
        want = orc.levenshtein_pairs(sw.Strs(a), sw.Strs(b), algo="wf")
        for i in range(100):
            d, ops = reference_script(a[i], b[i])
            assert d == int(want[i]) and script_errors(a[i], b[i], ops, d) is None


def test_alignments_cigar_and_editops(sw):
    ops = b"X===X=I" + b"D===I" + b""
    got = sw.Alignments(np.array([3, 2, 5], np.uint32), np.array([0, 7, 12, 12], np.uint64), np.frombuffer(ops, np.uint8))
    assert len(got) == 3 and got[0] == b"X===X=I" and got[1] == b"D===I" and got[2] == b"" and got[-1] == b""
    assert got.cigar(0) == "1X3=1X1=1I" and got.cigar(1) == "1D3=1I" and got.cigar(2) == ""
    assert got.editops(0) == [("replace", 0, 0), ("replace", 4, 4), ("insert", 6, 6)]
    assert got.editops(1) == [("delete", 0, 0), ("insert", 4, 3)]
    with pytest.raises(IndexError):
        got[3]


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


@pytest.mark.gpu
def test_examples_and_exhaustive(sw, scope, lev, lev8):
    got = lev.align(sw.Strs([x[0] for x in EXAMPLES]), sw.Strs([x[1] for x in EXAMPLES]), scope)
    for i, (_, _, d, ops) in enumerate(EXAMPLES):
        assert int(got.distances[i]) == d and got[i] == ops, i
    assert got.cigar(0) == "1X3=1X1=1I"
    for alphabet, engine, utf8 in (("ab", lev, False), ("aé", lev8, True)):
        strs = ["".join(p) for n in range(7) for p in itertools.product(alphabet, repeat=n)]
        a = [x for x in strs for _ in strs]
        b = [y for _ in strs for y in strs]
        got = engine.align(sw.Strs(a), sw.Strs(b), scope)
        assert len(got) == len(a) == 127 * 127
        check_exact(sw, got, a, b, utf8=utf8)


@pytest.mark.gpu
def test_random_byte_pairs(sw, scope, lev):
    rng = np.random.default_rng(11)
    a, b = [], []
    for alphabet in (2, 4, 26, 256):
        a += random_strs(rng, 450, 0, 300, alphabet)
        b += random_strs(rng, 450, 0, 300, alphabet)
        for n in (63, 64, 65, 127, 128, 129):   # one route's edge and the 32-row block edges
            a += random_strs(rng, 4, n, n, alphabet)
            b += random_strs(rng, 4, max(0, n - 5), n + 5, alphabet)
    got = lev.align(sw.Strs(a), sw.Strs(b), scope)
    assert (got.distances == lev.pairs(sw.Strs(a), sw.Strs(b), scope)).all()
    check_exact(sw, got, a, b)


@pytest.mark.gpu
def test_long_pairs(sw, scope, lev):
    rng = np.random.default_rng(12)
    a = [bytes(rng.integers(0, 4, size=n).astype(np.uint8)) for n in (2047, 2049, 3000, 5000)]
    b = [x[: len(x) // 2] + bytes(rng.integers(0, 4, size=300).astype(np.uint8)) + x[len(x) // 2 + 100:] for x in a]
    # very unequal lengths, both ways round: the pattern is the longer string, so one orientation runs transposed
    a += [bytes(rng.integers(0, 4, size=5).astype(np.uint8)), bytes(rng.integers(0, 4, size=3000).astype(np.uint8))]
    b += [bytes(rng.integers(0, 4, size=3000).astype(np.uint8)), bytes(rng.integers(0, 4, size=40).astype(np.uint8))]
    got = lev.align(sw.Strs(a), sw.Strs(b), scope)
    check_exact(sw, got, a, b)
    big_a = bytes(rng.integers(0, 26, size=20000).astype(np.uint8) + 97)
    big_b = bytearray(big_a)
    for p in rng.integers(0, 20000, size=2000):
        big_b[p] = 97 + int(rng.integers(0, 26))
    big_b = bytes(big_b[:15000]) + bytes(rng.integers(97, 123, size=5000).astype(np.uint8))
    got = lev.align(sw.Strs([big_a]), sw.Strs([big_b]), scope)
    assert int(got.distances[0]) == int(lev.pairs(sw.Strs([big_a]), sw.Strs([big_b]), scope)[0])
    assert script_errors(big_a, big_b, got[0], int(got.distances[0])) is None


@pytest.mark.gpu
def test_c2_batch(sw, scope, lev):
    a, b = sw.generate_pairs("tokens64", 1_000_000, seed=5)
    got = lev.align(a, b, scope)
    assert (got.distances == lev.pairs(a, b, scope)).all()
    check_valid_batch((a.data, a.offsets), (b.data, b.offsets), got)
    sample = range(0, len(a), len(a) // 2000)
    al = {i: bytes(a.data[int(a.offsets[i]):int(a.offsets[i + 1])]) for i in sample}
    bl = {i: bytes(b.data[int(b.offsets[i]):int(b.offsets[i + 1])]) for i in sample}
    check_exact(sw, got, al, bl, indices=sample)


@pytest.mark.gpu
def test_utf8_batch(sw, scope, lev8):
    a, b = sw.generate_pairs("utf8_lines", 2000, seed=6)
    got = lev8.align(a, b, scope)
    assert (got.distances == lev8.pairs(a, b, scope)).all()
    sa = [bytes(a.data[int(a.offsets[i]):int(a.offsets[i + 1])]).decode() for i in range(len(a))]
    sb = [bytes(b.data[int(b.offsets[i]):int(b.offsets[i + 1])]).decode() for i in range(len(b))]
    check_valid_batch(code_point_tape(sa), code_point_tape(sb), got, utf8=True)
    check_exact(sw, got, sa, sb, utf8=True, indices=range(0, len(sa), 100))
    with pytest.raises(sw.StringWarsError, match="invalid_utf8"):
        lev8.align(sw.Strs([b"ok", b"\xff\xfe"]), sw.Strs([b"ok", b"x"]), scope)


@pytest.mark.gpu
def test_bounds(sw, scope, lev):
    rng = np.random.default_rng(13)
    a = random_strs(rng, 600, 0, 80, 4)
    b = [x[: len(x) // 2] + bytes(rng.integers(0, 4, size=int(rng.integers(0, 30))).astype(np.uint8)) for x in a]
    b[::10] = a[::10]   # some pairs within every bound
    b[1::10] = [x[:-2] for x in a[1::10]]
    for bound in (0, 3, 32):
        got = lev.align(sw.Strs(a), sw.Strs(b), scope, bound=bound)
        assert (got.distances == lev.pairs(sw.Strs(a), sw.Strs(b), scope, bound=bound)).all()
        assert (got.distances > bound).any() and (got.distances <= bound).any()
        check_exact(sw, got, a, b, bound=bound)


@pytest.mark.gpu
def test_edge_cases(sw, scope, lev):
    from stringwars_amd import _native as N
    got = lev.align(sw.Strs([]), sw.Strs([]), scope)
    assert len(got) == 0 and list(got.offsets) == [0]
    a, b = [b"", b"abc", b"", b"same", b"x" * 70], [b"xyz", b"", b"", b"same", b"x" * 70]
    got = lev.align(sw.Strs(a), sw.Strs(b), scope)
    assert [got[i] for i in range(5)] == [b"III", b"DDD", b"", b"====", b"=" * 70] and list(got.distances) == [3, 3, 0, 0, 0]
    # ops_capacity one short: invalid_argument, nothing written
    ta, tb = sw.Strs([b"kitten", b"ab"]), sw.Strs([b"sitting", b"ba"])
    ca, _, ka = sw.engines._c_tape(ta, want64=True)
    cb, _, kb = sw.engines._c_tape(tb, want64=True)
    dist = np.full(2, 77, np.uint32); offs = np.full(3, 77, np.uint64); ops = np.full(64, 77, np.uint8)
    err = C.c_char_p()
    status = N.lib.swh_levenshtein_align_u64tape(lev._handle, scope.handle, C.byref(ca), C.byref(cb), N.UNBOUNDED, C.c_void_p(dist.ctypes.data),
                                                 C.c_void_p(offs.ctypes.data), C.c_void_p(ops.ctypes.data), 16, C.byref(err))
    assert N.STATUS_NAMES[status] == "invalid_argument" and (dist == 77).all() and (offs == 77).all() and (ops == 77).all()
    status = N.lib.swh_levenshtein_align_u64tape(lev._handle, scope.handle, C.byref(ca), C.byref(cb), N.UNBOUNDED, C.c_void_p(dist.ctypes.data),
                                                 C.c_void_p(offs.ctypes.data), C.c_void_p(ops.ctypes.data), 17, C.byref(err))
    assert status == 0 and list(offs) == [0, 7, 9] and ops[:9].tobytes() == b"X===X=IXX"
    # a pair over SWH_ALIGN_MAX_CELLS: unsupported_length, named, nothing written
    big = sw.Strs([b"a", b"x" * 40000]), sw.Strs([b"b", b"y" * 30000])
    with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
        lev.align(big[0], big[1], scope)
    assert "pair 1" in str(info.value)
    # non-unit costs: not implemented
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    with pytest.raises(sw.StringWarsError, match="not_implemented"):
        costly.align(ta, tb, scope)
    with pytest.raises(ValueError):
        lev.align(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope)


@pytest.mark.gpu
def test_forms_and_scopes(sw, scope, lev):
    import torch
    a, b = sw.generate_pairs("short_words", 5000, seed=9)
    want = lev.align(a, b, scope)
    again = lev.align(a, b, scope)
    assert (want.distances == again.distances).all() and (want.offsets == again.offsets).all() and want.ops.tobytes() == again.ops.tobytes()
    pa, pb = sw.PreparedTape(scope, a), sw.PreparedTape(scope, b)
    got = lev.align(pa, pb, scope)
    assert (got.distances == want.distances).all() and (got.offsets == want.offsets).all() and (got.ops == want.ops).all()
    sub = lev.align(pa[1000:3000], pb[1000:3000], scope)
    assert [sub[i] for i in range(0, 2000, 37)] == [want[1000 + i] for i in range(0, 2000, 37)]
    assert (sub.distances == want.distances[1000:3000]).all()
    # device outputs (torch tensors) equal host outputs
    from stringwars_amd import _native as N
    ca, _, ka = sw.engines._c_tape(a, want64=True)
    cb, _, kb = sw.engines._c_tape(b, want64=True)
    capacity = len(a.data) + len(b.data)
    dist = torch.zeros(len(a), dtype=torch.int32, device="cuda")
    offs = torch.zeros(len(a) + 1, dtype=torch.int64, device="cuda")
    ops = torch.zeros(capacity, dtype=torch.uint8, device="cuda")
    err = C.c_char_p()
    status = N.lib.swh_levenshtein_align_u64tape(lev._handle, scope.handle, C.byref(ca), C.byref(cb), N.UNBOUNDED, C.c_void_p(dist.data_ptr()),
                                                 C.c_void_p(offs.data_ptr()), C.c_void_p(ops.data_ptr()), capacity, C.byref(err))
    assert status == 0, err.value
    assert (dist.cpu().numpy().astype(np.uint32) == want.distances).all() and (offs.cpu().numpy().astype(np.uint64) == want.offsets).all()
    assert ops.cpu().numpy()[:len(want.ops)].tobytes() == want.ops.tobytes()
    # asynchronous and pipelined scopes: the results are visible when the call returns
    for mode in ("async", "pipelined"):
        other = sw.DeviceScope(gpu_device=0)
        engine = sw.LevenshteinDistances(capabilities=other)
        if mode == "async":
            other.set_async(True)
        else:
            other.set_pipelined(True)
        engine.pairs(a, b, other)   # outstanding work the call joins
        got = engine.align(a, b, other)
        assert (got.distances == want.distances).all() and got.ops.tobytes() == want.ops.tobytes(), mode
        other.synchronize()


@pytest.mark.gpu
def test_profiling_reports_the_call(sw, scope, lev):
    a, b = sw.generate_pairs("tokens64", 20000, seed=3)
    scope.set_profiling(True)
    try:
        lev.align(a, b, scope)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    la, lb = np.diff(a.offsets.astype(np.int64)), np.diff(b.offsets.astype(np.int64))
    assert timing["cells"] == int((la * lb).sum())
    assert timing["dominant_name"] == "align" and timing["kernels"] >= 5   # k_align, not the sizing, scans or emit


@pytest.mark.gpu
def test_seeded_sweep(sw, scope, lev, lev8):
    rng = np.random.default_rng(2026)
    parts = []
    for workload, count in (("short_words", 100_000), ("tokens64", 80_000), ("protein4k", 8)):
        a, b = sw.generate_pairs(workload, count, seed=int(rng.integers(1 << 30)))
        got = lev.align(a, b, scope)
        assert (got.distances == lev.pairs(a, b, scope)).all(), workload
        check_valid_batch((a.data, a.offsets), (b.data, b.offsets), got)
        parts.append(len(got))
    a, b = sw.generate_pairs("utf8_lines", 400, seed=int(rng.integers(1 << 30)))
    got = lev8.align(a, b, scope, bound=200)
    assert (got.distances == lev8.pairs(a, b, scope, bound=200)).all()
    assert sum(parts) + 400 >= 180_000


@pytest.mark.gpu
def test_many_chunks(request, sw, orc):
    """STRINGWARS_AMD_ALIGN_CHUNK_KB (test library) shrinks the chunks of consecutive pairs to a few KB of stored vectors, so that a
    small batch runs as many chunks -- among them ones of a single pair larger than the target -- with the same results."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_ALIGN_CHUNK_KB="4"), test_library=True):
        return
    scope = sw.DeviceScope(gpu_device=0)
    lev = sw.LevenshteinDistances(capabilities=scope)
    rng = np.random.default_rng(21)
    a = random_strs(rng, 700, 0, 120, 4) + random_strs(rng, 3, 600, 700, 4)
    b = random_strs(rng, 700, 0, 120, 4) + random_strs(rng, 3, 500, 700, 4)
    order = rng.permutation(len(a))
    a, b = [a[i] for i in order], [b[i] for i in order]
    scope.set_profiling(True)
    got = lev.align(sw.Strs(a), sw.Strs(b), scope)
    kernels = scope.last_timing()["kernels"]
    scope.set_profiling(False)
    assert kernels > 50   # sizes + 2 scans + the chunks + 1 scan + emit
    assert (got.distances == lev.pairs(sw.Strs(a), sw.Strs(b), scope)).all()
    check_exact(sw, got, a, b)


# ---- adversarial cases: offset widths, bounds across blocks, code-point groups, scan edges, the cell limit ----------------------------
def mutated(rng, s, edits, draw):
    """`s` (a list of symbols) after `edits` random substitutions, insertions and deletions with symbols from `draw()`."""
    s = list(s)
    for _ in range(edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(0, max(len(s), 1)))
        if op == 0 and s:
            s[at] = draw()
        elif op == 1:
            s.insert(at, draw())
        elif s:
            del s[at]
    return s


def same_alignments(got, want):
    return (got.distances == want.distances).all() and (got.offsets == want.offsets).all() and got.ops.tobytes() == want.ops.tobytes()


@pytest.mark.gpu
def test_offset_widths(sw, scope, lev):
    """k_align<uint8_t, OffA, OffB>: prepared tapes with 32- and 64-bit offsets in all four combinations, byte for byte the all-64-bit
    result (which is checked against the reference script), whole tapes and sub-views."""
    rng = np.random.default_rng(31)
    a = random_strs(rng, 400, 0, 300, 4)
    b = [bytes(mutated(rng, x, int(rng.integers(0, 12)), lambda: int(rng.integers(0, 4)))) for x in a[:250]] + random_strs(rng, 150, 0, 300, 4)
    a[0], b[0], a[-1], b[-1] = b"", b"", bytes(300), bytes(299)
    # the two tapes differ in size and in where their strings start, so an offset read from the wrong tape or at the wrong width shows
    assert sum(map(len, a)) != sum(map(len, b)) and max(map(len, a + b)) >= 300 and min(map(len, a + b)) == 0
    tapes = {(w, name): sw.PreparedTape(scope, sw.Strs(items).with_offsets(w)) for w in (np.uint32, np.uint64) for name, items in (("a", a), ("b", b))}
    want = lev.align(tapes[(np.uint64, "a")], tapes[(np.uint64, "b")], scope)
    check_exact(sw, want, a, b)
    assert same_alignments(lev.align(sw.Strs(a), sw.Strs(b), scope), want)
    for wa, wb in itertools.product((np.uint32, np.uint64), repeat=2):
        pa, pb = tapes[(wa, "a")], tapes[(wb, "b")]
        assert same_alignments(lev.align(pa, pb, scope), want), (wa, wb)
        sub = lev.align(pa[37:333], pb[37:333], scope, bound=25)
        bounded = lev.align(tapes[(np.uint64, "a")][37:333], tapes[(np.uint64, "b")][37:333], scope, bound=25)
        assert same_alignments(sub, bounded), (wa, wb)
        assert all(sub[i] == (want[37 + i] if want.distances[37 + i] <= 25 else b"") for i in range(296)), (wa, wb)


BLOCK_LENGTHS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 129, 300, 1000)   # around the edges of the pattern's 32-row blocks, and many blocks


@pytest.mark.gpu
def test_bounds_across_blocks(sw, scope, lev):
    """Every pair of lengths around the 32-row block edges, both ways round (the pattern is the longer string: one orientation runs
    transposed), related pairs a known number of edits apart and unrelated ones, under bounds that fall below the length difference
    (the early exit), between it and the distance (the exit after the forward pass), and above the distance (the script)."""
    rng = np.random.default_rng(32)
    a, b, edits_of = [], [], []
    for la in BLOCK_LENGTHS:
        for lb in BLOCK_LENGTHS:
            base = rng.integers(97, 123, max(la, lb)).astype(np.uint8)
            for edits in (0, 1, 5, 40):   # substitutions at distinct places of the common prefix, on top of the length difference
                y = base[:lb].copy()
                at = rng.choice(min(la, lb), min(edits, la, lb), replace=False)
                y[at] = 97 + (y[at] - 97 + rng.integers(1, 26, len(at))) % 26
                a.append(base[:la].tobytes()); b.append(y.tobytes()); edits_of.append(abs(la - lb) + len(at))
            a.append(bytes(rng.integers(0, 4, la).astype(np.uint8))); b.append(bytes(rng.integers(0, 4, lb).astype(np.uint8))); edits_of.append(None)
    reference = [reference_script(x, y) for x, y in zip(a, b)]
    for (d, _), edits, x, y in zip(reference, edits_of, a, b):
        assert abs(len(x) - len(y)) <= d <= (edits if edits is not None else max(len(x), len(y)))
    # (the edit count is the distance unless the longer string's tail offers the shorter one better matches)
    assert sum(d == e for (d, _), e in zip(reference, edits_of)) > 350
    sa, sb = sw.Strs(a), sw.Strs(b)
    for bound in (0, 1, 5, 40, 200):
        got = lev.align(sa, sb, scope, bound=bound)
        assert (got.distances == lev.pairs(sa, sb, scope, bound=bound)).all(), bound
        by_gap = by_distance = within = 0
        for i, (d, ops) in enumerate(reference):
            if d > bound:
                assert int(got.distances[i]) == bound + 1 and got[i] == b"", (bound, i, len(a[i]), len(b[i]))
                by_gap += abs(len(a[i]) - len(b[i])) > bound
                by_distance += abs(len(a[i]) - len(b[i])) <= bound
            else:
                assert int(got.distances[i]) == d and got[i] == ops, (bound, i, len(a[i]), len(b[i]), got[i][:80], ops[:80])
                within += 1
        assert by_gap and by_distance and within, (bound, by_gap, by_distance, within)


# code points that differ from 0x41 in exactly one of the seven 3-bit groups GroupTables3 looks up (bits 0, 3, 7, 9, 12, 16, 20), two that
# differ in the two top groups alone, and the edges of the UTF-8 lengths
GROUP_SYMBOLS = [0x41, 0x40, 0x49, 0xC1, 0x241, 0x1041, 0x10041, 0x100041, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0xFFFFF, 0x10FFFF]


def test_group_symbols_differ_in_single_groups():
    groups = lambda c: [(c >> (3 * g)) & 7 for g in range(7)]
    differing = [sum(x != y for x, y in zip(groups(0x41), groups(c))) for c in GROUP_SYMBOLS[1:8]]
    assert differing == [1] * 7 and sorted(next(g for g in range(7) if groups(c)[g] != groups(0x41)[g]) for c in GROUP_SYMBOLS[1:8]) == list(range(7))
    assert [g for g in range(7) if groups(0xFFFFF)[g] != groups(0x10FFFF)[g]] == [5, 6]
    assert all("".join(map(chr, GROUP_SYMBOLS)).encode("utf-8").decode("utf-8")[i] == chr(c) for i, c in enumerate(GROUP_SYMBOLS))


@pytest.mark.gpu
def test_code_point_groups(sw, scope, lev8):
    """Exact scripts over symbols a wrong 3-bit group would confuse -- every pair checked -- and over patterns of >= 300 distinct ones."""
    rng = np.random.default_rng(33)
    draw = lambda: int(rng.choice(GROUP_SYMBOLS))
    a, b = [], []
    for i in range(1500):
        x = [draw() for _ in range(int(rng.integers(0, 121)))]
        y = mutated(rng, x, int(rng.integers(0, 10)), draw) if i % 3 else [draw() for _ in range(int(rng.integers(0, 121)))]
        a.append("".join(map(chr, x))); b.append("".join(map(chr, y[:120])))
    got = lev8.align(sw.Strs(a), sw.Strs(b), scope)
    assert (got.distances == lev8.pairs(sw.Strs(a), sw.Strs(b), scope)).all()
    check_exact(sw, got, a, b, utf8=True)
    # many distinct symbols per pattern, among them pairs that differ in one group only (c and c ^ 0x10000, c and c ^ 8)
    wide = np.concatenate([np.arange(0x4E00, 0x4E00 + 700), np.arange(0x4E00, 0x4E00 + 700) ^ 0x10000, np.arange(0x4E00, 0x4E00 + 700) ^ 0x1000])
    assert len(set(wide.tolist())) == 2100
    a, b = [], []
    for i in range(24):
        x = rng.choice(wide, int(rng.integers(320, 420)), replace=False).tolist()
        y = mutated(rng, x, int(rng.integers(0, 20)), lambda: int(rng.choice(wide)))
        if i % 4 == 3:
            x, y = y, x
        assert min(len(set(x)), len(set(y))) >= 300
        a.append("".join(map(chr, x))); b.append("".join(map(chr, y)))
    got = lev8.align(sw.Strs(a), sw.Strs(b), scope)
    check_exact(sw, got, a, b, utf8=True)


def check_offsets_from_ops(a, b, got):
    """The offsets are the running sums of the pairs' op counts la + lb - (ops that consume a symbol of both strings)."""
    offsets = got.offsets.astype(np.int64)
    assert offsets[0] == 0 and offsets[-1] == len(got.ops) and (np.diff(offsets) >= 0).all()
    seg = np.repeat(np.arange(len(got)), np.diff(offsets))
    both = np.bincount(seg[(got.ops == ord("=")) | (got.ops == ord("X"))], minlength=len(got))
    counts = a.lengths + b.lengths - both
    within = np.diff(offsets) > 0
    assert (np.diff(offsets)[within] == counts[within]).all()
    return within


@pytest.mark.gpu
@pytest.mark.parametrize("count", [2047, 2048, 2049, 4095, 4096, 4097, 8192, 256 * 2048 + 1, 256 * 4096 + 1])
def test_scan_and_emit_edges(sw, scope, lev, count):
    """Pair counts at the edges of the offsets scan, which works in tiles of 4096 values: one tile less one, exactly, plus one, two
    tiles, and one pair more than 256 tiles (the scan's 256 threads then add up more than one preceding tile sum apiece). With them the
    counts at the edges of 2048, the tile of the scan the alignments had of their own, and one pair more than 256 of those. The large
    counts are checked whole by the vectorised checks and against the reference script at the tile edges and 500 sampled pairs."""
    a, b = sw.generate_pairs("short_words", count, seed=count)
    assert len(a) == len(b) == count
    got = lev.align(a, b, scope)
    assert (got.distances == lev.pairs(a, b, scope)).all()
    check_valid_batch((a.data, a.offsets), (b.data, b.offsets), got)
    within = check_offsets_from_ops(a, b, got)
    assert within.sum() >= count - (a.lengths + b.lengths == 0).sum()
    rng = np.random.default_rng(count)
    last = (count - 1) // 4096 * 4096   # where the last tile begins
    tiles = range(0, count + 1, 2048) if count < 10_000 else (0, 2048, 4096, 8192, 255 * 2048, 256 * 2048, last - 4096, last)
    edges = [i for t in tiles for i in (t - 2, t - 1, t, t + 1) if 0 <= i < count]
    sample = sorted(set(edges + [0, count - 1] + rng.choice(count, 500, replace=False).tolist()))
    check_exact(sw, got, {i: a[i] for i in sample}, {i: b[i] for i in sample}, indices=sample)


@pytest.mark.gpu
def test_mostly_empty_scripts(sw, scope, lev):
    """Only every 1000th pair is within the bound: nearly every count the scans add is zero."""
    rng = np.random.default_rng(35)
    a, other = sw.generate_pairs("short_words", 100_000, seed=35)
    items_a = [a[i] for i in range(len(a))]
    items_b = [bytes(reversed(x)) + b"##" for x in items_a]                      # at least two edits away
    for i in range(0, len(a), 1000):
        items_b[i] = items_a[i][:3] + b"#" + items_a[i][4:]                       # at most one
    b = sw.Strs(items_b)
    got = lev.align(a, b, scope, bound=1)
    assert (got.distances == lev.pairs(a, b, scope, bound=1)).all()
    within = np.nonzero(got.distances <= 1)[0]
    assert within.tolist() == list(range(0, len(a), 1000))
    lengths = np.diff(got.offsets.astype(np.int64))
    assert (lengths[got.distances > 1] == 0).all() and (lengths[within] > 0).all() and got.offsets[-1] == len(got.ops)
    check_exact(sw, got, items_a, items_b, bound=1, indices=list(within) + [1, 999, 1001, 2047, 2048, 2049, 99_999])


@pytest.mark.gpu
def test_cell_limit(sw, scope, lev):
    """SWH_ALIGN_MAX_CELLS exactly: a pair of 2^20 x 1024 symbols (2^30 cells) is aligned, one of (2^20 + 1) x 1024 is refused."""
    rng = np.random.default_rng(36)
    long_a = bytes(rng.integers(0, 4, (1 << 20) + 1).astype(np.uint8))
    short_b = bytes(rng.integers(0, 4, 1024).astype(np.uint8))
    assert sw.ALIGN_MAX_CELLS == (1 << 20) * 1024
    for a, b in (([b"ab", long_a], [b"ba", short_b]), ([b"ab", short_b], [b"ba", long_a])):
        with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
            lev.align(sw.Strs(a), sw.Strs(b), scope)
        assert "pair 1" in str(info.value) and "1048577" in str(info.value)
    a, b = sw.Strs([b"ab", long_a[:-1]]), sw.Strs([b"ba", short_b])
    got = lev.align(a, b, scope)
    assert (got.distances == lev.pairs(a, b, scope)).all() and got[0] == b"XX"
    assert (1 << 20) - 1024 <= int(got.distances[1]) <= 1 << 20
    assert script_errors(long_a[:-1], short_b, got[1], int(got.distances[1])) is None
