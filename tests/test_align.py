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
