"""Levenshtein infix search (swh_levenshtein_infix_*): the best approximate occurrence of every pattern in its text.

The reference is computed here with numpy: the semi-global Wagner-Fischer matrix row by row -- the row loop of test_align.py's
`wagner_fischer` with a first row of zeros, so an occurrence may start anywhere -- gives d = min of the last row and end = its first
minimum; the start is the first column j whose value is d in the last row of a GLOBAL matrix of the reversed pattern against the
reversed t[:end] (start = end - j: the shortest occurrence that ends there). A pure-Python brute force over all (s, e) pins it on
the tiny cases, the oracle's Wagner-Fischer pins its distances."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def symbols(s, utf8=False) -> np.ndarray:
    if isinstance(s, str):
        return np.array([ord(c) for c in s], dtype=np.int64) if utf8 else np.frombuffer(s.encode(), dtype=np.uint8).astype(np.int64)
    return np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64)


def last_row(p: np.ndarray, t: np.ndarray, anchored: bool) -> np.ndarray:
    """Row m of the Wagner-Fischer matrix of p (rows) against t (columns); first row 0..n (anchored: global) or all zeros (semi-global)."""
    n = len(t)
    ar = np.arange(n + 1, dtype=np.int32)
    row = ar.copy() if anchored else np.zeros(n + 1, dtype=np.int32)
    tmp = np.empty(n + 1, dtype=np.int32)
    for i in range(1, len(p) + 1):
        tmp[0] = i
        np.minimum(row[:-1] + (t != p[i - 1]), row[1:] + 1, out=tmp[1:])
        row = np.minimum.accumulate(tmp - ar) + ar
    return row


def reference_infix(p, t, utf8=False):
    """(d, start, end) of the canonical occurrence."""
    p, t = symbols(p, utf8), symbols(t, utf8)
    row = last_row(p, t, anchored=False)
    d, end = int(row.min()), int(row.argmin())
    back = last_row(p[::-1], t[:end][::-1], anchored=True)
    j = int(np.nonzero(back == d)[0][0])
    return d, end - j, end


def py_levenshtein(a, b) -> int:
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j - 1] + (x != y), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[-1]


def brute_force(p, t):
    """Smallest d, then smallest end, then largest start, over every substring."""
    best = None
    for e in range(len(t) + 1):
        for s in range(e + 1):
            key = (py_levenshtein(p, t[s:e]), e, -s)
            if best is None or key < best:
                best = key
    return best[0], -best[2], best[1]


EXAMPLES = [("kitten", "the sitting cat", (2, 5, 10)), ("abc", "xxabcxx", (0, 2, 5)), ("lawn", "flaw in law", (1, 1, 4)),
            ("ab", "ba", (1, 0, 1)), ("aaa", "bbb", (3, 0, 0)), ("", "abc", (0, 0, 0)), ("abc", "", (3, 0, 0)), ("", "", (0, 0, 0))]


def rand_bytes(rng, n, alphabet, base=0):
    return bytes((rng.integers(0, alphabet, size=int(n)) + base).astype(np.uint8))


def mutated(rng, s, edits, draw):
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


def check_exact(got, patterns, texts, utf8=False, bound=None, indices=None):
    indices = range(len(patterns)) if indices is None else indices
    for i in indices:
        d, s, e = reference_infix(patterns[i], texts[i], utf8)
        have = (int(got.distances[i]), int(got.starts[i]), int(got.ends[i]))
        if bound is not None and d > bound:
            assert have == (bound + 1, NONE, NONE) and got[i] is None, (i, have, (d, s, e))
        else:
            assert have == (d, s, e) and got[i] == (d, s, e), (i, len(patterns[i]), len(texts[i]), have, (d, s, e))


def raw_call(sw, engine, scope, patterns, texts, outs, bound=None, utf8=False):
    """The C ABI itself on raw u64 tapes; `outs` are three pointers (host or device). Returns (status name, message)."""
    from stringwars_amd import _native as N
    tp, _, keep_p = sw.engines._c_tape(patterns, want64=True)
    tt, _, keep_t = sw.engines._c_tape(texts, want64=True)
    fn = N.lib.swh_levenshtein_utf8_infix_u64tape if utf8 else N.lib.swh_levenshtein_infix_u64tape
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(tp), C.byref(tt), N.UNBOUNDED if bound is None else bound,
                *(C.c_void_p(o) for o in outs), C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    for name in ("swh_levenshtein_infix_u64tape", "swh_levenshtein_utf8_infix_u64tape", "swh_levenshtein_infix_prepared"):
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "infix" in sw.capabilities().split(",")
    assert callable(sw.LevenshteinDistances.infix) and sw.LevenshteinDistancesUTF8.infix is sw.LevenshteinDistances.infix
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    assert re.search(r"#define SWH_INFIX_MAX_PATTERN 2048u", header) and N.INFIX_MAX_PATTERN == 2048 == sw.INFIX_MAX_PATTERN
    assert re.search(r"#define SWH_INFIX_NONE 0xFFFFFFFFu", header) and N.INFIX_NONE == NONE == sw.INFIX_NONE


def test_calls_fail_loudly_without_device(sw):
    import torch
    from stringwars_amd import _native as N
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    tp, _, keep_p = sw.engines._c_tape(sw.Strs([b"abc"]), want64=True)
    tt, _, keep_t = sw.engines._c_tape(sw.Strs([b"xxabcxx"]), want64=True)
    outs = [np.full(1, 77, np.uint32) for _ in range(3)]
    pointers = [C.c_void_p(o.ctypes.data) for o in outs]
    for name in ("swh_levenshtein_infix_u64tape", "swh_levenshtein_utf8_infix_u64tape"):
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, C.byref(tp), C.byref(tt), N.UNBOUNDED, *pointers, C.byref(err))
        assert N.STATUS_NAMES[status] == "no_device" and err.value, name
    view = N.PreparedView(None, 0, 1)
    err = C.c_char_p()
    status = N.lib.swh_levenshtein_infix_prepared(None, None, C.byref(view), C.byref(view), N.UNBOUNDED, *pointers, C.byref(err))
    assert N.STATUS_NAMES[status] == "no_device" and err.value
    assert all((o == 77).all() for o in outs)


def test_reference_equals_brute_force():
    strs = lambda upto: ["".join(x) for n in range(upto + 1) for x in itertools.product("ab", repeat=n)]
    pairs = [(p, t) for p in strs(3) for t in strs(5)]
    assert len(pairs) == 945
    mismatches = [(p, t) for p, t in pairs if reference_infix(p, t) != brute_force(p, t)]
    assert not mismatches, mismatches[:5]


def test_reference_distance_equals_oracle_minimum(orc, sw):
    rng = np.random.default_rng(5)
    patterns = [rand_bytes(rng, rng.integers(0, 7), 3, 97) for _ in range(200)]
    texts = [rand_bytes(rng, rng.integers(0, 13), 3, 97) for _ in range(200)]
    subs = [(i, t[s:e]) for i, t in enumerate(texts) for e in range(len(t) + 1) for s in range(e + 1)]
    owner = np.array([i for i, _ in subs])
    all_d = orc.levenshtein_pairs(sw.Strs([patterns[i] for i, _ in subs]), sw.Strs([x for _, x in subs]), algo="wf")
    for i in range(200):
        d, s, e = reference_infix(patterns[i], texts[i])
        assert d == int(np.asarray(all_d)[owner == i].min()), i
        assert py_levenshtein(patterns[i], texts[i][s:e]) == d


def test_reference_examples():
    for p, t, want in EXAMPLES:
        assert reference_infix(p, t) == want == brute_force(p, t), (p, t)


def test_infix_matches_object(sw):
    got = sw.InfixMatches(np.array([2, 4, 0], np.uint32), np.array([5, NONE, 0], np.uint32), np.array([10, NONE, 0], np.uint32))
    assert len(got) == 3 and got[0] == (2, 5, 10) and got[1] is None and got[2] == (0, 0, 0) and got[-1] == (0, 0, 0)
    assert got.found.tolist() == [True, False, True] and got.found.dtype == np.bool_
    assert got.distances.dtype == got.starts.dtype == got.ends.dtype == np.uint32
    with pytest.raises(IndexError):
        got[3]
    with pytest.raises(ValueError):
        sw.InfixMatches([1], [1, 2], [1])


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


@pytest.mark.gpu
def test_examples_and_exhaustive(sw, scope, lev, lev8):
    got = lev.infix(sw.Strs([x[0] for x in EXAMPLES]), sw.Strs([x[1] for x in EXAMPLES]), scope)
    assert [got[i] for i in range(len(EXAMPLES))] == [x[2] for x in EXAMPLES]
    for alphabet, engine, utf8 in (("ab", lev, False), ("aé", lev8, True)):
        strs = lambda upto: ["".join(x) for n in range(upto + 1) for x in itertools.product(alphabet, repeat=n)]
        pairs = [(p, t) for p in strs(4) for t in strs(6)]
        assert len(pairs) == 3937
        patterns, texts = [p for p, _ in pairs], [t for _, t in pairs]
        got = engine.infix(sw.Strs(patterns), sw.Strs(texts), scope)
        check_exact(got, patterns, texts, utf8=utf8)


BLOCK_M = (1, 31, 32, 33, 63, 64, 65, 96, 2047, 2048)


def block_edge_batch():
    rng = np.random.default_rng(41)
    patterns, texts = [], []
    for m in BLOCK_M:
        p = rand_bytes(rng, m, 4, 97)
        widths = [0, 1, 15, 16, 17, 31, 33, m - 1, m, m + 1, 300]
        if m >= 2047:
            widths = [300, m, m + 1]   # the numpy reference stays in seconds
        for k, n in enumerate(widths):
            for where in (("front", "middle", "end") if m < 2047 else (("front", "middle", "end")[k],)):
                occurrence = bytes(mutated(rng, p, int(rng.integers(0, 4)), lambda: int(rng.integers(97, 101))))
                filler = n - len(occurrence)
                if filler <= 0:
                    t = occurrence[:n] if where != "end" else occurrence[len(occurrence) - n:]
                elif where == "front":
                    t = occurrence + rand_bytes(rng, filler, 4, 97)
                elif where == "end":
                    t = rand_bytes(rng, filler, 4, 97) + occurrence
                else:
                    t = rand_bytes(rng, filler // 2, 4, 97) + occurrence + rand_bytes(rng, filler - filler // 2, 4, 97)
                assert len(t) == n
                patterns.append(p); texts.append(t)
    return patterns, texts


@pytest.mark.gpu
def test_block_edges(sw, scope, lev):
    patterns, texts = block_edge_batch()
    got = lev.infix(sw.Strs(patterns), sw.Strs(texts), scope)
    check_exact(got, patterns, texts)
    lengths = np.array([len(t) for t in texts])
    rows = np.array([len(p) for p in patterns])
    assert ((got.ends == lengths) & (lengths > 0)).any() and ((got.starts == 0) & (got.ends > 0)).any()
    assert ((got.distances <= 3) & (rows >= 2047)).any()


@pytest.mark.gpu
def test_mixed_items(sw, scope, lev):
    """Consecutive pairs of different block counts share a work item (idle lanes past the shorter patterns); per-pair results do not
    depend on which pairs are neighbours."""
    rng = np.random.default_rng(42)
    patterns, texts = [], []
    for i in range(500):
        m, n = (3, 40, 70, 200)[i % 4], int(rng.integers(0, 401))
        p = rand_bytes(rng, m, 4, 97)
        t = rand_bytes(rng, n, 4, 97)
        if i % 3 == 0 and n > m + 8:
            at = int(rng.integers(0, n - m - 4))
            t = t[:at] + bytes(mutated(rng, p, int(rng.integers(0, 5)), lambda: int(rng.integers(97, 101)))) + t[at + m:]
        patterns.append(p); texts.append(t)
    got = lev.infix(sw.Strs(patterns), sw.Strs(texts), scope)
    check_exact(got, patterns, texts)
    order = rng.permutation(500)
    again = lev.infix(sw.Strs([patterns[i] for i in order]), sw.Strs([texts[i] for i in order]), scope)
    for name in ("distances", "starts", "ends"):
        assert (getattr(again, name) == getattr(got, name)[order]).all(), name


@pytest.mark.gpu
def test_ties(sw, scope, lev):
    patterns = [b"abab"] + [b"a" * m for m in (1, 2, 31, 32, 33, 64, 65)] + [b"abc" * 20, b"xyz", b"q" * 70]
    texts = [b"ab" * 50] + [b"a" * n for n in (5, 1, 40, 32, 32, 200, 64)] + [b"defg" * 30, b"a" * 100, b""]
    got = lev.infix(sw.Strs(patterns), sw.Strs(texts), scope)
    assert got[0] == (0, 0, 4)
    # a run of one letter in a longer run: the first end that holds the whole pattern; in a shorter run: the whole text, the rest deleted
    assert [got[i] for i in range(1, 8)] == [(0, 0, 1), (1, 0, 1), (0, 0, 31), (0, 0, 32), (1, 0, 32), (0, 0, 64), (1, 0, 64)]
    assert [got[i] for i in range(8, 11)] == [(60, 0, 0), (3, 0, 0), (70, 0, 0)]   # disjoint alphabets, an empty text: (m, 0, 0)
    check_exact(got, patterns, texts)


def bounded_batch():
    """Patterns that end in '#', a byte used nowhere else in pattern or text: an exact occurrence is then the only one that ends where
    it ends, so at bound 0 the start is bytes.find's."""
    rng = np.random.default_rng(43)
    patterns, texts = [], []
    for i in range(390):
        p = rand_bytes(rng, rng.integers(20, 45), 26, 97) + b"#"
        occurrence = bytes(mutated(rng, p, i % 13, lambda: int(rng.integers(97, 123))))
        t = rand_bytes(rng, rng.integers(0, 120), 26, 97) + occurrence + rand_bytes(rng, rng.integers(0, 120), 26, 97)
        patterns.append(p); texts.append(t)
    return patterns, texts


@pytest.mark.gpu
def test_bounds(sw, scope, lev):
    patterns, texts = bounded_batch()
    reference = [reference_infix(p, t) for p, t in zip(patterns, texts)]
    assert set(range(13)) <= {d for d, _, _ in reference}
    sp, st = sw.Strs(patterns), sw.Strs(texts)
    for bound in (0, 1, 2, 7):
        got = lev.infix(sp, st, scope, bound=bound)
        for i, (d, s, e) in enumerate(reference):
            have = (int(got.distances[i]), int(got.starts[i]), int(got.ends[i]))
            assert have == ((d, s, e) if d <= bound else (bound + 1, NONE, NONE)), (bound, i, have, (d, s, e))
        assert (got.found == (np.array([d for d, _, _ in reference]) <= bound)).all() and got.found.any() and not got.found.all()
        if bound == 0:
            finds = np.array([t.find(p) for p, t in zip(patterns, texts)])
            assert ((finds >= 0) == got.found).all() and (got.starts[got.found] == finds[finds >= 0]).all()
            assert (got.ends[got.found] == finds[finds >= 0] + np.array([len(p) for p in patterns])[got.found]).all()
    unbounded = lev.infix(sp, st, scope)
    assert [unbounded[i] for i in range(len(patterns))] == reference


def same(got, want):
    return all((getattr(got, name) == getattr(want, name)).all() for name in ("distances", "starts", "ends"))


@pytest.mark.gpu
def test_forms_and_scopes(sw, scope, lev):
    import torch
    from stringwars_amd import _native as N
    rng = np.random.default_rng(44)
    patterns = [rand_bytes(rng, rng.integers(0, 90), 4, 97) for _ in range(700)]
    texts = [rand_bytes(rng, rng.integers(0, 300), 4, 97) for _ in range(700)]
    for i in range(0, 700, 2):   # half the patterns occur, a few edits off
        at = int(rng.integers(0, len(texts[i]) + 1))
        texts[i] = texts[i][:at] + bytes(mutated(rng, patterns[i], int(rng.integers(0, 4)), lambda: int(rng.integers(97, 101)))) + texts[i][at:]
    sp, st = sw.Strs(patterns), sw.Strs(texts)
    assert sp.offsets[-1] != st.offsets[-1]
    want = lev.infix(sp, st, scope, bound=20)
    check_exact(want, patterns, texts, bound=20, indices=range(0, 700, 7))
    assert want.found.any() and not want.found.all()
    # device outputs equal host outputs
    outs = [torch.full((700,), 77, dtype=torch.int32, device="cuda") for _ in range(3)]
    status, message = raw_call(sw, lev, scope, sp, st, [o.data_ptr() for o in outs], bound=20)
    assert status == "success", message
    device = sw.InfixMatches(*(o.cpu().numpy().astype(np.uint32) for o in outs))
    assert same(device, want)
    # one output on the device, two on the host
    mixed_d = torch.zeros(700, dtype=torch.int32, device="cuda")
    host_s, host_e = np.zeros(700, np.uint32), np.zeros(700, np.uint32)
    status, message = raw_call(sw, lev, scope, sp, st, [mixed_d.data_ptr(), host_s.ctypes.data, host_e.ctypes.data], bound=20)
    assert status == "success" and same(sw.InfixMatches(mixed_d.cpu().numpy().astype(np.uint32), host_s, host_e), want)
    # raw device tapes; prepared tapes in all four offset-width mixes, whole and as sub-views
    assert same(lev.infix(sp.to_device(scope), st.to_device(scope), scope, bound=20), want)
    tapes = {(w, name): sw.PreparedTape(scope, sw.Strs(items).with_offsets(w)) for w in (np.uint32, np.uint64)
             for name, items in (("p", patterns), ("t", texts))}
    for wp, wt in itertools.product((np.uint32, np.uint64), repeat=2):
        pp, pt = tapes[(wp, "p")], tapes[(wt, "t")]
        assert same(lev.infix(pp, pt, scope, bound=20), want), (wp, wt)
        sub = lev.infix(pp[37:333], pt[37:333], scope, bound=20)
        assert all((getattr(sub, name) == getattr(want, name)[37:333]).all() for name in ("distances", "starts", "ends")), (wp, wt)
    # tapes of two kinds: refused by the C ABI, nothing written
    as_utf8 = sw.PreparedTape(scope, st, utf8=True)
    vp, vt, err = tapes[(np.uint64, "p")].view(), as_utf8.view(), C.c_char_p()
    untouched = [np.full(700, 77, np.uint32) for _ in range(3)]
    status = N.lib.swh_levenshtein_infix_prepared(lev._handle, scope.handle, C.byref(vp), C.byref(vt), N.UNBOUNDED,
                                                  *(C.c_void_p(o.ctypes.data) for o in untouched), C.byref(err))
    assert N.STATUS_NAMES[status] == "invalid_argument" and all((o == 77).all() for o in untouched)
    with pytest.raises(ValueError):
        lev.infix(tapes[(np.uint64, "p")], as_utf8, scope)
    # a caller-stream scope -- synchronous, then asynchronous, then pipelined: the results are visible when the call returns
    other = sw.DeviceScope(gpu_device=0, stream=torch.cuda.current_stream().cuda_stream)
    engine = sw.LevenshteinDistances(capabilities=other)
    assert same(engine.infix(sp, st, other, bound=20), want)
    for mode in ("async", "pipelined"):
        if mode == "async":
            other.set_async(True)
        else:
            other.set_async(False)
            other.set_pipelined(True)
        engine.pairs(sp, st, other)   # outstanding work the call joins
        assert same(engine.infix(sp, st, other, bound=20), want), mode
        other.synchronize()
    # count == 0: success, nothing written
    empty = lev.infix(sw.Strs([]), sw.Strs([]), scope)
    assert len(empty) == 0 and empty.found.tolist() == []
    untouched = [np.full(4, 77, np.uint32) for _ in range(3)]
    status, _ = raw_call(sw, lev, scope, sw.Strs([]), sw.Strs([]), [o.ctypes.data for o in untouched])
    assert status == "success" and all((o == 77).all() for o in untouched)
    # profiling describes the whole call
    scope.set_profiling(True)
    try:
        lev.infix(sp, st, scope)
        timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    assert timing["cells"] == int((sp.lengths * st.lengths).sum())
    assert timing["dominant_name"].startswith("infix") and timing["kernels"] == 3


def golden_lines():
    z = np.load(os.path.join(GOLDEN, "script_lines.npz"))
    lines = []
    for side in "ab":
        data, offsets = z[side + "_data"], z[side + "_offsets"].astype(np.int64)
        lines += [bytes(data[offsets[i]:offsets[i + 1]]).decode("utf-8") for i in range(len(offsets) - 1)]
    return lines


@pytest.mark.gpu
def test_utf8(sw, scope, lev8):
    rng = np.random.default_rng(45)
    patterns, texts = [], []
    for line in golden_lines():   # words of line i searched in line i, some of them one or two edits off
        words = [w for w in line.split() if len(w) >= 2]
        for k, w in enumerate(words[3::max(1, len(words) // 10)][:10]):
            drawn = mutated(rng, w, k % 3, lambda: line[int(rng.integers(0, len(line)))])
            patterns.append("".join(drawn)); texts.append(line)
    z = np.load(os.path.join(GOLDEN, "uwords.npz"))
    words = lambda side: [bytes(z[side + "_data"][int(z[side + "_offsets"][i]):int(z[side + "_offsets"][i + 1])]).decode("utf-8")
                          for i in range(len(z[side + "_offsets"]) - 1)]
    haystack = " ".join(words("c"))
    for w in words("q"):
        patterns.append(w); texts.append(haystack)
    # mixed 1- to 4-byte sequences: positions are code points, not bytes
    mixed = [0x61, 0x62, 0xE9, 0x3B1, 0x4E2D, 0x6587, 0x1F600, 0x10FFFF, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000]
    for i in range(300):
        p = [int(rng.choice(mixed)) for _ in range(int(rng.integers(0, 70)))]
        t = [int(rng.choice(mixed)) for _ in range(int(rng.integers(0, 150)))]
        if i % 2:
            at = int(rng.integers(0, len(t) + 1))
            t = t[:at] + mutated(rng, p, int(rng.integers(0, 4)), lambda: int(rng.choice(mixed))) + t[at:]
        patterns.append("".join(map(chr, p))); texts.append("".join(map(chr, t)))
    assert len(patterns) >= 400 and any(len(t.encode()) > len(t) for t in texts)
    got = lev8.infix(sw.Strs(patterns), sw.Strs(texts), scope)
    check_exact(got, patterns, texts, utf8=True)
    prepared = lev8.infix(sw.PreparedTape(scope, sw.Strs(patterns), utf8=True), sw.PreparedTape(scope, sw.Strs(texts), utf8=True), scope)
    assert same(prepared, got)
    exact = (got.distances == 0) & (np.array([len(p) for p in patterns]) > 0)   # positions in code points: end - start = len(pattern)
    assert exact.sum() >= 40 and (got.ends[exact] - got.starts[exact] == np.array([len(p) for p in patterns])[exact]).all()
    # invalid UTF-8 in either tape: the status, and the outputs untouched
    outs = [np.full(2, 77, np.uint32) for _ in range(3)]
    for bad_p, bad_t in (([b"ok", b"\xff\xfe"], [b"ok", b"x"]), ([b"ok", b"x"], [b"ok", b"\xc3"])):
        status, _ = raw_call(sw, lev8, scope, sw.Strs(bad_p), sw.Strs(bad_t), [o.ctypes.data for o in outs], utf8=True)
        assert status == "invalid_utf8" and all((o == 77).all() for o in outs)


@pytest.mark.gpu
def test_refusals(sw, scope, lev):
    rng = np.random.default_rng(46)
    patterns = [b"abc", rand_bytes(rng, 2048, 4, 97), rand_bytes(rng, 2049, 4, 97), b"abc", rand_bytes(rng, 3000, 4, 97)]
    texts = [b"xxabcxx", rand_bytes(rng, 100, 4, 97), rand_bytes(rng, 100, 4, 97), b"", b"abc"]
    outs = [np.full(5, 77, np.uint32) for _ in range(3)]
    status, message = raw_call(sw, lev, scope, sw.Strs(patterns), sw.Strs(texts), [o.ctypes.data for o in outs])
    assert status == "unsupported_length" and "pair 2" in message and "2049" in message, message
    assert all((o == 77).all() for o in outs)
    with pytest.raises(sw.StringWarsError, match="unsupported_length") as info:
        lev.infix(sw.Strs(patterns), sw.Strs(texts), scope)
    assert "pair 2" in str(info.value)
    got = lev.infix(sw.Strs(patterns[:2]), sw.Strs(texts[:2]), scope)   # 2048 symbols are accepted
    check_exact(got, patterns[:2], texts[:2])
    # count mismatch
    status, _ = raw_call(sw, lev, scope, sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), [o.ctypes.data for o in outs])
    assert status == "invalid_argument" and all((o == 77).all() for o in outs)
    with pytest.raises(ValueError):
        lev.infix(sw.Strs([b"a"]), sw.Strs([b"a", b"b"]), scope)
    # a general-cost engine
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    with pytest.raises(sw.StringWarsError, match="not_implemented"):
        costly.infix(sw.Strs([b"abc"]), sw.Strs([b"xxabcxx"]), scope)


@pytest.mark.gpu
def test_seeded_random_round(sw, orc, scope, lev):
    rng = np.random.default_rng(2027)
    count = 20_000
    alphabets = np.array([2, 4, 26, 256])[rng.integers(0, 4, size=count)]
    rows, columns = rng.integers(0, 101, size=count), rng.integers(0, 601, size=count)
    planted, edits = rng.integers(0, 2, size=count), rng.integers(0, 6, size=count)
    patterns, texts = [], []
    for i in range(count):
        alphabet = int(alphabets[i])
        p, t = rand_bytes(rng, rows[i], alphabet), rand_bytes(rng, columns[i], alphabet)
        if planted[i]:
            at = int(rng.integers(0, len(t) + 1))
            t = (t[:at] + bytes(mutated(rng, p, int(edits[i]), lambda: int(rng.integers(0, alphabet)))) + t[at:])[:600]
        patterns.append(p); texts.append(t)
    # every random number is drawn: the device comes now
    got = lev.infix(sw.Strs(patterns), sw.Strs(texts), scope)
    check_exact(got, patterns, texts, indices=range(0, count, 400))
    lengths = np.array([len(t) for t in texts])
    assert got.found.all() and (got.starts <= got.ends).all() and (got.ends <= lengths).all()
    assert (got.distances <= np.array([len(p) for p in patterns])).all()
    occurrences = [t[int(s):int(e)] for t, s, e in zip(texts, got.starts, got.ends)]
    valid = orc.levenshtein_pairs(sw.Strs(patterns), sw.Strs(occurrences), algo="wf")
    assert (np.asarray(valid).astype(np.int64) == got.distances.astype(np.int64)).all()
