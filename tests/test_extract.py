"""The score search (swh_levenshtein_extract_*, engine.extract): the k best candidates of every query by an OSA, Indel, LCS, ratio,
Jaro or Jaro-Winkler score, against references in pure Python.

The counts come from the references of tests/test_osa.py (Wagner-Fischer with the transposition term), tests/test_lcs.py (the LCS
table) and tests/test_jaro.py (the header's matching on big integers); the scores are the header's expressions, evaluated here
operation by operation on Python floats; the expected rows are a stable sort of the admitted candidates by score. Every comparison
is exact: indices equal, scores equal as 64-bit patterns."""
import ctypes as C
import functools
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child
from test_jaro import mutated, r2 as jaro_counts_of, symbols as symbols_of
from test_lcs import reference_lcs
from test_osa import reference_osa

SCORERS = ("osa", "indel", "lcs", "ratio", "jaro", "jaro_winkler")
LARGER_IS_BETTER = {"osa": False, "indel": False, "lcs": True, "ratio": True, "jaro": True, "jaro_winkler": True}
EXTRACT_SYMBOLS = ("swh_levenshtein_extract_u64tape", "swh_levenshtein_utf8_extract_u64tape", "swh_levenshtein_extract_prepared")
PAD_INDEX, PAD_BITS = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
HOOK = "STRINGWARS_AMD_EXTRACT_CHUNK_PAIRS"
SENTINEL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE, PACKAGE = os.path.join(ROOT, "include"), os.path.join(ROOT, "stringwars_amd")


# ---- the references -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distinct_counts(queries, candidates, utf8):
    """osa, lcs, M, t, prefix as (len(queries), len(candidates)) int64 arrays and the symbol lengths m, n, for tuples of strings."""
    a = [q for q in queries for _ in candidates]
    b = [c for _ in queries for c in candidates]
    shape = (len(queries), len(candidates))
    jaro = np.array([jaro_counts_of(symbols_of(x, utf8), symbols_of(y, utf8)) for x, y in zip(a, b)], dtype=np.int64).reshape(shape + (3,))
    m = np.array([len(symbols_of(q, utf8)) for q in queries], dtype=np.int64)
    n = np.array([len(symbols_of(c, utf8)) for c in candidates], dtype=np.int64)
    return (reference_osa(a, b, utf8).reshape(shape), reference_lcs(a, b, utf8).reshape(shape), jaro[..., 0], jaro[..., 1], jaro[..., 2], m, n)


def reference_counts(queries, candidates, utf8=False):
    """The same for lists with repeats: every distinct pair is worked out once."""
    dq, dc = sorted(set(queries)), sorted(set(candidates))
    osa, lcs, M, t, prefix, m, n = _distinct_counts(tuple(dq), tuple(dc), utf8)
    qi, ci = [dq.index(q) for q in queries], [dc.index(c) for c in candidates]
    at = np.ix_(qi, ci)
    return osa[at], lcs[at], M[at], t[at], prefix[at], m[qi], n[ci]


def score_of(scorer, osa, L, M, t, prefix, m, n, p=0.1):
    """The header's expressions on Python ints and floats, one IEEE operation at a time, as written."""
    indel = m + n - 2 * L
    if scorer == "osa":
        return float(osa)
    if scorer == "indel":
        return float(indel)
    if scorer == "lcs":
        return float(L)
    if scorer == "ratio":
        twice = 2.0 * float(L)
        total = float(indel) + twice
        return 100.0 * twice / total if total > 0 else 100.0
    if m == 0 and n == 0:
        jaro = 1.0
    elif M == 0:
        jaro = 0.0
    else:
        jaro = (float(M) / float(m) + float(M) / float(n) + (float(M) - float(t)) / float(M)) / 3.0
    if scorer == "jaro":
        return jaro
    return jaro + float(prefix) * p * (1.0 - jaro) if jaro > 0.7 else jaro


def reference_scores(scorer, counts, p=0.1):
    osa, lcs, M, t, prefix, m, n = counts
    rows, columns = osa.shape
    return np.array([[score_of(scorer, int(osa[i, j]), int(lcs[i, j]), int(M[i, j]), int(t[i, j]), int(prefix[i, j]), int(m[i]), int(n[j]), p)
                      for j in range(columns)] for i in range(rows)], dtype=np.float64).reshape(rows, columns)


def expected_rows(scores, larger_is_better, k, cutoff=None):
    """(indices uint32, score patterns uint64), each (rows, k): per row a STABLE sort of the admitted candidates by score -- equal
    float64 scores stay in index order -- cut at k and padded with 0xFFFFFFFF and a pattern of ones."""
    scores = np.asarray(scores, dtype=np.float64)
    rows, columns = scores.shape
    indices = np.full((rows, k), PAD_INDEX, dtype=np.uint32)
    bits = np.full((rows, k), PAD_BITS, dtype=np.uint64)
    for i in range(rows):
        row = scores[i]
        admitted = np.ones(columns, dtype=bool) if cutoff is None else (row >= cutoff if larger_is_better else row <= cutoff)
        order = np.argsort(-row if larger_is_better else row, kind="stable")
        order = order[admitted[order]][:k]
        indices[i, :len(order)] = order
        bits[i, :len(order)] = row[order].view(np.uint64)
    return indices, bits


def winkler_fused(jaro, prefix, p):
    """The Winkler term with the second product unrounded -- what a fused multiply-add computes: fl(jaro + fl(l * p) * fl(1 - jaro))."""
    if not jaro > 0.7:
        return jaro
    lp, rest = float(prefix) * p, 1.0 - jaro
    return float(Fraction(jaro) + Fraction(lp) * Fraction(rest))   # (int / int of a Fraction is correctly rounded)


def fused_differs(counts, p):
    """How many pairs of `counts` get another Jaro-Winkler value from the contracted form than from the expression as written."""
    osa, lcs, M, t, prefix, m, n = counts
    differ = 0
    for i in range(M.shape[0]):
        for j in range(M.shape[1]):
            jaro = score_of("jaro", 0, 0, int(M[i, j]), int(t[i, j]), 0, int(m[i]), int(n[j]))
            differ += winkler_fused(jaro, int(prefix[i, j]), p) != score_of("jaro_winkler", 0, 0, int(M[i, j]), int(t[i, j]), int(prefix[i, j]),
                                                                            int(m[i]), int(n[j]), p)
    return differ


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 80)
PLANTED_ROWS, PLANTED_COLUMNS = (30, 31), (40, 291)


@functools.lru_cache(maxsize=None)
def word_batch(utf8, queries=70, candidates=300, seed=5):
    """Mutated words of 0 .. 80 symbols over a small alphabet: pairs cross the 32- and 64-symbol block edges, many match well (a
    shared base word: common prefixes, Jaro over 0.7) and many badly. The query of row 30 sits in the first 64 candidates and the one
    of row 31 in the last 44: a best candidate in the first slice and one in the last, where the columns are cut into 64s."""
    rng = np.random.default_rng(seed + (100 if utf8 else 0))
    alphabet = list("aé中ж😀bcd") if utf8 else list("abcdefgh")
    draw = lambda: alphabet[int(rng.integers(0, len(alphabet)))]
    word = lambda size: "".join(draw() for _ in range(size))
    bases = [word(size) for size in EDGE_LENGTHS] + [word(int(size)) for size in rng.integers(2, 81, 15)]
    def family(count):
        out = []
        for i in range(count):
            base = bases[i % len(bases)] if i < 2 * len(bases) else bases[int(rng.integers(0, len(bases)))]
            out.append("".join(mutated(rng, base, int(rng.integers(0, 5)) if i >= len(bases) else 0, draw))[:80])
        return out
    qs, cs = family(queries), family(candidates)
    qs[PLANTED_ROWS[0]], qs[PLANTED_ROWS[1]] = word(40), word(41)
    cs[PLANTED_COLUMNS[0]], cs[PLANTED_COLUMNS[1]] = qs[PLANTED_ROWS[0]], qs[PLANTED_ROWS[1]]
    return tuple(qs), tuple(cs)


@functools.lru_cache(maxsize=None)
def word_batch_counts(utf8):
    qs, cs = word_batch(utf8)
    return reference_counts(list(qs), list(cs), utf8)


@functools.lru_cache(maxsize=None)
def word_batch_scores(utf8, scorer, p=0.1):
    return reference_scores(scorer, word_batch_counts(utf8), p)


def as_items(strings, utf8):
    return list(strings) if utf8 else [s.encode() for s in strings]


def tapes(sw, scope, engine, queries, candidates, form):
    """The two sides in one of the forms a call takes. `candidates` None: the self-search."""
    make = {
        "strs": lambda items: sw.Strs(items),
        "strs32": lambda items: sw.Strs(items).with_offsets(np.uint32),
        "device": lambda items: sw.Strs(items).to_device(scope),
        "prepared": lambda items: sw.PreparedTape(scope, sw.Strs(items), utf8=engine._utf8),
        "prepared32": lambda items: sw.PreparedTape(scope, sw.Strs(items).with_offsets(np.uint32), utf8=engine._utf8),
    }[form]
    return make(queries), None if candidates is None else make(candidates)


def run_extract(sw, scope, engine, queries, candidates, form="strs", device_out=False, **kw):
    """engine.extract on one tape form, into host arrays or device tensors: (indices uint32, score patterns uint64)."""
    q, c = tapes(sw, scope, engine, queries, candidates, form)
    if not device_out:
        indices, scores = engine.extract(q, c, scope, **kw)
        return indices, scores.view(np.uint64)
    import torch
    rows, k = len(queries), kw["k"]
    indices = torch.full((rows, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    scores = torch.full((rows, k), 7.0, dtype=torch.float64, device="cuda")
    engine.extract(q, c, scope, out=(indices, scores), **kw)
    torch.cuda.synchronize()
    return indices.cpu().numpy().view(np.uint32), scores.cpu().numpy().view(np.uint64)


def assert_rows(got, want, what):
    (got_i, got_s), (want_i, want_s) = got, want
    assert got_i.shape == want_i.shape and got_s.shape == want_s.shape, what
    bad = np.argwhere((got_i != want_i) | (got_s != want_s))
    if len(bad):
        i, j = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at row {i} place {j}: got index {int(got_i[i, j])} score "
                             f"{got_s[i, j:j + 1].view(np.float64)[0]!r}, want index {int(want_i[i, j])} score {want_s[i, j:j + 1].view(np.float64)[0]!r}")


def raw_extract(sw, engine, scope, queries, candidates, scorer, k, cutoff, p, indices, scores, utf8=False):
    """The C ABI itself on raw u64 tapes. Returns (status name, message)."""
    from stringwars_amd import _native as N
    tq, _, keep_q = sw.engines._c_tape(sw.Strs(queries), want64=True)
    tc, _, keep_c = sw.engines._c_tape(sw.Strs(candidates), want64=True) if candidates is not None else (None, None, None)
    fn = N.lib.swh_levenshtein_utf8_extract_u64tape if utf8 else N.lib.swh_levenshtein_extract_u64tape
    bits = [C.c_uint64(int(np.float64(value).view(np.uint64))) for value in (cutoff, p)]
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(tq), C.byref(tc) if tc is not None else None, scorer, k, bits[0], bits[1],
                C.c_void_p(indices.ctypes.data), C.c_void_p(scores.ctypes.data), C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


# ---- CPU: the surface and the references -------------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    shipped, test_library = C.CDLL(sw.LIBRARY_PATH), C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    for name in EXTRACT_SYMBOLS:
        assert hasattr(shipped, name) and hasattr(test_library, name) and name in N.SIGNATURES, name
    assert "extract" in sw.capabilities().split(",")
    assert tuple(sw.SCORERS) == SCORERS and [N.SCORERS[name] for name in SCORERS] == list(range(6))
    for cls in (sw.LevenshteinDistances, sw.LevenshteinDistancesUTF8):
        assert callable(getattr(cls, "extract"))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stringwars_amd.h")).read()
    for value, name in enumerate(("OSA", "INDEL", "LCS", "RATIO", "JARO", "JARO_WINKLER")):
        assert f"#define SWH_SCORER_{name} {value}\n" in header


def test_calls_fail_loudly_without_handles(sw):
    """No scope or engine can exist without a device: with null handles every export says that there is no device -- or, where there is
    one, that the handles are null -- sets a message and writes nothing."""
    import torch
    from stringwars_amd import _native as N
    want = "invalid_argument" if torch.cuda.is_available() else "no_device"
    tape, _, keep = sw.engines._c_tape(sw.Strs([b"abc"]), want64=True)
    view = N.PreparedView(None, 0, 1)
    for name in EXTRACT_SYMBOLS:
        indices, scores = np.full(4, SENTINEL, dtype=np.uint8), np.full(8, SENTINEL, dtype=np.uint8)
        side = C.byref(view) if name.endswith("prepared") else C.byref(tape)
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, side, side, 4, 1, 0, 0, C.c_void_p(indices.ctypes.data), C.c_void_p(scores.ctypes.data), C.byref(err))
        assert N.STATUS_NAMES[status] == want and err.value, (name, status)
        assert (indices == SENTINEL).all() and (scores == SENTINEL).all(), name
    with pytest.raises(ValueError):
        sw.LevenshteinDistances.extract(None, [b"a"], None, None, scorer="jaro", k=1)   # (no scope: refused before anything is touched)


def test_expected_rows_on_a_tie_case():
    """Hand-written: equal scores keep index order, the cutoff admits a score equal to it, short rows are padded."""
    scores = np.array([[0.5, 0.9, 0.5, 0.9, 0.1], [2.0, 1.0, 2.0, 1.0, 1.0]])
    indices, bits = expected_rows(scores, True, 3)
    assert indices.tolist() == [[1, 3, 0], [0, 2, 1]]
    assert bits.view(np.float64).tolist() == [[0.9, 0.9, 0.5], [2.0, 2.0, 1.0]]
    indices, bits = expected_rows(scores, False, 4, cutoff=1.0)
    assert indices.tolist() == [[4, 0, 2, 1], [1, 3, 4, PAD_INDEX]]
    assert bits[1, 3] == PAD_BITS and np.isnan(bits.view(np.float64)[1, 3]) and bits.view(np.float64)[1, :3].tolist() == [1.0, 1.0, 1.0]
    indices, bits = expected_rows(scores, True, 2, cutoff=0.9)
    assert indices.tolist() == [[1, 3], [0, 2]]
    indices, bits = expected_rows(scores[:1], True, 2, cutoff=0.95)
    assert indices.tolist() == [[PAD_INDEX, PAD_INDEX]] and (bits == PAD_BITS).all()
    assert expected_rows(np.zeros((2, 0)), True, 2)[0].tolist() == [[PAD_INDEX] * 2] * 2


def test_expected_rows_on_the_worked_examples(sw):
    """The header's table through the references and the row helper; the engines' own host expressions give the same bits."""
    pairs = [("MARTHA", "MARHTA", 0.9444444444444445, 0.9611111111111111), ("DWAYNE", "DUANE", 0.8222222222222223, 0.8400000000000001),
             ("DIXON", "DICKSONX", 0.7666666666666666, 0.8133333333333332), ("CRATE", "TRACE", 0.7333333333333334, 0.7333333333333334),
             ("", "", 1.0, 1.0), ("ab", "ba", 0.0, 0.0)]
    for a, b, jaro, winkler in pairs:
        counts = reference_counts([a], [b])
        assert reference_scores("jaro", counts)[0, 0] == jaro and reference_scores("jaro_winkler", counts)[0, 0] == winkler, (a, b)
    counts = reference_counts(["CRATE"], ["TRACE"])   # jaro > 0.7 with no common prefix: the Winkler branch is taken and adds nothing
    assert int(counts[2][0, 0]) == 3 and int(counts[4][0, 0]) == 0 and reference_scores("jaro", counts)[0, 0] > 0.7
    # the worked row of the header
    counts = reference_counts(["MARTHA"], ["MARHTA", "DWAYNE", "MARTHA", "MARTHA"])
    indices, bits = expected_rows(reference_scores("jaro_winkler", counts), True, 3)
    assert indices.tolist() == [[2, 3, 0]] and bits.view(np.float64).tolist() == [[1.0, 1.0, 0.9611111111111111]]
    indices, bits = expected_rows(reference_scores("osa", counts), False, 4, cutoff=2.0)
    assert indices.tolist() == [[2, 3, 0, PAD_INDEX]] and bits.view(np.float64)[0, :3].tolist() == [0.0, 0.0, 1.0]
    # the scalar expressions here and the numpy expressions of engines.py, bit for bit, on the word batch
    osa, lcs, M, t, prefix, m, n = word_batch_counts(False)
    engine = sw.LevenshteinDistances
    indel = m[:, None] + n[None, :] - 2 * lcs
    assert (engine._ratio(indel.astype(np.uint64), lcs.astype(np.uint64)).view(np.uint64) == word_batch_scores(False, "ratio").view(np.uint64)).all()
    jaro = engine._jaro(M.astype(np.uint64), t.astype(np.uint64), m[:, None], n[None, :])
    assert (jaro.view(np.uint64) == word_batch_scores(False, "jaro").view(np.uint64)).all()
    for p in (0.0, 0.1, 0.25):
        assert (engine._winkler(jaro, prefix.astype(np.uint64), p).view(np.uint64) == word_batch_scores(False, "jaro_winkler", p).view(np.uint64)).all()


def test_the_word_batch_reaches_what_it_is_for():
    """Both sides of jaro > 0.7, common prefixes of four, block-edge lengths, ties, the planted best candidates, and candidates whose
    Jaro-Winkler value a contracted multiply-add would get wrong in the last bit."""
    for utf8 in (False, True):
        qs, cs = word_batch(utf8)
        osa, lcs, M, t, prefix, m, n = word_batch_counts(utf8)
        assert len(qs) == 70 and len(cs) == 300 and set(EDGE_LENGTHS) <= set(m.tolist()) and set(EDGE_LENGTHS) <= set(n.tolist())
        jaro = word_batch_scores(utf8, "jaro")
        assert (jaro > 0.7).sum() > 100 and (jaro <= 0.7).sum() > 100 and ((prefix == 4) & (jaro > 0.7)).sum() > 20 and (t > 0).sum() > 100
        assert [int(jaro[row].argmax()) for row in PLANTED_ROWS] == list(PLANTED_COLUMNS) and jaro[PLANTED_ROWS[0], PLANTED_COLUMNS[0]] == 1.0
        assert fused_differs(tuple(x[:12] for x in (osa, lcs, M, t, prefix)) + (m[:12], n), 0.1) > 0
        # ... and the rows the GPU tests compare would show it: with the contracted values in place the expected rows are others
        fused = np.array([[winkler_fused(float(jaro[i, j]), int(prefix[i, j]), 0.1) for j in range(300)] for i in range(70)])
        assert (expected_rows(fused, True, 64)[1] != expected_rows(word_batch_scores(utf8, "jaro_winkler"), True, 64)[1]).any()


@functools.lru_cache(maxsize=None)
def wide_key_case():
    """Query 'a' * m (M of its symbols can match); candidate (M, n) = 'a' * M + 'c' * (n - M): M matches in order, no transposition,
    jaro = (M / m + M / n + M / M) / 3. Over all M <= m and n <= 2048, two candidates whose scores differ as float64 and agree as
    float32. Returns (m, (M, n) of the worse one, (M, n) of the better one)."""
    m = 1024
    M = np.repeat(np.arange(1, m + 1, dtype=np.float64), 2048)
    n = np.tile(np.arange(1, 2049, dtype=np.float64), m)
    keep = n >= M
    M, n = M[keep], n[keep]
    jaro = (M / float(m) + M / n + (M - 0.0) / M) / 3.0
    order = np.argsort(jaro, kind="stable")
    ordered = jaro[order]
    close = np.nonzero((ordered[1:] != ordered[:-1]) & (ordered[1:].astype(np.float32) == ordered[:-1].astype(np.float32)) &
                       ((ordered[1:].view(np.uint64) >> np.uint64(32)) == (ordered[:-1].view(np.uint64) >> np.uint64(32))))[0]
    assert len(close), "no two of these candidates agree as float32 and differ as float64"
    at = int(close[len(close) // 2])
    worse, better = int(order[at]), int(order[at + 1])
    return m, (int(M[worse]), int(n[worse])), (int(M[better]), int(n[better]))


def wide_key_strings():
    m, worse, better = wide_key_case()
    return "a" * m, ["a" * worse[0] + "c" * (worse[1] - worse[0]), "a" * better[0] + "c" * (better[1] - better[0])]


def test_wide_key_case_is_what_it_claims():
    """The CPU search finds such a pair well below 2048 symbols: the scores differ as float64, coincide as float32 (and in their upper
    32 bits: a key of 32 score bits and the index would merge them), and the better one has the larger index."""
    query, candidates = wide_key_strings()
    counts = reference_counts([query], candidates)
    m, worse, better = wide_key_case()
    assert counts[2].tolist() == [[worse[0], better[0]]] and counts[3].tolist() == [[0, 0]]
    scores = reference_scores("jaro", counts)[0]
    assert scores[1] > scores[0] and np.float32(scores[1]) == np.float32(scores[0])
    assert int(scores.view(np.uint64)[0]) >> 32 == int(scores.view(np.uint64)[1]) >> 32
    assert expected_rows(scores[None, :], True, 1)[0].tolist() == [[1]]


# ---- the C++ wrappers: a program of their own ---------------------------------------------------------------------------------------------
def build_check_extract(tmp_path):
    """tests/bindings/check_extract.cpp against include/stringwars_amd.hpp and the shipped library."""
    binary = tmp_path / "check_extract"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "tests", "bindings", "check_extract.cpp"),
                    "-o", str(binary), "-L", PACKAGE, "-lstringwars_amd", f"-Wl,-rpath,{PACKAGE}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True, timeout=300)
    return binary


def write_extract_case(path, utf8, queries, candidates, requests):
    """The case file of check_extract.cpp; `requests`: (scorer id, prepared, self, k, cutoff or None, prefix weight)."""
    with open(path, "wb") as out:
        out.write(struct.pack("<i", int(utf8)))
        for side in (queries, candidates):
            items = [s.encode() for s in side]
            offsets = np.zeros(len(items) + 1, dtype=np.uint64)
            np.cumsum([len(s) for s in items], out=offsets[1:])
            out.write(struct.pack("<Q", len(items)) + offsets.tobytes() + b"".join(items))
        out.write(struct.pack("<I", len(requests)))
        for scorer, prepared, own, k, cutoff, p in requests:
            out.write(struct.pack("<iiiQdd", scorer, int(prepared), int(own), k, float("nan") if cutoff is None else cutoff, p))


def test_cpp_program_builds_and_fails_loudly_without_a_device(tmp_path):
    """The wrappers' program compiles against the header with warnings as errors; where no device is visible it ends with the
    library's status (no_device) on stderr and writes no result."""
    import torch
    binary = build_check_extract(tmp_path)
    if torch.cuda.is_available():
        return   # (with a device the program is run by test_cpp_wrappers_against_the_reference)
    write_extract_case(tmp_path / "tiny.case", False, ["martha"], ["marhta"], [(4, 0, 0, 1, None, 0.1)])
    done = subprocess.run([str(binary), str(tmp_path / "tiny.case"), str(tmp_path / "tiny.out")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2 and "status 5" in done.stderr, (done.returncode, done.stderr)
    assert os.path.getsize(tmp_path / "tiny.out") == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


@pytest.mark.gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
@pytest.mark.parametrize("scorer", SCORERS)
def test_every_scorer_on_every_form(sw, scope, lev, lev8, scorer, utf8):
    """70 x 300 mutated words of 0 .. 80 symbols, k in {1, 5, 64}, host and device outputs, raw tapes with 64- and 32-bit offsets,
    device tapes and prepared tapes of both offset widths (and a sub-view of one)."""
    engine = lev8 if utf8 else lev
    qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
    scores = word_batch_scores(utf8, scorer)
    for k in (1, 5, 64):
        want = expected_rows(scores, LARGER_IS_BETTER[scorer], k)
        for form in ("strs", "strs32", "device", "prepared", "prepared32"):
            for device_out in ((False, True) if form in ("strs", "prepared32") else (False,)):
                got = run_extract(sw, scope, engine, qs, cs, form, device_out, scorer=scorer, k=k)
                assert_rows(got, want, f"{scorer} utf8={utf8} k={k} {form} device_out={device_out}")
    # views of prepared tapes: rows 9 .. 40 against candidates 17 .. 290 (indices count from the view's first candidate)
    pq, pc = tapes(sw, scope, engine, qs, cs, "prepared")
    indices, got_scores = engine.extract(pq[9:40], pc[17:290], scope, scorer=scorer, k=5)
    assert_rows((indices, got_scores.view(np.uint64)), expected_rows(scores[9:40, 17:290], LARGER_IS_BETTER[scorer], 5), f"{scorer} views")


@pytest.mark.gpu
def test_slices(request, sw, scope):
    """The same batch with the slice lowered to 4096 pairs (the test library's hook): two query blocks (64 + 6 rows) x five candidate
    slices (4 x 64 + 44 columns), the best candidate of row 30 in the first slice and of row 31 in the last. The rows equal those of the
    walk in one slice and the reference; with profiling on the call reports the kernels of every slice."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV), test_library=True):
        return
    assert sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    for utf8 in (False, True):
        engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
        qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
        osa, lcs, M, t, prefix, m, n = word_batch_counts(utf8)
        for scorer in SCORERS:
            scores = word_batch_scores(utf8, scorer)
            for k in (1, 5, 64):
                want = expected_rows(scores, LARGER_IS_BETTER[scorer], k)
                assert [int(want[0][row, 0]) for row in PLANTED_ROWS] == list(PLANTED_COLUMNS)
                os.environ.pop(HOOK, None)
                whole = run_extract(sw, scope, engine, qs, cs, "prepared", scorer=scorer, k=k)
                os.environ[HOOK] = "4096"
                scope.set_profiling(True)
                try:
                    sliced = run_extract(sw, scope, engine, qs, cs, "prepared", scorer=scorer, k=k)
                    timing = scope.last_timing()
                finally:
                    scope.set_profiling(False)
                    os.environ.pop(HOOK, None)
                assert_rows(sliced, whole, f"{scorer} utf8={utf8} k={k}: sliced against whole")
                assert_rows(sliced, want, f"{scorer} utf8={utf8} k={k}: sliced against the reference")
                family = {"osa": "osa", "jaro": "jaro", "jaro_winkler": "jaro"}.get(scorer, "lcs") + ("_u32" if utf8 else "")
                assert timing["dominant_name"] == f"extract_select/{family}", timing
                # 2 x 5 slices of a sizes kernel, a scoring kernel and a fold, and the two length passes
                assert timing["kernels"] == 2 * 5 * 3 + 2 and timing["cells"] == int(m.sum()) * int(n.sum()), timing


@pytest.mark.gpu
def test_ties(request, sw, scope):
    """Five distinct candidates repeated 200 times over: equal scores straddle the chunks of 64 columns and, with the slice lowered to
    1024 pairs (16 rows x 64 columns), the slices. Every row takes the lowest indices."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV), test_library=True):
        return
    engine = sw.LevenshteinDistances(capabilities=scope)
    distinct = ["martha", "marhta", "martha jones", "dwayne", ""]
    candidates = [distinct[(i * 7) % 5] for i in range(200)]
    queries = ["martha", "duane", "", "marth"] * 5
    counts = reference_counts(queries, candidates)
    for scorer in SCORERS:
        scores = reference_scores(scorer, counts)
        for k in (1, 5, 64):
            want = expected_rows(scores, LARGER_IS_BETTER[scorer], k)
            # (the helper's rows are what the test is about: a run of equal scores holds the lowest indices with that score, ascending)
            for i in range(len(queries)):
                row_i, row_s = want[0][i], want[1][i]
                for value in set(row_s.tolist()) - {PAD_BITS}:
                    held, every = row_i[row_s == value], np.nonzero(scores[i].view(np.uint64) == value)[0]
                    assert held.tolist() == every[:len(held)].tolist()
            for hook in (None, "1024"):
                os.environ.pop(HOOK, None)
                if hook:
                    os.environ[HOOK] = hook
                try:
                    got = run_extract(sw, scope, engine, as_items(queries, False), as_items(candidates, False), "strs", scorer=scorer, k=k)
                finally:
                    os.environ.pop(HOOK, None)
                assert_rows(got, want, f"{scorer} k={k} hook={hook}")


@pytest.mark.gpu
def test_wide_key(sw, scope, lev):
    """Two candidates whose Jaro scores differ as float64 and coincide as float32, the better one second: k = 1 names it."""
    query, candidates = wide_key_strings()
    scores = reference_scores("jaro", reference_counts([query], candidates))
    for form in ("strs", "prepared"):
        for k in (1, 2):
            got = run_extract(sw, scope, lev, [query.encode()], [c.encode() for c in candidates], form, scorer="jaro", k=k)
            assert_rows(got, expected_rows(scores, True, k), f"wide key {form} k={k}")
            assert int(got[0][0, 0]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1, 0.25])
def test_jaro_winkler_prefix_weights(sw, scope, lev, lev8, p):
    """The word batch has candidates on both sides of jaro > 0.7 and common prefixes of four (and longer: the count stops at four),
    and -- checked here -- pairs for which a contracted multiply-add gives another last bit than the expression as written."""
    for utf8, engine in ((False, lev), (True, lev8)):
        qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
        counts = word_batch_counts(utf8)
        if p == 0.1:   # (at 0.25 the product l * p is exact and 0.25, 0.5 and 1.0 times anything is too: few pairs can tell, if any)
            assert fused_differs(tuple(x[:12] for x in counts[:5]) + (counts[5][:12], counts[6]), p) > 0
        scores = word_batch_scores(utf8, "jaro_winkler", p)
        for k in (1, 5, 64):
            got = run_extract(sw, scope, engine, qs, cs, "prepared", scorer="jaro_winkler", k=k, prefix_weight=p)
            assert_rows(got, expected_rows(scores, True, k), f"jaro_winkler p={p} utf8={utf8} k={k}")
    longer = reference_counts(["prefixes"], ["prefixed", "prefix", "prefab", "pxefixes"])
    assert longer[4].tolist() == [[4, 4, 4, 1]]
    got = run_extract(sw, scope, lev, [b"prefixes"], [b"prefixed", b"prefix", b"prefab", b"pxefixes"], scorer="jaro_winkler", k=4, prefix_weight=p)
    assert_rows(got, expected_rows(reference_scores("jaro_winkler", longer, p), True, 4), f"long prefixes p={p}")


@pytest.mark.gpu
def test_cutoffs_and_empty_strings(sw, scope, lev, lev8):
    """A cutoff equal to an occurring score admits it (a distance scorer and a similarity scorer, and the rest too), rows are padded
    where fewer than k pass; empty strings on one side and on both under every scorer, `ratio` 100.0 and `jaro` 1.0 for two of them."""
    qs, cs = (as_items(side, False) for side in word_batch(False))
    for scorer in SCORERS:
        scores = word_batch_scores(False, scorer)
        larger = LARGER_IS_BETTER[scorer]
        ranked = np.sort(scores[5])[::-1] if larger else np.sort(scores[5])   # row 5, best first
        padded = kept = False
        for cutoff in (float(ranked[0]), float(ranked[9]), float(ranked[40])):
            for k in (5, 64):
                want = expected_rows(scores, larger, k, cutoff)
                if k == 64:   # (fewer than 64 candidates of row 5 are strictly better: the ones at the cutoff are in the row)
                    assert (want[1].view(np.float64)[5] == cutoff).any()
                padded, kept = padded or bool((want[0] == PAD_INDEX).any()), kept or bool((want[0] != PAD_INDEX).any())
                got = run_extract(sw, scope, lev, qs, cs, "prepared", scorer=scorer, k=k, cutoff=cutoff)
                assert_rows(got, want, f"{scorer} cutoff={cutoff!r} k={k}")
        assert padded and kept
        got = run_extract(sw, scope, lev, qs, cs, "strs", scorer=scorer, k=3, cutoff=float("inf") if larger else 0.0)   # nothing / exact copies only
        assert_rows(got, expected_rows(scores, larger, 3, float("inf") if larger else 0.0), f"{scorer} strictest cutoff")
    for utf8, engine in ((False, lev), (True, lev8)):
        for queries, candidates in ((["", "abc"], ["", "abd", ""]), ([""], ["", ""]), (["", ""], ["ab", "é" if utf8 else "e"]), (["ab"], [""])):
            counts = reference_counts(queries, candidates, utf8)
            for scorer in SCORERS:
                scores = reference_scores(scorer, counts)
                got = run_extract(sw, scope, engine, as_items(queries, utf8), as_items(candidates, utf8), scorer=scorer, k=3)
                assert_rows(got, expected_rows(scores, LARGER_IS_BETTER[scorer], 3), f"{scorer} {queries} {candidates} utf8={utf8}")
                if scorer in ("ratio", "jaro") and queries[0] == "" and candidates[0] == "":
                    assert got[1].view(np.float64)[0, 0] == (100.0 if scorer == "ratio" else 1.0)


@pytest.mark.gpu
def test_edges_and_refusals(sw, scope, lev, lev8):
    qs, cs = [b"martha", b"dwayne"], [b"marhta", b"duane", b"martha"]
    counts = reference_counts([q.decode() for q in qs], [c.decode() for c in cs])
    for scorer in SCORERS:
        scores, larger = reference_scores(scorer, counts), LARGER_IS_BETTER[scorer]
        # no queries: nothing is written; no candidates, fewer candidates than k: padding
        indices, values = lev.extract([], cs, scope, scorer=scorer, k=4)
        assert indices.shape == (0, 4) and values.shape == (0, 4)
        assert_rows(run_extract(sw, scope, lev, qs, [], scorer=scorer, k=4), expected_rows(np.zeros((2, 0)), larger, 4), f"{scorer} no candidates")
        assert_rows(run_extract(sw, scope, lev, qs, cs, scorer=scorer, k=7), expected_rows(scores, larger, 7), f"{scorer} nc < k")
        # the self-search, diagonal included
        own = reference_scores(scorer, reference_counts([c.decode() for c in cs], [c.decode() for c in cs]))
        for form in ("strs", "prepared"):
            assert_rows(run_extract(sw, scope, lev, cs, None, form, scorer=scorer, k=3), expected_rows(own, larger, 3), f"{scorer} self {form}")

    def refused(engine, queries, candidates, scorer, k, cutoff, p, status, utf8=False, words=()):
        indices, values = np.full((len(queries), 64), 0xA5A5A5A5, dtype=np.uint32), np.full((len(queries), 64), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        got, message = raw_extract(sw, engine, scope, queries, candidates, scorer, k, cutoff, p, indices, values, utf8)
        assert got == status and message and all(word in message for word in words), (got, message, status)
        assert (indices == 0xA5A5A5A5).all() and (values == 0xA5A5A5A5A5A5A5A5).all(), (status, message)

    inf = float("inf")
    refused(lev, qs, cs, 4, 0, 0.0, 0.1, "invalid_argument")
    refused(lev, qs, cs, 4, 65, 0.0, 0.1, "invalid_argument")
    refused(lev, qs, cs, 6, 2, 0.0, 0.1, "invalid_argument")
    refused(lev, qs, cs, -1, 2, 0.0, 0.1, "invalid_argument")
    for scorer in range(6):
        refused(lev, qs, cs, scorer, 2, float("nan"), 0.1, "invalid_argument")
        refused(lev, qs, cs, scorer, 2, -1.0, 0.1, "invalid_argument")
        refused(lev, qs, cs, scorer, 2, -inf, 0.1, "invalid_argument")
    refused(lev, qs, cs, 5, 2, 0.0, 0.3, "invalid_argument")
    refused(lev, qs, cs, 5, 2, 0.0, -0.1, "invalid_argument")
    refused(lev, qs, cs, 5, 2, 0.0, float("nan"), "invalid_argument")
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    for scorer in range(6):
        refused(costly, qs, cs, scorer, 2, inf if scorer < 2 else 0.0, 0.1, "not_implemented")
        refused(lev8, qs, [b"ok", b"\xff\xfe"], scorer, 2, inf if scorer < 2 else 0.0, 0.1, "invalid_utf8", utf8=True)
        refused(lev8, [b"\xc3"], cs, scorer, 2, inf if scorer < 2 else 0.0, 0.1, "invalid_utf8", utf8=True)
    # the families' length limits, before any output is written: the message names a pair and both lengths
    long_q, long_c = [b"ab", b"a" * 2049], [b"abc", b"b" * 5, b"c" * 2049]
    for scorer in range(4):   # OSA, Indel, LCS, ratio: the SHORTER string of a pair is over the limit only when both are long
        refused(lev, long_q, long_c, scorer, 2, inf if scorer < 2 else 0.0, 0.1, "unsupported_length", words=("(1, 2)", "2049 x 2049"))
    for scorer in (4, 5):     # Jaro: either string
        refused(lev, long_q, cs, scorer, 2, 0.0, 0.1, "unsupported_length", words=("(1, 0)", "2049 x 6"))
        refused(lev, qs, long_c, scorer, 2, 0.0, 0.1, "unsupported_length", words=("(0, 2)", "6 x 2049"))
    with pytest.raises(sw.StringWarsError) as info:
        lev.extract(long_q, long_c, scope, scorer="ratio", k=1)
    assert info.value.status == "unsupported_length"
    # one long side is within the limit of the first four scorers: 2049 symbols against short candidates (and the other way round)
    counts = reference_counts(["ab", "a" * 2049], ["abc", "b" * 5, "aab"])
    for scorer in SCORERS[:4]:
        want = expected_rows(reference_scores(scorer, counts), LARGER_IS_BETTER[scorer], 2)
        assert_rows(run_extract(sw, scope, lev, long_q, [b"abc", b"b" * 5, b"aab"], scorer=scorer, k=2), want, f"{scorer} one long side")
    # the Python layer's own argument checks
    with pytest.raises(ValueError):
        lev.extract(qs, cs, scope, scorer="levenshtein", k=2)
    with pytest.raises(ValueError):
        lev.extract(qs, cs, scope, scorer="jaro", k=2, out=(np.zeros((2, 2), np.uint32), np.zeros((2, 2), np.float32)))
    import torch
    for rows, dtype in ((1, torch.float64), (2, torch.float32)):   # a device tensor too small for the rows, or of another width: refused, not overrun
        with pytest.raises(ValueError):
            lev.extract(qs, cs, scope, scorer="jaro", k=2, out=(torch.zeros((2, 2), dtype=torch.int32, device="cuda"), torch.zeros((rows, 2), dtype=dtype, device="cuda")))
    with pytest.raises(sw.StringWarsError):
        lev.extract(qs, cs, scope, scorer="jaro_winkler", k=2, prefix_weight=0.3)
    assert_rows(run_extract(sw, scope, lev, qs, cs, scorer="ratio", k=2, prefix_weight=0.3),   # (ignored by the other scorers)
                expected_rows(reference_scores("ratio", reference_counts(["martha", "dwayne"], ["marhta", "duane", "martha"])), True, 2), "ratio ignores p")


@pytest.mark.gpu
def test_agreement_with_the_dense_calls(sw, scope, lev):
    """200 x 500: the search equals the dense calls followed by the same selection on the host -- the device evaluation held to the
    shipped host expressions (engines.py) directly, scorer by scorer."""
    rng = np.random.default_rng(77)
    draw = lambda: int(rng.integers(97, 103))
    bases = [bytes(draw() for _ in range(int(size))) for size in rng.integers(0, 48, 40)]
    words = lambda count: [bytes(mutated(rng, bases[int(rng.integers(0, 40))], int(rng.integers(0, 4)), draw)) for _ in range(count)]
    qs, cs = words(200), words(500)
    pq, pc = sw.PreparedTape(scope, sw.Strs(qs)), sw.PreparedTape(scope, sw.Strs(cs))
    dense = {"osa": lev.osa_cross(pq, pc, scope).astype(np.float64), "indel": lev.indel_cross(pq, pc, scope).astype(np.float64),
             "lcs": lev.lcs_cross(pq, pc, scope).astype(np.float64), "ratio": lev.ratio_cross(pq, pc, scope),
             "jaro": lev.jaro_cross(pq, pc, scope), "jaro_winkler": lev.jaro_winkler_cross(pq, pc, scope, prefix_weight=0.1)}
    for scorer in SCORERS:
        for k, cutoff in ((1, None), (10, None), (64, float(np.median(dense[scorer])))):
            indices, scores = lev.extract(pq, pc, scope, scorer=scorer, k=k, cutoff=cutoff)
            assert_rows((indices, scores.view(np.uint64)), expected_rows(dense[scorer], LARGER_IS_BETTER[scorer], k, cutoff), f"{scorer} k={k} cutoff={cutoff}")


@pytest.mark.gpu
def test_seeded_random_round(request, sw, scope):
    """A dozen draws of scorer, k, cutoff, prefix weight, tape form, output memory and slice (the hook) on batches of a few hundred pairs."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV), test_library=True):
        return
    rng = np.random.default_rng(2026)
    engines = {False: sw.LevenshteinDistances(capabilities=scope), True: sw.LevenshteinDistancesUTF8(capabilities=scope)}
    for draw_index in range(12):
        utf8 = bool(rng.integers(0, 2))
        alphabet = list("aé中bc") if utf8 else list("abcd")
        draw = lambda: alphabet[int(rng.integers(0, len(alphabet)))]
        bases = ["".join(draw() for _ in range(int(size))) for size in rng.integers(0, 70, 6)]
        word = lambda: "".join(mutated(rng, bases[int(rng.integers(0, 6))], int(rng.integers(0, 4)), draw))
        queries, candidates = [word() for _ in range(int(rng.integers(1, 20)))], [word() for _ in range(int(rng.integers(1, 90)))]
        scorer = SCORERS[draw_index % 6]
        k, p = int(rng.choice([1, 2, 7, 33, 64])), float(rng.choice([0.0, 0.05, 0.1, 0.25]))
        scores = reference_scores(scorer, reference_counts(queries, candidates, utf8), p)
        cutoff = None if rng.integers(0, 2) else float(rng.choice(scores.ravel()))
        form, device_out = str(rng.choice(["strs", "strs32", "device", "prepared", "prepared32"])), bool(rng.integers(0, 2))
        hook = [None, "1", "64", "100", "640", "4096"][int(rng.integers(0, 6))]
        os.environ.pop(HOOK, None)
        if hook:
            os.environ[HOOK] = hook
        try:
            got = run_extract(sw, scope, engines[utf8], as_items(queries, utf8), as_items(candidates, utf8), form, device_out, scorer=scorer, k=k,
                              cutoff=cutoff, prefix_weight=p)
        finally:
            os.environ.pop(HOOK, None)
        assert_rows(got, expected_rows(scores, LARGER_IS_BETTER[scorer], k, cutoff),
                    f"draw {draw_index}: {scorer} utf8={utf8} k={k} p={p} cutoff={cutoff!r} {form} device_out={device_out} hook={hook} "
                    f"{len(queries)} x {len(candidates)}")


@pytest.mark.gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_cpp_wrappers_against_the_reference(tmp_path, utf8):
    """Both overloads of LevenshteinDistances::extract (stringwars_amd.hpp) from a C++ program: raw tape views and prepared tapes, every
    scorer, `no_cutoff(scorer)` and a cutoff that occurs, two prefix weights, candidates and the self-search (a null pointer) -- the
    doubles cross as the wrapper's own bit copies. The rows the program writes equal the reference bit for bit."""
    binary = build_check_extract(tmp_path)
    qs, cs = word_batch(utf8)
    own_counts = reference_counts(list(qs), list(qs), utf8)
    requests, wants = [], []
    for scorer_id, scorer in enumerate(SCORERS):
        larger = LARGER_IS_BETTER[scorer]
        scores, own = word_batch_scores(utf8, scorer), reference_scores(scorer, own_counts)
        cutoff = float(np.sort(scores[5])[::-1][20] if larger else np.sort(scores[5])[20])
        for prepared in (0, 1):
            requests += [(scorer_id, prepared, 0, 5, None, 0.1), (scorer_id, prepared, 0, 64, cutoff, 0.1), (scorer_id, prepared, 1, 3, None, 0.1)]
            wants += [expected_rows(scores, larger, 5), expected_rows(scores, larger, 64, cutoff), expected_rows(own, larger, 3)]
    for prepared in (0, 1):
        requests.append((5, prepared, 0, 7, None, 0.25))
        wants.append(expected_rows(word_batch_scores(utf8, "jaro_winkler", 0.25), True, 7))
    write_extract_case(tmp_path / "batch.case", utf8, qs, cs, requests)
    done = subprocess.run([str(binary), str(tmp_path / "batch.case"), str(tmp_path / "batch.out")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    raw = open(tmp_path / "batch.out", "rb").read()
    at = 0
    for request, want in zip(requests, wants):
        k = request[3]
        indices = np.frombuffer(raw, dtype=np.uint32, count=len(qs) * k, offset=at).reshape(len(qs), k)
        at += indices.nbytes
        bits = np.frombuffer(raw, dtype=np.uint64, count=len(qs) * k, offset=at).reshape(len(qs), k)
        at += bits.nbytes
        assert_rows((indices, bits), want, f"C++ extract utf8={utf8} request {request}")
    assert at == len(raw)
