"""The score range search (swh_levenshtein_extract_within_*, engine.extract_within): every candidate of every query whose OSA, Indel,
LCS, ratio, Jaro or Jaro-Winkler score passes a cutoff, as CSR rows, against the pure-Python references of tests/test_extract.py.

The expected result of a call is, per row, the ascending indices where the reference score passes the cutoff, and those scores as
uint64 patterns. Every comparison is exact: offsets equal, indices equal, scores equal as 64-bit patterns."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child
from test_extract import (HOOK, INCLUDE, LARGER_IS_BETTER, PACKAGE, ROOT, SCORERS, as_items, expected_rows, fused_differs, reference_counts,
                          reference_scores, tapes, word_batch, word_batch_counts, word_batch_scores)

WITHIN_SYMBOLS = ("swh_levenshtein_extract_within_u64tape", "swh_levenshtein_utf8_extract_within_u64tape",
                  "swh_levenshtein_extract_within_prepared")
SENTINEL32, SENTINEL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
PAD_INDEX = 0xFFFFFFFF


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def expected_within(scores, larger_is_better, cutoff):
    """(offsets uint64, indices uint32, score patterns uint64): per row the ascending indices whose score passes the cutoff."""
    scores = np.asarray(scores, dtype=np.float64)
    hit = scores >= cutoff if larger_is_better else scores <= cutoff
    offsets = np.zeros(scores.shape[0] + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(hit.sum(axis=1))
    return offsets, np.nonzero(hit)[1].astype(np.uint32), scores[hit].view(np.uint64)   # (row-major: ascending within a row)


def batch_cutoffs(scores, larger_is_better):
    """(loose, tight), both values that occur in the matrix: its median score, and the one at the best 3 %."""
    ranked = np.sort(np.asarray(scores).ravel())
    if larger_is_better:
        ranked = ranked[::-1]   # best first
    return float(ranked[ranked.size // 2]), float(ranked[int(0.03 * ranked.size)])


@functools.lru_cache(maxsize=None)
def word_batch_cutoffs(utf8, scorer):
    return batch_cutoffs(word_batch_scores(utf8, scorer), LARGER_IS_BETTER[scorer])


def run_within(sw, scope, engine, queries, candidates, form="strs", device_out=False, room=None, **kw):
    """engine.extract_within on one tape form, into host arrays or device tensors of `room` entries (sentinel-filled):
    (offsets uint64, indices uint32, score patterns uint64), the last two cut at the total -- and, for device tensors, the untouched
    tail checked here."""
    q, c = tapes(sw, scope, engine, queries, candidates, form)
    if not device_out:
        found = engine.extract_within(q, c, scope, **kw)
        return np.asarray(found.offsets), found.indices, found.scores.view(np.uint64)
    import torch
    offsets = torch.full((len(queries) + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    indices = torch.full((room,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    scores = torch.full((room,), 7.0, dtype=torch.float64, device="cuda")
    found = engine.extract_within(q, c, scope, out=(offsets, indices, scores), **kw)
    torch.cuda.synchronize()
    total = int(found.offsets[-1])
    assert len(found.indices) == total and (indices[total:] == 0x5A5A5A5A).all() and (scores[total:] == 7.0).all()
    return offsets.cpu().numpy().view(np.uint64), indices.cpu().numpy().view(np.uint32)[:total], scores.cpu().numpy().view(np.uint64)[:total]


def assert_csr(got, want, what):
    (got_o, got_i, got_s), (want_o, want_i, want_s) = got, want
    assert np.array_equal(np.asarray(got_o, dtype=np.uint64), want_o), f"{what}: row offsets differ: {np.asarray(got_o)[:8]} ... want {want_o[:8]} ..."
    assert got_i.shape == want_i.shape and got_s.shape == want_s.shape, what
    bad = np.nonzero((got_i != want_i) | (got_s != want_s))[0]
    if len(bad):
        at = int(bad[0])
        row = int(np.searchsorted(want_o, at, side="right")) - 1
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {at} (row {row}): got index {int(got_i[at])} score "
                             f"{got_s[at:at + 1].view(np.float64)[0]!r}, want index {int(want_i[at])} score {want_s[at:at + 1].view(np.float64)[0]!r}")


def raw_within(sw, engine, scope, queries, candidates, scorer, cutoff, p, offsets, indices, scores, capacity, utf8=False):
    """The C ABI itself on raw u64 tapes; an output may be None (a null pointer). Returns (status name, message)."""
    from stringwars_amd import _native as N
    tq, _, keep_q = sw.engines._c_tape(sw.Strs(queries), want64=True)
    tc, _, keep_c = sw.engines._c_tape(sw.Strs(candidates), want64=True) if candidates is not None else (None, None, None)
    fn = N.lib.swh_levenshtein_utf8_extract_within_u64tape if utf8 else N.lib.swh_levenshtein_extract_within_u64tape
    bits = [C.c_uint64(int(np.float64(value).view(np.uint64))) for value in (cutoff, p)]
    pointer = lambda array: C.c_void_p(None if array is None else array.ctypes.data)
    err = C.c_char_p()
    status = fn(engine._handle, scope.handle, C.byref(tq), C.byref(tc) if tc is not None else None, scorer, bits[0], bits[1],
                pointer(offsets), pointer(indices), pointer(scores), capacity, C.byref(err))
    return N.STATUS_NAMES[status], (err.value or b"").decode()


# ---- CPU: the surface, the reference, the batch ------------------------------------------------------------------------------------------
def test_abi_exports_and_python_surface(sw):
    from stringwars_amd import _native as N
    shipped, test_library = C.CDLL(sw.LIBRARY_PATH), C.CDLL(TEST_LIBRARY_ENV["STRINGWARS_AMD_LIBRARY"])
    for name in WITHIN_SYMBOLS:
        assert hasattr(shipped, name) and hasattr(test_library, name) and name in N.SIGNATURES, name
    assert "extract_within" in sw.capabilities().split(",")
    for cls in (sw.LevenshteinDistances, sw.LevenshteinDistancesUTF8):
        assert callable(getattr(cls, "extract_within"))
    found = sw.ScoreMatches(np.array([0, 2, 2, 3], dtype=np.uint64), np.array([1, 4, 0], dtype=np.uint32), np.array([0.5, 1.0, 0.25]))
    assert len(found) == 3 and found.counts.tolist() == [2, 0, 1]
    assert [x.tolist() for x in found.row(0)] == [[1, 4], [0.5, 1.0]] and [x.tolist() for x in found.row(-1)] == [[0], [0.25]]
    assert [x.tolist() for x in found.pairs()] == [[0, 0, 2], [1, 4, 0], [0.5, 1.0, 0.25]]
    assert [x.tolist() for x in found.pairs(upper=True)] == [[0, 0], [1, 4], [0.5, 1.0]]
    counted = sw.ScoreMatches(np.array([0, 2], dtype=np.uint64), None, None)
    assert counted.counts.tolist() == [2]
    with pytest.raises(ValueError):
        counted.row(0)
    with pytest.raises(ValueError):
        sw.ScoreMatches(np.array([0, 2], dtype=np.uint64), np.zeros(2, np.uint32), None)
    # null handles fail loudly: no device -- or, where there is one, null handles -- a message, and nothing written
    import torch
    want = "invalid_argument" if torch.cuda.is_available() else "no_device"
    tape, _, keep = sw.engines._c_tape(sw.Strs([b"abc"]), want64=True)
    view = N.PreparedView(None, 0, 1)
    for name in WITHIN_SYMBOLS:
        offsets, indices, scores = (np.full(16, 0xA5, dtype=np.uint8) for _ in range(3))
        side = C.byref(view) if name.endswith("prepared") else C.byref(tape)
        err = C.c_char_p()
        status = getattr(N.lib, name)(None, None, side, side, 4, 0, 0, C.c_void_p(offsets.ctypes.data), C.c_void_p(indices.ctypes.data),
                                      C.c_void_p(scores.ctypes.data), 1, C.byref(err))
        assert N.STATUS_NAMES[status] == want and err.value, (name, status)
        assert (offsets == 0xA5).all() and (indices == 0xA5).all() and (scores == 0xA5).all(), name
    with pytest.raises(ValueError):
        sw.LevenshteinDistances.extract_within(None, [b"a"], None, None, scorer="jaro", cutoff=0.5)   # (no scope: refused before anything is touched)


def test_expected_within_on_the_worked_row():
    """The header's worked row through the references and the CSR helper; a hand-written case with an empty row."""
    scores = reference_scores("jaro_winkler", reference_counts(["MARTHA"], ["MARHTA", "DWAYNE", "MARTHA", "MARTHA"]))
    offsets, indices, bits = expected_within(scores, True, 0.97)
    assert offsets.tolist() == [0, 2] and indices.tolist() == [2, 3] and bits.view(np.float64).tolist() == [1.0, 1.0]
    offsets, indices, bits = expected_within(scores, True, 0.9611111111111111)
    assert offsets.tolist() == [0, 3] and indices.tolist() == [0, 2, 3] and bits.view(np.float64).tolist() == [0.9611111111111111, 1.0, 1.0]
    offsets, indices, bits = expected_within(np.array([[2.0, 1.0, 3.0], [5.0, 4.0, 6.0], [1.0, 1.0, 0.0]]), False, 1.0)
    assert offsets.tolist() == [0, 1, 1, 4] and indices.tolist() == [1, 0, 1, 2] and bits.view(np.float64).tolist() == [1.0, 1.0, 1.0, 0.0]
    assert expected_within(np.zeros((2, 0)), True, 0.0)[0].tolist() == [0, 0, 0]
    assert batch_cutoffs(np.arange(100.0).reshape(10, 10), True) == (49.0, 96.0) and batch_cutoffs(np.arange(100.0), False) == (50.0, 3.0)


def test_the_word_batch_and_its_cutoffs_reach_what_they_are_for():
    """On the reference alone: over the cases of the GPU tests (every scorer, both forms, the loose and the tight cutoff) there are
    rows without a hit, rows with more than 64 (what extract's k cannot hold), scores exactly at the cutoff, hits in columns 63 and 64
    of one row (both sides of a seam between chunks of 64 columns, and between the slices of the lowered hook), and totals that
    differ between the two cutoffs."""
    empty_rows = long_rows = at_cutoff = seams = 0
    for utf8 in (False, True):
        for scorer in SCORERS:
            scores, larger = word_batch_scores(utf8, scorer), LARGER_IS_BETTER[scorer]
            totals = []
            for cutoff in word_batch_cutoffs(utf8, scorer):
                assert (scores == cutoff).any(), (scorer, utf8, cutoff)   # taken from the batch: "at the cutoff" is hit by construction
                offsets, indices, bits = expected_within(scores, larger, cutoff)
                counts = np.diff(offsets.astype(np.int64))
                hit = scores >= cutoff if larger else scores <= cutoff
                empty_rows += int((counts == 0).sum())
                long_rows += int((counts > 64).sum())
                at_cutoff += int((bits.view(np.float64) == cutoff).sum())
                seams += sum(int((hit[:, edge - 1] & hit[:, edge]).sum()) for edge in (64, 128, 192, 256))
                totals.append(int(offsets[-1]))
            assert totals[0] > totals[1] > 0, (scorer, utf8, totals)
    assert empty_rows > 0 and long_rows > 0 and at_cutoff > 0 and seams > 0, (empty_rows, long_rows, at_cutoff, seams)


# ---- the C++ wrappers: a program of their own ---------------------------------------------------------------------------------------------
def build_check_extract_within(tmp_path):
    """tests/bindings/check_extract_within.cpp against include/stringwars_amd.hpp and the shipped library."""
    binary = tmp_path / "check_extract_within"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE,
                    os.path.join(ROOT, "tests", "bindings", "check_extract_within.cpp"), "-o", str(binary), "-L", PACKAGE, "-lstringwars_amd",
                    f"-Wl,-rpath,{PACKAGE}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True, timeout=300)
    return binary


def write_within_case(path, utf8, queries, candidates, requests):
    """The case file of check_extract_within.cpp; `requests`: (scorer id, prepared, self, cutoff, prefix weight)."""
    with open(path, "wb") as out:
        out.write(struct.pack("<i", int(utf8)))
        for side in (queries, candidates):
            items = [s.encode() for s in side]
            offsets = np.zeros(len(items) + 1, dtype=np.uint64)
            np.cumsum([len(s) for s in items], out=offsets[1:])
            out.write(struct.pack("<Q", len(items)) + offsets.tobytes() + b"".join(items))
        out.write(struct.pack("<I", len(requests)))
        for scorer, prepared, own, cutoff, p in requests:
            out.write(struct.pack("<iiidd", scorer, int(prepared), int(own), cutoff, p))


def test_cpp_program_builds_and_fails_loudly_without_a_device(tmp_path):
    """The wrappers' program compiles against the header with warnings as errors; where no device is visible it ends with the
    library's status (no_device) on stderr and writes no result."""
    import torch
    binary = build_check_extract_within(tmp_path)
    if torch.cuda.is_available():
        return   # (with a device the program is run by test_cpp_wrappers_against_the_reference)
    write_within_case(tmp_path / "tiny.case", False, ["martha"], ["marhta"], [(5, 0, 0, 0.9, 0.1)])
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
    """70 x 300 mutated words of 0 .. 80 symbols at the loose and the tight cutoff: raw tapes, device tapes and prepared tapes, into
    host arrays (the loose total is over the default capacity: the exact retry) and into device tensors a little larger than the
    total (the tail stays as it was), and views of prepared tapes."""
    engine = lev8 if utf8 else lev
    qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
    scores, larger = word_batch_scores(utf8, scorer), LARGER_IS_BETTER[scorer]
    for cutoff in word_batch_cutoffs(utf8, scorer):
        want = expected_within(scores, larger, cutoff)
        for form in ("strs", "device", "prepared"):
            for device_out in (False, True):
                got = run_within(sw, scope, engine, qs, cs, form, device_out, room=len(want[1]) + 3, scorer=scorer, cutoff=cutoff)
                assert_csr(got, want, f"{scorer} utf8={utf8} cutoff={cutoff!r} {form} device_out={device_out}")
    # views of prepared tapes: rows 9 .. 40 against candidates 17 .. 290 (indices count from the view's first candidate)
    pq, pc = tapes(sw, scope, engine, qs, cs, "prepared")
    cutoff = word_batch_cutoffs(utf8, scorer)[0]
    found = engine.extract_within(pq[9:40], pc[17:290], scope, scorer=scorer, cutoff=cutoff)
    assert_csr((found.offsets, found.indices, found.scores.view(np.uint64)), expected_within(scores[9:40, 17:290], larger, cutoff), f"{scorer} views")


@pytest.mark.gpu
def test_slices_and_blocks(request, sw, scope):
    """The same batch with the slice lowered (the test library's hook). 4096 pairs: two query blocks (64 + 6 rows) x five candidate
    slices (4 x 64 + 44 columns); 640 pairs: seven blocks of 10 rows x the same five slices. A row's cursor crosses every slice: the
    results equal those of the walk in one slice and the reference; with profiling on the call reports the kernels of both walks
    and counts the cells once."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV), test_library=True):
        return
    assert sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    for utf8 in (False, True):
        engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
        qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
        osa, lcs, M, t, prefix, m, n = word_batch_counts(utf8)
        for scorer in SCORERS:
            scores, larger = word_batch_scores(utf8, scorer), LARGER_IS_BETTER[scorer]
            for cutoff in word_batch_cutoffs(utf8, scorer):
                want = expected_within(scores, larger, cutoff)
                total = int(want[0][-1])
                os.environ.pop(HOOK, None)
                whole = run_within(sw, scope, engine, qs, cs, "prepared", scorer=scorer, cutoff=cutoff, capacity=total)
                assert_csr(whole, want, f"{scorer} utf8={utf8} cutoff={cutoff!r}: whole against the reference")
                for hook, blocks in (("4096", 2), ("640", 7)):
                    os.environ[HOOK] = hook
                    scope.set_profiling(True)
                    try:
                        sliced = run_within(sw, scope, engine, qs, cs, "prepared", scorer=scorer, cutoff=cutoff, capacity=total)
                        timing = scope.last_timing()
                    finally:
                        scope.set_profiling(False)
                        os.environ.pop(HOOK, None)
                    assert_csr(sliced, whole, f"{scorer} utf8={utf8} cutoff={cutoff!r} hook={hook}: sliced against whole")
                    family = {"osa": "osa", "jaro": "jaro", "jaro_winkler": "jaro"}.get(scorer, "lcs") + ("_u32" if utf8 else "")
                    assert timing["dominant_name"] == f"extract_within/{family}", timing
                    # two walks of blocks x 5 slices of a sizes kernel, a scoring kernel and the compaction; the two length passes; the scan's two
                    assert timing["kernels"] == 2 * blocks * 5 * 3 + 2 + 2 and timing["cells"] == int(m.sum()) * int(n.sum()), timing


@pytest.mark.gpu
def test_counting_protocol(sw, scope, lev):
    """A counting call writes the offsets only; with a capacity one below the total the offsets are full and the arrays untouched; a
    capacity equal to the total fills; one above leaves the tail untouched. Host arrays through the C ABI, device tensors and the
    retry through the Python layer."""
    qs, cs = (as_items(side, False) for side in word_batch(False))
    scores = word_batch_scores(False, "jaro_winkler")
    cutoff = word_batch_cutoffs(False, "jaro_winkler")[1]
    want = expected_within(scores, True, cutoff)
    total = int(want[0][-1])
    assert total > 70

    def fresh(room):
        return np.full(71, SENTINEL64, dtype=np.uint64), np.full(room, SENTINEL32, dtype=np.uint32), np.full(room, SENTINEL64, dtype=np.uint64)

    offsets, _, _ = fresh(0)
    assert raw_within(sw, lev, scope, qs, cs, 5, cutoff, 0.1, offsets, None, None, 0) == ("success", "")
    assert np.array_equal(offsets, want[0])
    offsets, indices, values = fresh(total + 5)
    assert raw_within(sw, lev, scope, qs, cs, 5, cutoff, 0.1, offsets, indices, values, total - 1) == ("success", "")
    assert np.array_equal(offsets, want[0]) and (indices == SENTINEL32).all() and (values == SENTINEL64).all()
    for capacity in (total, total + 5):
        offsets, indices, values = fresh(total + 5)
        assert raw_within(sw, lev, scope, qs, cs, 5, cutoff, 0.1, offsets, indices, values, capacity) == ("success", "")
        assert_csr((offsets, indices[:total], values[:total]), want, f"capacity {capacity}")
        assert (indices[total:] == SENTINEL32).all() and (values[total:] == SENTINEL64).all()
    # the Python layer: a capacity of one takes the retry; the counting form; arrays that are too small
    assert_csr(run_within(sw, scope, lev, qs, cs, scorer="jaro_winkler", cutoff=cutoff, capacity=1), want, "capacity=1")
    import torch
    for offsets in (np.zeros(71, dtype=np.uint64), torch.zeros(71, dtype=torch.int64, device="cuda")):
        counted = lev.extract_within(qs, cs, scope, scorer="jaro_winkler", cutoff=cutoff, out=(offsets, None, None))
        assert counted.indices is None and counted.scores is None and np.array_equal(counted.counts, np.diff(want[0]))
    for device in (False, True):
        offsets, indices, values = fresh(total - 1)
        if device:
            offsets, indices, values = (torch.from_numpy(x.view({4: np.int32, 8: np.int64}[x.itemsize])).cuda() for x in (offsets, indices, values))
        with pytest.raises(ValueError):
            lev.extract_within(qs, cs, scope, scorer="jaro_winkler", cutoff=cutoff, out=(offsets, indices, values.view(torch.float64) if device else values.view(np.float64)))
        if device:
            torch.cuda.synchronize()
            offsets, indices, values = (x.cpu().numpy() for x in (offsets, indices, values))
        assert np.array_equal(offsets.view(np.uint64), want[0]), "the offsets are written before the refusal"
        assert (indices.view(np.uint32) == SENTINEL32).all() and (values.view(np.uint64) == SENTINEL64).all()
    with pytest.raises(ValueError):   # one array without the other, a size that is not the other's, another width
        lev.extract_within(qs, cs, scope, scorer="jaro", cutoff=0.5, out=(np.zeros(71, np.uint64), np.zeros(8, np.uint32), None))
    with pytest.raises(ValueError):
        lev.extract_within(qs, cs, scope, scorer="jaro", cutoff=0.5, out=(np.zeros(71, np.uint64), np.zeros(8, np.uint32), np.zeros(9)))
    with pytest.raises(ValueError):
        lev.extract_within(qs, cs, scope, scorer="jaro", cutoff=0.5, out=(np.zeros(71, np.uint64), np.zeros(8, np.uint32), np.zeros(8, np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_agreement_with_extract_and_the_pairwise_calls(sw, scope, lev, lev8, utf8):
    """At the tight cutoffs every row of at most 64 hits, ordered best score first and then by index, is extract(k=64, cutoff)'s
    unpadded row -- the same pairs admitted, the same bits -- and a handful of hits carry the bits of the pairwise calls."""
    engine = lev8 if utf8 else lev
    qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
    pq, pc = tapes(sw, scope, engine, qs, cs, "prepared")
    compared = 0
    for scorer in SCORERS:
        larger = LARGER_IS_BETTER[scorer]
        cutoff = word_batch_cutoffs(utf8, scorer)[1]
        found = engine.extract_within(pq, pc, scope, scorer=scorer, cutoff=cutoff)
        top_i, top_s = engine.extract(pq, pc, scope, scorer=scorer, k=64, cutoff=cutoff)
        for row in range(len(qs)):
            indices, values = found.row(row)
            if len(indices) > 64:
                assert (top_i[row] != PAD_INDEX).all()
                continue
            order = np.argsort(-values if larger else values, kind="stable")   # (ascending indices: a stable sort breaks ties by index)
            kept = int((top_i[row] != PAD_INDEX).sum())
            assert kept == len(indices) and np.array_equal(top_i[row, :kept], indices[order]), (scorer, row)
            assert np.array_equal(top_s[row, :kept].view(np.uint64), values[order].view(np.uint64)), (scorer, row)
            compared += 1
        i, j, values = found.pairs()
        pick = np.linspace(0, len(i) - 1, 12).astype(np.int64)
        a, b = [qs[int(x)] for x in i[pick]], [cs[int(x)] for x in j[pick]]
        pairwise = {"osa": lambda: engine.osa(a, b, scope).astype(np.float64), "indel": lambda: engine.indel(a, b, scope).astype(np.float64),
                    "lcs": lambda: engine.lcs(a, b, scope).astype(np.float64), "ratio": lambda: engine.ratio(a, b, scope),
                    "jaro": lambda: engine.jaro(a, b, scope), "jaro_winkler": lambda: engine.jaro_winkler(a, b, scope, prefix_weight=0.1)}[scorer]()
        assert np.array_equal(pairwise.view(np.uint64), values[pick].view(np.uint64)), scorer
    assert compared > 100


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1, 0.25])
def test_jaro_winkler_prefix_weights(sw, scope, lev, lev8, p):
    """The word batch has pairs for which a contracted multiply-add gives another last bit than the expression as written (checked
    here at p = 0.1): the loose cutoff admits half the matrix, those pairs among them, with the reference's bits."""
    for utf8, engine in ((False, lev), (True, lev8)):
        qs, cs = (as_items(side, utf8) for side in word_batch(utf8))
        counts = word_batch_counts(utf8)
        if p == 0.1:   # (at 0.25 the product l * p is exact and 0.25, 0.5 and 1.0 times anything is too: few pairs can tell, if any)
            assert fused_differs(tuple(x[:12] for x in counts[:5]) + (counts[5][:12], counts[6]), p) > 0
        scores = word_batch_scores(utf8, "jaro_winkler", p)
        for cutoff in batch_cutoffs(scores, True) + (0.7,):
            got = run_within(sw, scope, engine, qs, cs, "prepared", scorer="jaro_winkler", cutoff=cutoff, prefix_weight=p)
            assert_csr(got, expected_within(scores, True, cutoff), f"jaro_winkler p={p} utf8={utf8} cutoff={cutoff!r}")
    longer = reference_counts(["prefixes"], ["prefixed", "prefix", "prefab", "pxefixes"])
    assert longer[4].tolist() == [[4, 4, 4, 1]]
    got = run_within(sw, scope, lev, [b"prefixes"], [b"prefixed", b"prefix", b"prefab", b"pxefixes"], scorer="jaro_winkler", cutoff=0.8, prefix_weight=p)
    assert_csr(got, expected_within(reference_scores("jaro_winkler", longer, p), True, 0.8), f"long prefixes p={p}")


@pytest.mark.gpu
def test_edges_and_refusals(sw, scope, lev, lev8):
    qs, cs = [b"martha", b"dwayne"], [b"marhta", b"duane", b"martha"]
    counts = reference_counts([q.decode() for q in qs], [c.decode() for c in cs])
    sample = {"osa": 2.0, "indel": 2.0, "lcs": 4.0, "ratio": 80.0, "jaro": 0.9, "jaro_winkler": 0.9}
    for scorer in SCORERS:
        scores, larger = reference_scores(scorer, counts), LARGER_IS_BETTER[scorer]
        # no queries: one offset; no candidates: every row empty
        found = lev.extract_within([], cs, scope, scorer=scorer, cutoff=sample[scorer])
        assert np.asarray(found.offsets).tolist() == [0] and len(found.indices) == 0 and len(found) == 0
        assert_csr(run_within(sw, scope, lev, qs, [], scorer=scorer, cutoff=sample[scorer]), expected_within(np.zeros((2, 0)), larger, 1.0), f"{scorer} no candidates")
        assert_csr(run_within(sw, scope, lev, qs, cs, scorer=scorer, cutoff=sample[scorer]), expected_within(scores, larger, sample[scorer]), f"{scorer} small")
        # the self-search: diagonal and both orientations; pairs(upper=True) holds each unordered pair once
        own = reference_scores(scorer, reference_counts([c.decode() for c in cs], [c.decode() for c in cs]))
        for form in ("strs", "prepared"):
            q, _ = tapes(sw, scope, lev, cs, None, form)
            found = lev.extract_within(q, None, scope, scorer=scorer, cutoff=sample[scorer])
            want = expected_within(own, larger, sample[scorer])
            assert_csr((found.offsets, found.indices, found.scores.view(np.uint64)), want, f"{scorer} self {form}")
            i, j, values = found.pairs(upper=True)
            hit = own >= sample[scorer] if larger else own <= sample[scorer]
            assert sorted(zip(i.tolist(), j.tolist())) == [(a, b) for a in range(3) for b in range(a + 1, 3) if hit[a, b]]
            assert all(hit[a, a] for a in range(3)) and len(found.pairs()[0]) == int(hit.sum())
    # empty strings on one side and on both under every scorer: ratio 100.0 and jaro 1.0 for two of them
    for utf8, engine in ((False, lev), (True, lev8)):
        for queries, candidates in ((["", "abc"], ["", "abd", ""]), ([""], ["", ""]), (["", ""], ["ab", "é" if utf8 else "e"]), (["ab"], [""])):
            both = reference_counts(queries, candidates, utf8)
            for scorer in SCORERS:
                scores, larger = reference_scores(scorer, both), LARGER_IS_BETTER[scorer]
                for cutoff in (0.0, 1.0, 100.0):
                    got = run_within(sw, scope, engine, as_items(queries, utf8), as_items(candidates, utf8), scorer=scorer, cutoff=cutoff)
                    assert_csr(got, expected_within(scores, larger, cutoff), f"{scorer} {queries} {candidates} utf8={utf8} cutoff={cutoff}")
                if scorer in ("ratio", "jaro") and queries[0] == "" and candidates[0] == "":
                    top = 100.0 if scorer == "ratio" else 1.0
                    got = run_within(sw, scope, engine, as_items(queries, utf8), as_items(candidates, utf8), scorer=scorer, cutoff=top)
                    assert got[1][0] == 0 and got[2].view(np.float64)[0] == top
    # a similarity cutoff of 0.0 returns every pair in order; an OSA cutoff of 0 exact duplicates only
    wq, wc = (as_items(side, False) for side in word_batch(False))
    for scorer in SCORERS[2:]:
        got = run_within(sw, scope, lev, wq, wc, "prepared", scorer=scorer, cutoff=0.0)
        assert got[0].tolist() == list(range(0, 70 * 300 + 1, 300)) and np.array_equal(got[1], np.tile(np.arange(300, dtype=np.uint32), 70))
        assert np.array_equal(got[2], word_batch_scores(False, scorer).view(np.uint64).ravel()), scorer
    got = run_within(sw, scope, lev, wq, wc, "prepared", scorer="osa", cutoff=0.0)
    same = np.array([[q == c for c in wc] for q in wq])
    assert same.sum() > 0 and np.array_equal(got[1], np.nonzero(same)[1]) and (got[2] == 0).all() and np.array_equal(np.diff(got[0].astype(np.int64)), same.sum(axis=1))

    def refused(engine, queries, candidates, scorer, cutoff, p, status, utf8=False, words=(), null=(), capacity=64):
        offsets = np.full(len(queries) + 1, SENTINEL64, dtype=np.uint64)
        indices, values = np.full(64, SENTINEL32, dtype=np.uint32), np.full(64, SENTINEL64, dtype=np.uint64)
        outs = [None if name in null else array for name, array in (("offsets", offsets), ("indices", indices), ("scores", values))]
        got, message = raw_within(sw, engine, scope, queries, candidates, scorer, cutoff, p, outs[0], outs[1], outs[2], capacity, utf8)
        assert got == status and message and all(word in message for word in words), (got, message, status)
        assert (offsets == SENTINEL64).all() and (indices == SENTINEL32).all() and (values == SENTINEL64).all(), (status, message)

    inf = float("inf")
    refused(lev, qs, cs, 6, 0.5, 0.1, "invalid_argument")
    refused(lev, qs, cs, -1, 0.5, 0.1, "invalid_argument")
    for scorer in range(6):
        refused(lev, qs, cs, scorer, float("nan"), 0.1, "invalid_argument")
        refused(lev, qs, cs, scorer, -1.0, 0.1, "invalid_argument")
        refused(lev, qs, cs, scorer, -inf, 0.1, "invalid_argument")
        refused(lev, qs, cs, scorer, 1.0, 0.1, "invalid_argument", null=("offsets",))
        refused(lev, qs, cs, scorer, 1.0, 0.1, "invalid_argument", null=("indices",))
        refused(lev, qs, cs, scorer, 1.0, 0.1, "invalid_argument", null=("scores",))
        refused(lev, qs, cs, scorer, 1.0, 0.1, "invalid_argument", null=("indices", "scores"))   # (a capacity without arrays)
    for scorer in (0, 1):
        refused(lev, qs, cs, scorer, inf, 0.1, "invalid_argument", words=("dense cross-product",))
    refused(lev, qs, cs, 5, 0.5, 0.3, "invalid_argument")
    refused(lev, qs, cs, 5, 0.5, -0.1, "invalid_argument")
    refused(lev, qs, cs, 5, 0.5, float("nan"), "invalid_argument")
    costly = sw.LevenshteinDistances(0, 2, 1, 1, capabilities=scope)
    for scorer in range(6):
        refused(costly, qs, cs, scorer, 1.0, 0.1, "not_implemented")
        refused(lev8, qs, [b"ok", b"\xff\xfe"], scorer, 1.0, 0.1, "invalid_utf8", utf8=True)
    # the families' length limits, before any output is written: the message names a pair and both lengths
    long_q, long_c = [b"ab", b"a" * 2049], [b"abc", b"b" * 5, b"c" * 2049]
    for scorer in range(4):   # OSA, Indel, LCS, ratio: the SHORTER string of a pair is over the limit only when both are long
        refused(lev, long_q, long_c, scorer, 1.0, 0.1, "unsupported_length", words=("(1, 2)", "2049 x 2049"))
    for scorer in (4, 5):     # Jaro: either string
        refused(lev, long_q, cs, scorer, 0.5, 0.1, "unsupported_length", words=("(1, 0)", "2049 x 6"))
        refused(lev, qs, long_c, scorer, 0.5, 0.1, "unsupported_length", words=("(0, 2)", "6 x 2049"))
    with pytest.raises(sw.StringWarsError) as info:
        lev.extract_within(long_q, long_c, scope, scorer="ratio", cutoff=50.0)
    assert info.value.status == "unsupported_length"
    # one long side is within the limit of the first four scorers
    one_long = reference_counts(["ab", "a" * 2049], ["abc", "b" * 5, "aab"])
    for scorer, cutoff in (("osa", 3.0), ("indel", 3.0), ("lcs", 1.0), ("ratio", 0.05)):
        want = expected_within(reference_scores(scorer, one_long), LARGER_IS_BETTER[scorer], cutoff)
        assert int(want[0][-1]) > 0
        assert_csr(run_within(sw, scope, lev, long_q, [b"abc", b"b" * 5, b"aab"], scorer=scorer, cutoff=cutoff), want, f"{scorer} one long side")
    # the Python layer's own argument checks
    with pytest.raises(ValueError):
        lev.extract_within(qs, cs, scope, scorer="levenshtein", cutoff=1.0)
    with pytest.raises(ValueError):
        lev.extract_within(qs, cs, scope, scorer="jaro", cutoff=None)
    with pytest.raises(TypeError):
        lev.extract_within(qs, cs, scope, scorer="jaro")
    with pytest.raises(sw.StringWarsError) as info:
        lev.extract_within(qs, cs, scope, scorer="jaro_winkler", cutoff=0.5, prefix_weight=0.3)
    assert info.value.status == "invalid_argument"
    with pytest.raises(sw.StringWarsError) as info:
        lev.extract_within(qs, cs, scope, scorer="osa", cutoff=inf)
    assert info.value.status == "invalid_argument"
    assert_csr(run_within(sw, scope, lev, qs, cs, scorer="ratio", cutoff=80.0, prefix_weight=0.3),   # (ignored by the other scorers)
               expected_within(reference_scores("ratio", counts), True, 80.0), "ratio ignores p")


@pytest.mark.gpu
def test_determinism(sw, scope, lev):
    """The same call twice: identical bytes in all three outputs, host arrays and device tensors."""
    qs, cs = (as_items(side, False) for side in word_batch(False))
    for scorer in ("ratio", "jaro_winkler", "osa"):
        cutoff = word_batch_cutoffs(False, scorer)[0]
        total = int(expected_within(word_batch_scores(False, scorer), LARGER_IS_BETTER[scorer], cutoff)[0][-1])
        for device_out in (False, True):
            first, second = (run_within(sw, scope, lev, qs, cs, "prepared", device_out, room=total, scorer=scorer, cutoff=cutoff) for _ in range(2))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), (scorer, device_out)


@pytest.mark.gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_cpp_wrappers_against_the_reference(tmp_path, utf8):
    """Both overloads of LevenshteinDistances::extract_within (stringwars_amd.hpp) from a C++ program: raw tape views and prepared
    tapes, every scorer at the tight cutoff, two prefix weights, candidates and the self-search (a null pointer); a counting call,
    then a filled call with exactly that room. What the program writes equals the reference bit for bit."""
    binary = build_check_extract_within(tmp_path)
    qs, cs = word_batch(utf8)
    own_counts = reference_counts(list(qs), list(qs), utf8)
    requests, wants = [], []
    for scorer_id, scorer in enumerate(SCORERS):
        larger = LARGER_IS_BETTER[scorer]
        scores, own = word_batch_scores(utf8, scorer), reference_scores(scorer, own_counts)
        cutoff = word_batch_cutoffs(utf8, scorer)[1]
        for prepared in (0, 1):
            requests += [(scorer_id, prepared, 0, cutoff, 0.1), (scorer_id, prepared, 1, cutoff, 0.1)]
            wants += [expected_within(scores, larger, cutoff), expected_within(own, larger, cutoff)]
    for prepared in (0, 1):
        requests.append((5, prepared, 0, 0.9, 0.25))
        wants.append(expected_within(word_batch_scores(utf8, "jaro_winkler", 0.25), True, 0.9))
    write_within_case(tmp_path / "batch.case", utf8, qs, cs, requests)
    done = subprocess.run([str(binary), str(tmp_path / "batch.case"), str(tmp_path / "batch.out")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    raw = open(tmp_path / "batch.out", "rb").read()
    at = 0
    for request, want in zip(requests, wants):
        total = int(want[0][-1])
        counted = np.frombuffer(raw, dtype=np.uint64, count=len(qs) + 1, offset=at)
        at += counted.nbytes
        offsets = np.frombuffer(raw, dtype=np.uint64, count=len(qs) + 1, offset=at)
        at += offsets.nbytes
        assert np.array_equal(counted, want[0]), f"C++ extract_within utf8={utf8} request {request}: the counting call"
        indices = np.frombuffer(raw, dtype=np.uint32, count=total, offset=at)
        at += indices.nbytes
        bits = np.frombuffer(raw, dtype=np.uint64, count=total, offset=at)
        at += bits.nbytes
        assert_csr((offsets, indices, bits), want, f"C++ extract_within utf8={utf8} request {request}")
    assert at == len(raw)
