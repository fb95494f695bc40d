"""Where the outputs live: every output of top-k, the score search and the alignments on the host or on the device, independently.

The synchronous two-tape calls (two_tape.hip) write an output in place when it is device memory, and stage it in scratch and copy it
back when it is host memory; each output decides for itself. The range search has this test in test_within.py, infix search and the
scored families one mixed case each in their own; here are the three calls whose own tests run all outputs on one side. What is
expected never comes from the library: the oracle's distance matrix (top-k), test_extract's host scorers (score search) and
test_align's canonical scripts (alignments, with the oracle's distance for the pairs too long for them)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child
from test_align import random_strs, reference_script, script_errors
from test_extract import LARGER_IS_BETTER, PAD_BITS, PAD_INDEX, as_items, expected_rows, word_batch, word_batch_scores
from test_topk import PAD, expected_topk, oracle_matrix

SENTINEL = 0x5A5A5A5A
ROWS, COLUMNS, K = 33, 200, 3   # three blocks of 16 queries less some, four chunks of 64 candidates less some


def placed(on_device, n, host_dtype, device_dtype, fill=SENTINEL):
    import torch
    return torch.full((n,), fill, dtype=device_dtype, device="cuda") if on_device else np.full(n, fill, host_dtype)


def on_host(array, dtype):
    return (array.cpu().numpy() if hasattr(array, "cpu") else array).view(dtype)


def dominant_kernel(scope, call):
    scope.set_profiling(True)
    try:
        call()
        return scope.last_timing()["dominant_name"]
    finally:
        scope.set_profiling(False)


# ---- top-k ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(sw, orc):
    """33 queries x 200 candidates of at most 16 bytes; the queries are candidates too, so a bound of 1 finds every row something."""
    candidates, _ = sw.generate_pairs("short_words", COLUMNS, seed=71)
    queries = candidates[100:100 + ROWS]
    return queries, candidates, oracle_matrix(sw, orc, queries, candidates)


@pytest.mark.gpu
def test_topk_outputs_on_host_and_device(sw, scope, words):
    import torch
    queries, candidates, d = words
    want = expected_topk(d, K, bound=1)
    padded = (want[0] == PAD).sum(axis=1)
    assert (padded < K).all() and (padded > 0).any() and (padded == 0).any()   # short rows and full ones, none empty
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    fused = sw.LevenshteinDistances(capabilities=scope)
    general = sw.LevenshteinDistances(capabilities=scope, algorithm="wavefront")   # never the fused kernel
    assert "cross_topk" in dominant_kernel(scope, lambda: fused.topk(pq, pc, scope, k=K, bound=1))
    assert dominant_kernel(scope, lambda: general.topk(pq, pc, scope, k=K, bound=1)).startswith("topk_select/")
    for (path, engine), (dev_i, dev_d) in itertools.product((("fused", fused), ("general", general)), itertools.product((False, True), repeat=2)):
        what = f"{path}: indices on {'device' if dev_i else 'host'}, distances on {'device' if dev_d else 'host'}"
        out = placed(dev_i, ROWS * K, np.uint32, torch.int32), placed(dev_d, ROWS * K, np.uint32, torch.int32)
        got = engine.topk(pq, pc, scope, k=K, bound=1, out=out)
        assert got[0] is out[0] and got[1] is out[1], what
        indices, distances = on_host(out[0], np.uint32).reshape(ROWS, K), on_host(out[1], np.uint32).reshape(ROWS, K)
        assert (indices == want[0]).all() and (distances == want[1]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("dev_i, dev_d", [(False, True), (True, False)])
def test_topk_without_candidates_pads_every_row(sw, scope, words, dev_i, dev_d):
    import torch
    queries = words[0]
    engine = sw.LevenshteinDistances(capabilities=scope)
    out = placed(dev_i, ROWS * K, np.uint32, torch.int32), placed(dev_d, ROWS * K, np.uint32, torch.int32)
    engine.topk(queries, sw.Strs([]), scope, k=K, out=out)
    assert (on_host(out[0], np.uint32) == PAD).all() and (on_host(out[1], np.uint32) == PAD).all()


# ---- the score search -----------------------------------------------------------------------------------------------------------------
# a cutoff per scorer that admits some candidates of a row and, in some rows, fewer than k (checked on the reference below)
CUTOFFS = {"osa": 3.0, "ratio": 80.0, "jaro_winkler": 0.9}


@pytest.mark.gpu
@pytest.mark.parametrize("scorer", sorted(CUTOFFS))   # one, two and three counts per pair go through the family's launcher
def test_extract_outputs_on_host_and_device(sw, scope, scorer):
    import torch
    queries, candidates = (as_items(side, False) for side in word_batch(False))
    queries, candidates = queries[:ROWS], candidates[:COLUMNS]
    scores = word_batch_scores(False, scorer)[:ROWS, :COLUMNS]
    want = expected_rows(scores, LARGER_IS_BETTER[scorer], K, CUTOFFS[scorer])
    padded = (want[0] == PAD_INDEX).sum(axis=1)
    assert (padded > 0).any() and (padded == 0).any()
    engine = sw.LevenshteinDistances(capabilities=scope)
    pq, pc = sw.PreparedTape(scope, sw.Strs(queries)), sw.PreparedTape(scope, sw.Strs(candidates))
    for dev_i, dev_s in itertools.product((False, True), repeat=2):
        what = f"{scorer}: indices on {'device' if dev_i else 'host'}, scores on {'device' if dev_s else 'host'}"
        out = placed(dev_i, ROWS * K, np.uint32, torch.int32), placed(dev_s, ROWS * K, np.float64, torch.float64, fill=7.0)
        engine.extract(pq, pc, scope, scorer=scorer, k=K, cutoff=CUTOFFS[scorer], out=out)
        indices, bits = on_host(out[0], np.uint32).reshape(ROWS, K), on_host(out[1], np.uint64).reshape(ROWS, K)
        assert (indices == want[0]).all(), what
        assert (bits == want[1]).all(), what   # bit for bit, the padding's pattern of ones included


@pytest.mark.gpu
@pytest.mark.parametrize("dev_i, dev_s", [(False, True), (True, False)])
def test_extract_without_candidates_pads_every_row(sw, scope, dev_i, dev_s):
    import torch
    queries = as_items(word_batch(False)[0], False)[:ROWS]
    engine = sw.LevenshteinDistances(capabilities=scope)
    out = placed(dev_i, ROWS * K, np.uint32, torch.int32), placed(dev_s, ROWS * K, np.float64, torch.float64, fill=7.0)
    engine.extract(sw.Strs(queries), sw.Strs([]), scope, scorer="ratio", k=K, out=out)
    assert (on_host(out[0], np.uint32) == PAD_INDEX).all() and (on_host(out[1], np.uint64) == PAD_BITS).all()


# ---- alignments -----------------------------------------------------------------------------------------------------------------------
def align_pairs():
    """64 pairs of up to 40 symbols over four letters, an empty string, an empty pair and an equal pair among them."""
    rng = np.random.default_rng(83)
    a, b = random_strs(rng, 64, 1, 40, 4), random_strs(rng, 64, 1, 40, 4)
    a[5], b[9], a[20], b[20], b[31] = b"", b"", b"", b"", a[31]
    return a, b


def expected_alignments(a, b):
    scripts = [reference_script(x, y) for x, y in zip(a, b)]
    offsets = np.zeros(len(a) + 1, dtype=np.uint64)
    np.cumsum([len(ops) for _, ops in scripts], out=offsets[1:])
    return np.array([d for d, _ in scripts], dtype=np.uint32), offsets, b"".join(ops for _, ops in scripts)


def raw_align(sw, engine, scope, a, b, placement):
    """swh_levenshtein_align_u64tape itself, each of (distances, offsets, ops) on the device where `placement` says so. Returns the
    three arrays on the host, the ops at their full capacity."""
    import torch
    from stringwars_amd import _native as N
    ta, _, keep_a = sw.engines._c_tape(sw.Strs(a), want64=True)
    tb, _, keep_b = sw.engines._c_tape(sw.Strs(b), want64=True)
    capacity = sum(len(x) for x in a) + sum(len(x) for x in b)
    outs = (placed(placement[0], len(a), np.uint32, torch.int32), placed(placement[1], len(a) + 1, np.uint64, torch.int64, fill=7),
            placed(placement[2], capacity, np.uint8, torch.uint8, fill=0x5A))
    pointers = [C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) for x in outs]
    err = C.c_char_p()
    status = N.lib.swh_levenshtein_align_u64tape(engine._handle, scope.handle, C.byref(ta), C.byref(tb), N.UNBOUNDED, *pointers, capacity, C.byref(err))
    assert status == 0, err.value
    return on_host(outs[0], np.uint32), on_host(outs[1], np.uint64), on_host(outs[2], np.uint8)


@pytest.mark.gpu
def test_align_outputs_on_host_and_device(sw, scope):
    a, b = align_pairs()
    want_d, want_o, want_ops = expected_alignments(a, b)
    assert 0 in want_d and len(want_ops) < sum(len(x) for x in a) + sum(len(x) for x in b)
    engine = sw.LevenshteinDistances(capabilities=scope)
    for placement in itertools.product((False, True), repeat=3):
        distances, offsets, ops = raw_align(sw, engine, scope, a, b, placement)
        assert (distances == want_d).all() and (offsets == want_o).all(), placement
        assert ops[:len(want_ops)].tobytes() == want_ops, placement
        if not placement[2]:   # a host array receives the ops there are, not the capacity
            assert (ops[len(want_ops):] == 0x5A).all(), placement


@pytest.mark.gpu
def test_align_mixed_placement_regrows_the_scratch(request, sw, orc):
    """Distances and ops on the host, offsets on the device, on a fresh scope whose alignment scratch is first sized for the fixed part
    (a few KB, so 1 MiB and a quarter) and then has to hold the op slots and the staged ops of 2 x 300 000 symbols besides: it is
    regrown after the measurements, and the fixed part, with the staged distances in it, is carved a second time.
    STRINGWARS_AMD_ALIGN_CHUNK_KB=4 (test library) makes the batch many chunks. The two long pairs are checked as scripts of the
    oracle's cost (a reference script of 300 000 x 24 cells is not worth its time), the others exactly."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_ALIGN_CHUNK_KB="4"), test_library=True):
        return
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    a, b = align_pairs()
    rng = np.random.default_rng(84)
    long_one, short_one = bytes(rng.integers(0, 4, 300_000).astype(np.uint8)), bytes(rng.integers(0, 4, 24).astype(np.uint8))
    a, b = a + [long_one, short_one], b + [short_one, long_one]
    want_d, want_o, want_ops = expected_alignments(a[:64], b[:64])
    long_d = orc.levenshtein_pairs(sw.Strs(a[64:]), sw.Strs(b[64:]), algo="hyyro")
    distances, offsets, ops = raw_align(sw, engine, scope, a, b, (False, True, False))
    assert (distances[:64] == want_d).all() and (offsets[:65] == want_o).all() and ops[:len(want_ops)].tobytes() == want_ops
    assert (distances[64:] == np.asarray(long_d, dtype=np.uint32)).all()
    for i in (64, 65):
        assert script_errors(a[i], b[i], ops[int(offsets[i]):int(offsets[i + 1])].tobytes(), int(distances[i])) is None, i
    assert (ops[int(offsets[66]):] == 0x5A).all()
