"""Levenshtein range search (`engine.within`, swh_levenshtein_within_*): every candidate within a bound of every query, as CSR.
The expected rows come from the CPU oracle's dense matrix: per row np.flatnonzero(d[i] <= bound) and the distances there. What each
input is for is asserted by the CPU tests on the oracle alone; the GPU tests compare offsets, indices and distances exactly."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child
from test_topk import (AB_STRINGS, CENTRE, _planted, _pool_and_words, centre_pool, check_rows, expected_topk, gather, oracle_matrix, pooled_queries,
                       prefix_family, staircase)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("swh_levenshtein_within_u64tape", "swh_levenshtein_utf8_within_u64tape", "swh_levenshtein_within_prepared")
BOUNDS = (0, 1, 3, 32)          # at 32 every word-sized pair hits: every lane of every chunk stores
QUERY_COUNTS = (1, 15, 16, 17, 33)                 # the 16-query block edge
CANDIDATE_COUNTS = (0, 1, 63, 64, 65, 129, 640)    # chunk edges, empty, several chunks
HIGH = bytes(range(0x80, 0x80 + 20))               # bytes >= 0x80: the high-nibble tables
FAR = b"\xfe" * 9                                  # nothing of the staircase input lies within 3 edits of it
FOREIGN_QUERY = b"~" * 20                          # a symbol no prefix holds: 20 or more edits from every candidate


def expected_csr(d: np.ndarray, bound: int):
    """(offsets, indices, distances) of a dense (nq, nc) distance matrix: per row the columns with d <= bound, ascending."""
    hit = d <= bound
    offsets = np.zeros(d.shape[0] + 1, dtype=np.uint64)
    np.cumsum(hit.sum(axis=1), out=offsets[1:])
    rows, columns = np.nonzero(hit)   # row-major: ascending columns within a row
    return offsets, columns.astype(np.uint32), d[rows, columns].astype(np.uint32)


def expected_csr_pooled(d_pool: np.ndarray, index: np.ndarray, bound: int):
    """The CSR of a search whose query i is string index[i] of a small pool: the pool's rows, repeated by the index."""
    pool_offsets, pool_indices, pool_distances = expected_csr(d_pool, bound)
    pool_offsets = pool_offsets.astype(np.int64)
    counts = np.diff(pool_offsets)[index]
    offsets = np.zeros(len(index) + 1, dtype=np.uint64)
    np.cumsum(counts, out=offsets[1:])
    source = np.repeat(pool_offsets[index], counts) + np.arange(int(offsets[-1]), dtype=np.int64) - np.repeat(offsets[:-1].astype(np.int64), counts)
    return offsets, pool_indices[source], pool_distances[source]


def check_csr(got, want, what=""):
    offsets, indices, distances = (_host(x) for x in ((got.offsets, got.indices, got.distances) if hasattr(got, "offsets") else got))
    assert (offsets.view(np.uint64) == want[0]).all(), f"offsets differ {what}: first bad row {np.argwhere(offsets.view(np.uint64) != want[0])[0]}"
    total = int(want[0][-1])
    assert len(indices) >= total and len(distances) >= total, what
    assert (indices[:total].view(np.uint32) == want[1]).all(), f"indices differ {what}: first at {np.argwhere(indices[:total].view(np.uint32) != want[1])[0]}"
    assert (distances[:total].view(np.uint32) == want[2]).all(), f"distances differ {what}: first at {np.argwhere(distances[:total].view(np.uint32) != want[2])[0]}"


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ---- the inputs of the fused route: 33 queries x 640 candidates each, sliced for the sweep; `bound`: where what the input is for shows ----
STAIR_LEVELS = [6, 2, 30, 1, 12, 0, 3, 30, 2, 5]   # chunk c of the candidates lies this far from the centre: near chunks in the first and last slice


def _fused_input(name):
    """(queries, candidates, the bound at which the CPU test checks what the input is for)."""
    if name == "staircase":      # queries one edit from the centre, an empty, a high-byte and a far one; chunks of candidates at known distances
        items = staircase(640, STAIR_LEVELS)
        items[3], items[70], items[200], items[639] = HIGH, b"", HIGH, b""
        return centre_pool(30) + [b"", HIGH, FAR], items, 3
    if name == "heavy_ties":     # every distance is 0 .. 5 and most rows hold hundreds of hits; nobody equals the last two queries
        rng = np.random.default_rng(3)
        return AB_STRINGS + [b"ababa", b"bbbbb"], [AB_STRINGS[i] for i in rng.integers(0, len(AB_STRINGS), 640)], 0
    if name == "prefixes":       # d == |m - n| exactly: the length-gap prune is tight
        pool, _, items, _ = prefix_family(640)
        return pool[1:33] + [FOREIGN_QUERY], items, 3
    raise KeyError(name)


FUSED_INPUTS = ("staircase", "heavy_ties", "prefixes")


@functools.lru_cache(maxsize=None)
def _fused_case(name):
    import oracle
    import stringwars_amd as sw
    queries, candidates, bound = _fused_input(name)
    assert len(queries) == 33 and len(candidates) == 640 and max(map(len, queries + candidates)) <= 32
    q, c = sw.Strs(queries), sw.Strs(candidates)
    d = oracle_matrix(sw, oracle, q, c)
    d.setflags(write=False)
    return q, c, d, bound


def _pooled_staircase(sw, orc, nq, nc):
    """`nq` queries drawn from the staircase input's 33, against its candidates continued to `nc`."""
    pool = _fused_input("staircase")[0]
    items = staircase(nc, STAIR_LEVELS)
    queries, index = pooled_queries(sw, pool, nq)
    candidates = sw.Strs(items)
    return queries, candidates, oracle_matrix(sw, orc, sw.Strs(pool), candidates), index


def _pooled_prefixes(sw, orc, nq, nc=3000):
    pool, _, items, _ = prefix_family(nc)
    queries, index = pooled_queries(sw, pool, nq)
    candidates = sw.Strs(items)
    return queries, candidates, oracle_matrix(sw, orc, sw.Strs(pool), candidates), index


def _general_blocks_input(sw, shape):
    """The inputs of test_topk_general_path_blocks: non-ASCII words, a pool planted in the first and the last candidate slice."""
    nq, nc, first, last = {"two_blocks_three_slices": ((1 << 18) + 37, 600, 256, 512), "one_block_two_slices": (9000, 9000, 7456, 7456)}[shape]
    pool, words = _pool_and_words(nc)
    items = _planted(words, pool, first, last)
    queries, index = pooled_queries(sw, pool, nq)
    return pool, items, queries, index, first, last


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_within_symbols_exported_and_announced(sw):
    from stringwars_amd import _native
    lib = C.CDLL(sw.LIBRARY_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _native.SIGNATURES, name
    assert "within" in sw.capabilities().split(",")


def test_range_matches_on_a_hand_written_csr(sw):
    # rows: {0: (0, d 0), (2, d 1)}, {1: nothing}, {2: (0, d 1), (2, d 0), (3, d 2)}, {3: (3, d 0)}
    r = sw.RangeMatches(np.array([0, 2, 2, 5, 6], np.uint64), np.array([0, 2, 0, 2, 3, 3], np.uint32), np.array([0, 1, 1, 0, 2, 0], np.uint32))
    assert len(r) == 4 and r.counts.tolist() == [2, 0, 3, 1]
    assert [x.tolist() for x in r.row(0)] == [[0, 2], [0, 1]] and [x.tolist() for x in r.row(1)] == [[], []]
    assert [x.tolist() for x in r.row(-1)] == [[3], [0]]
    with pytest.raises(IndexError):
        r.row(4)
    assert [x.tolist() for x in r.pairs()] == [[0, 0, 2, 2, 2, 3], [0, 2, 0, 2, 3, 3], [0, 1, 1, 0, 2, 0]]
    assert [x.tolist() for x in r.pairs(upper=True)] == [[0, 2], [2, 3], [1, 2]]
    empty = sw.RangeMatches(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert len(empty) == 0 and all(len(x) == 0 for x in empty.pairs())


def test_expected_csr_helpers():
    d = np.array([[0, 3, 1, 1], [5, 5, 5, 5], [2, 0, 2, 9]])
    offsets, indices, distances = expected_csr(d, 1)
    assert offsets.tolist() == [0, 3, 3, 4] and indices.tolist() == [0, 2, 3, 1] and distances.tolist() == [0, 1, 1, 0]
    index = np.array([2, 0, 1, 2, 0])
    pooled = expected_csr_pooled(d, index, 2)
    plain = expected_csr(d[index], 2)
    assert all((a == b).all() for a, b in zip(pooled, plain)) and int(plain[0][-1]) == 3 + 3 + 0 + 3 + 3


def _chunks_hit(d, bound):
    """Per row, the number of different 64-candidate chunks with a hit."""
    hit = d <= bound
    pad = (-hit.shape[1]) % 64
    return np.pad(hit, ((0, 0), (0, pad))).reshape(hit.shape[0], -1, 64).any(axis=2).sum(axis=1)


def _is_what_it_is_for(d, bound, what, last_slice_from=None):
    hit = d <= bound
    assert 0 < hit.sum() < d.size, what
    assert (hit.sum(axis=1) == 0).any(), f"{what}: no empty row"
    assert (_chunks_hit(d, bound) >= 2).any(), f"{what}: no row with hits in two chunks"
    if last_slice_from is not None:   # three slices of 4, 4 and 2 chunks (640 candidates), or the slices the shape is cut into
        first_slice_upto, last_from = last_slice_from
        assert hit[:, :first_slice_upto].any() and hit[:, last_from:].any(), f"{what}: the first or the last slice holds no hit"


def test_fused_inputs_are_what_they_are_for(sw, orc):
    for name in FUSED_INPUTS:
        q, c, d, bound = _fused_case(name)
        _is_what_it_is_for(d, bound, name, last_slice_from=(256, 512))
        assert (d <= 32).all(), name   # the dense extreme: at bound 32 every pair is a hit
        for nq in QUERY_COUNTS:        # every shape of the sweep that can hold a hit holds one at some bound below the dense one
            for nc in CANDIDATE_COUNTS[1:]:
                assert (d[:nq, :nc] <= 32).all()
        assert any(len(q[i]) == 0 for i in range(len(q))) or name == "prefixes"
        assert any(len(c[j]) == 0 for j in range(len(c))), name   # empty candidates in every input
    q, c, d, _ = _fused_case("staircase")
    assert any(max(q[i], default=0) >= 0x80 for i in range(len(q))) and any(max(c[j], default=0) >= 0x80 for j in range(len(c)))
    # the prefix family sits on the length gap: pairs at d == |m - n| == bound and at bound + 1, for every bound of the sweep below the dense one
    q, c, d, _ = _fused_case("prefixes")
    gap = np.abs(q.lengths.astype(np.int64)[:, None] - c.lengths.astype(np.int64)[None, :])
    assert (d >= gap).all()
    for bound in (0, 1, 3):
        assert ((d == gap) & (gap == bound)).any() and ((d == gap) & (gap == bound + 1)).any(), bound
    assert len(q[31]) == 32 and (c.lengths == 32).any() and (c.lengths == 0).any()   # the 32-row mask and the empty string


def test_pooled_inputs_are_what_they_are_for(sw, orc):
    queries, candidates, d_pool, index = _pooled_staircase(sw, orc, 4096, 700)
    _is_what_it_is_for(d_pool, 1, "pooled staircase bound 1")
    assert 0 < (d_pool <= 0).sum() and ((d_pool <= 0).sum(axis=1) == 0).any()   # bound 0: the centre's row alone, one chunk of it
    assert len(np.unique(index)) == 33 and len(candidates) == 700
    queries, candidates, d_pool, index = _pooled_prefixes(sw, orc, 2048)
    assert 0 < (d_pool <= 3).sum() < d_pool.size and (_chunks_hit(d_pool, 3) >= 2).any()   # (its empty rows are the 33 x 640 input's)


def test_general_inputs_are_what_they_are_for(sw, orc):
    for shape in ("two_blocks_three_slices", "one_block_two_slices"):
        pool, items, queries, index, first, last = _general_blocks_input(sw, shape)
        d_pool = oracle_matrix(sw, orc, sw.Strs(pool), sw.Strs(items), utf8=True)
        hit = d_pool <= 1
        assert 0 < hit.sum() < d_pool.size and (_chunks_hit(d_pool, 1) >= 2).any(), shape
        assert hit[:, :first].any() and hit[:, last:].any(), shape   # hits in the first and in the last candidate slice
        assert (d_pool <= 0).sum(axis=1).min() >= 1   # (every pool word is planted: no empty row here; the other general inputs have them)
    q, c, d = _tokens_case(sw, orc)
    for bound in (0, 8):
        assert ((d <= bound).sum(axis=1) == 0).any(), bound
    assert 0 < (d <= 8).sum() and (d <= 200).all()
    q, c, d = _costs_case(sw, orc)
    assert 0 < (d <= COSTS_BOUND).sum() < d.size and ((d <= COSTS_BOUND).sum(axis=1) == 0).any()


COSTS = (0, 2, 3, 1)
COSTS_BOUND = 40


def _tokens_case(sw, orc):
    a, b = sw.generate_pairs("tokens64", 64, seed=13)
    items = [b[i] for i in range(64)]
    items[5], items[40] = a[9], a[9][:-1]   # one exact and one near candidate: bound 0 and bound 8 both find something
    c = sw.Strs(items)
    return a, c, oracle_matrix(sw, orc, a, c)


def _costs_case(sw, orc):
    rng = np.random.default_rng(21)
    letters = np.frombuffer(b"ACGT", np.uint8)
    def strings(count):
        return [bytes(rng.choice(letters, int(n))) for n in rng.integers(80, 121, count)]
    queries, items = strings(8), strings(40)
    for j in (3, 17, 38):   # near copies of three queries: a few in-bound pairs among ~100-symbol strings that are otherwise far apart
        s = bytearray(queries[j % 8])
        for at in rng.choice(len(s), 6, replace=False):
            s[at] = int(rng.choice(letters))
        items[j] = bytes(s)
    q, c = sw.Strs(queries), sw.Strs(items)
    return q, c, oracle_matrix(sw, orc, q, c, costs=COSTS)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _fused_slices(timing, nq, nc, symbols, total, offset_bytes=8):
    """The candidate slices per query block of a fused call, from the byte count the header documents: the two tapes, 12 bytes per
    (query, slice) count, the row offsets and 8 bytes per stored hit."""
    rest = timing["bytes"] - symbols - (nq + nc) * offset_bytes - (nq + 1) * 8 - total * 8
    assert rest % (12 * nq) == 0, timing
    return rest // (12 * nq)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED_INPUTS)
def test_within_fused_sweep(sw, scope, name):
    """Query counts around the 16-query block, candidate counts around the 64-candidate chunk, bounds from exact match to the dense
    extreme: offsets, indices and distances exactly, on raw tapes and on prepared sub-views."""
    q, c, d, _ = _fused_case(name)
    engine = sw.LevenshteinDistances(capabilities=scope)
    pq, pc = sw.PreparedTape(scope, q), sw.PreparedTape(scope, c)
    scope.set_profiling(True)
    try:
        for nq in QUERY_COUNTS:
            for nc in CANDIDATE_COUNTS:
                for bound in BOUNDS:
                    want = expected_csr(d[:nq, :nc], bound)
                    what = f"{name} {nq} x {nc} bound {bound}"
                    if nc == 0:
                        check_csr(engine.within(q[:nq], sw.Strs([]), scope, bound=bound), want, what)
                        continue
                    check_csr(engine.within(pq[:nq], pc[:nc], scope, bound=bound), want, "prepared " + what)
                    assert scope.last_timing()["dominant_name"] == "cross_within", (what, scope.last_timing())
                    if bound == 32:
                        assert int(want[0][-1]) == nq * nc
                    if nc in (1, 65, 640):
                        check_csr(engine.within(q[:nq], c[:nc], scope, bound=bound), want, "raw " + what)
    finally:
        scope.set_profiling(False)
    got = engine.within(sw.Strs([]), c, scope, bound=3)
    assert len(got) == 0 and got.offsets.tolist() == [0] and len(got.indices) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("slices", [1, 3])
def test_within_slice_regimes(request, sw, scope, slices):
    """33 x 640 with one slice and with three (STRINGWARS_AMD_WITHIN_SLICES, a child on the test library) and, in this process, with the
    ten the slicing rule gives (one per chunk). The regime reached is read from the call: the 12 bytes per (query, slice) in its byte count."""
    in_child = run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_WITHIN_SLICES=str(slices)), test_library=True)
    if in_child:
        assert os.environ["STRINGWARS_AMD_WITHIN_SLICES"] == str(slices) and sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    else:
        assert "STRINGWARS_AMD_WITHIN_SLICES" not in os.environ
    engine = sw.LevenshteinDistances(capabilities=scope)
    scope.set_profiling(True)
    try:
        for name in FUSED_INPUTS:
            q, c, d, _ = _fused_case(name)
            pq, pc = sw.PreparedTape(scope, q), sw.PreparedTape(scope, c)
            for bound in BOUNDS:
                want = expected_csr(d, bound)
                check_csr(engine.within(pq, pc, scope, bound=bound, capacity=33 * 640), want, f"{name} bound {bound} slices {slices}")
                timing = scope.last_timing()
                assert timing["dominant_name"] == "cross_within", timing
                reached = _fused_slices(timing, 33, 640, int(q.lengths.sum()) + int(c.lengths.sum()), int(want[0][-1]))
                assert reached == (slices if in_child else 10), (reached, timing)
    finally:
        scope.set_profiling(False)


WORD_EDGE_LENGTHS = (0, 1, 31, 32)   # empty, one column, one short of the longest word, the longest
WORD_EDGE_CANDIDATES = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def _word_edge_case(misfit):
    """33 queries x 129 candidates over a four-letter alphabet, every length one of WORD_EDGE_LENGTHS (`misfit`: candidate 70 has 33
    bytes), and the oracle's matrix."""
    import oracle
    import stringwars_amd as sw
    rng = np.random.default_rng(71)
    words = [bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), int(n))) for n in rng.choice(WORD_EDGE_LENGTHS, 33 + 129)]
    if misfit:
        words[33 + 70] = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 33))
    q, c = sw.Strs(words[:33]), sw.Strs(words[33:])
    assert set(q.lengths.tolist()) == set(WORD_EDGE_LENGTHS) and int(c.lengths.max()) == (33 if misfit else 32)
    d = oracle_matrix(sw, oracle, q, c)
    d.setflags(write=False)
    return q, c, d


@pytest.mark.gpu
def test_word_kernels_share_their_item_edges(request, sw, scope):
    """The three word-sized cross-product kernels on the same inputs against the oracle's dense matrix: query counts around the
    16-query block, candidate counts around the 64-candidate chunk, strings of 0, 1, 31 and 32 bytes, 32- and 64-bit offsets; then one
    candidate of 33 bytes on raw tapes (the kernels report it and the call is redone); and the range search again on three forced
    slices (STRINGWARS_AMD_WITHIN_SLICES=3, a child on the test library)."""
    in_child = run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_WITHIN_SLICES="3"), test_library=True)
    engine = sw.LevenshteinDistances(capabilities=scope)
    q, c, d = _word_edge_case(False)
    scope.set_profiling(True)
    try:
        for w in (np.uint32, np.uint64):
            pq, pc = sw.PreparedTape(scope, q.with_offsets(w)), sw.PreparedTape(scope, c.with_offsets(w))
            if in_child:
                assert os.environ["STRINGWARS_AMD_WITHIN_SLICES"] == "3" and sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
                for bound in (0, 2, 40):
                    want = expected_csr(d, bound)
                    check_csr(engine.within(pq, pc, scope, bound=bound, capacity=33 * 129), want, f"three slices {w.__name__} bound {bound}")
                    timing = scope.last_timing()
                    assert timing["dominant_name"] == "cross_within", timing
                    assert _fused_slices(timing, 33, 129, int(q.lengths.sum()) + int(c.lengths.sum()), int(want[0][-1]), np.dtype(w).itemsize) == 3, timing
                continue
            for nq in QUERY_COUNTS:
                for nc in WORD_EDGE_CANDIDATES:
                    what, part = f"{w.__name__} {nq} x {nc}", d[:nq, :nc]
                    assert (np.asarray(engine(pq[:nq], pc[:nc], scope)).astype(np.int64) == part).all(), what
                    assert scope.last_timing()["dominant_name"] == "cross_short", (what, scope.last_timing())
                    for bound in (0, 2, None):
                        check_rows(engine.topk(pq[:nq], pc[:nc], scope, k=64, bound=bound), expected_topk(part, 64, bound), f"{what} top-k bound {bound}")
                        assert "cross_topk" in scope.last_timing()["dominant_name"], (what, scope.last_timing())
                    for bound in (0, 2, 40):
                        check_csr(engine.within(pq[:nq], pc[:nc], scope, bound=bound), expected_csr(part, bound), f"{what} within bound {bound}")
                        assert scope.last_timing()["dominant_name"] == "cross_within", (what, scope.last_timing())
    finally:
        scope.set_profiling(False)
    if in_child:
        return
    q, c, d = _word_edge_case(True)
    assert (np.asarray(engine(q, c, scope)).astype(np.int64) == d).all()
    for bound in (0, 2, None):
        check_rows(engine.topk(q, c, scope, k=64, bound=bound), expected_topk(d, 64, bound), f"a 33-byte candidate, top-k bound {bound}")
    for bound in (0, 2, 40):
        check_csr(engine.within(q, c, scope, bound=bound), expected_csr(d, bound), f"a 33-byte candidate, within bound {bound}")


@pytest.mark.gpu
def test_within_one_natural_slice(sw, orc, scope):
    """131 072 queries (8192 blocks of 16: at least 32 per compute unit) drawn from 33 against 700 candidates: one slice by the rule."""
    nq, nc = 131_072, 700
    queries, candidates, d_pool, index = _pooled_staircase(sw, orc, nq, nc)
    engine = sw.LevenshteinDistances(capabilities=scope)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    scope.set_profiling(True)
    try:
        for bound in (0, 1):
            want = expected_csr_pooled(d_pool, index, bound)
            total = int(want[0][-1])
            check_csr(engine.within(pq, pc, scope, bound=bound, capacity=total), want, f"one slice bound {bound}")
            timing = scope.last_timing()
            assert timing["dominant_name"] == "cross_within" and timing["kernels"] == 4, timing   # count, sums, offsets, fill
            assert _fused_slices(timing, nq, nc, int(queries.lengths.sum()) + int(candidates.lengths.sum()), total) == 1, timing
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
def test_within_pruned_and_unpruned_walks_agree(request, sw, orc, scope):
    """d == |m - n| on prefixes of one string: the prune (no lane at |m - n| <= bound) is tight. The pruned walk (this process) and the
    walk of every chunk (STRINGWARS_AMD_WITHIN_PRUNE=0, a child on the test library) both equal the oracle."""
    in_child = run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_WITHIN_PRUNE="0"), test_library=True)
    if in_child:
        assert os.environ["STRINGWARS_AMD_WITHIN_PRUNE"] == "0" and sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    else:
        assert "STRINGWARS_AMD_WITHIN_PRUNE" not in os.environ
    engine = sw.LevenshteinDistances(capabilities=scope)
    q, c, d, _ = _fused_case("prefixes")
    for bound in BOUNDS:
        check_csr(engine.within(q, c, scope, bound=bound), expected_csr(d, bound), f"prefixes bound {bound}")
    queries, candidates, d_pool, index = _pooled_prefixes(sw, orc, 2048)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    for bound in (0, 1, 3):
        check_csr(engine.within(pq, pc, scope, bound=bound), expected_csr_pooled(d_pool, index, bound), f"prefixes x 2048 bound {bound}")


@pytest.mark.gpu
def test_within_fused_and_select_routes_agree(request, sw, scope):
    """The sweep's inputs on the fused kernel (this process) and on the general path (STRINGWARS_AMD_WITHIN_ROUTE=select, a child on the
    test library): the same output -- the oracle's -- from both, and the name and the cells the header promises for each."""
    in_child = run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_WITHIN_ROUTE="select"), test_library=True)
    if in_child:
        assert os.environ["STRINGWARS_AMD_WITHIN_ROUTE"] == "select" and sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    engine = sw.LevenshteinDistances(capabilities=scope)
    scope.set_profiling(True)
    try:
        for name in FUSED_INPUTS:
            q, c, d, _ = _fused_case(name)
            pq, pc = sw.PreparedTape(scope, q), sw.PreparedTape(scope, c)
            for bound in BOUNDS:
                for capacity in (33 * 640, None):   # one call that fits, and the wrapper's own guess (a second call when it does not)
                    check_csr(engine.within(pq, pc, scope, bound=bound, capacity=capacity), expected_csr(d, bound), f"{name} bound {bound}")
                    timing = scope.last_timing()
                    assert timing["cells"] == int(q.lengths.sum()) * int(c.lengths.sum()), timing   # counted once, walked twice
                    if in_child:
                        assert timing["dominant_name"].startswith("within_select/"), timing
                    else:
                        assert timing["dominant_name"] == "cross_within", timing
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
def test_within_code_points(sw, orc, scope):
    """tests/golden/uwords.npz (all of it: 24 x 40 words of four scripts) on the UTF-8 engine, against the recorded matrix and the oracle."""
    z = np.load(os.path.join(GOLDEN, "uwords.npz"))
    q, c = sw.Strs(data=z["q_data"], offsets=z["q_offsets"].astype(np.uint64)), sw.Strs(data=z["c_data"], offsets=z["c_offsets"].astype(np.uint64))
    d = z["lev_utf8"].astype(np.int64)
    assert (d == oracle_matrix(sw, orc, q, c, utf8=True)).all()
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope)
    pq, pc = sw.PreparedTape(scope, q, utf8=True), sw.PreparedTape(scope, c, utf8=True)
    assert ((d <= 2).sum(axis=1) == 0).any() and (d <= 2).any()
    scope.set_profiling(True)
    try:
        for bound in (0, 2, 5, 100):
            want = expected_csr(d, bound)
            check_csr(engine.within(q, c, scope, bound=bound), want, f"uwords bound {bound}")
            check_csr(engine.within(pq, pc, scope, bound=bound), want, f"prepared uwords bound {bound}")
            assert scope.last_timing()["dominant_name"].startswith("within_select/"), scope.last_timing()
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
def test_within_general_path_inputs(sw, orc, scope):
    engine = sw.LevenshteinDistances(capabilities=scope)
    # one 33-byte string among word-sized candidates: not the fused kernel's
    q, c, d, _ = _fused_case("staircase")
    items = [c[j] for j in range(130)]
    items[67] = CENTRE + b"xyz"
    assert len(items[67]) == 33
    misfit = sw.Strs(items)
    d_misfit = oracle_matrix(sw, orc, q, misfit)
    scope.set_profiling(True)
    try:
        for bound in (0, 3, 33):
            check_csr(engine.within(q, misfit, scope, bound=bound), expected_csr(d_misfit, bound), f"33 bytes, bound {bound}")
            assert scope.last_timing()["dominant_name"].startswith("within_select/"), scope.last_timing()
        assert (d_misfit[:, 67] <= 3).any() and (d_misfit <= 33).all()
        # tokens of up to 64 bytes, 64 x 64
        a, b, d_tokens = _tokens_case(sw, orc)
        for bound in (0, 8, 200):
            check_csr(engine.within(a, b, scope, bound=bound), expected_csr(d_tokens, bound), f"tokens64 bound {bound}")
            check_csr(engine.within(sw.PreparedTape(scope, a), sw.PreparedTape(scope, b), scope, bound=bound), expected_csr(d_tokens, bound),
                      f"prepared tokens64 bound {bound}")
            timing = scope.last_timing()
            assert timing["dominant_name"].startswith("within_select/") and timing["cells"] == int(a.lengths.sum()) * int(b.lengths.sum()), timing
        # general costs on strings of ~100 symbols, 8 x 40
        q, c, d_costs = _costs_case(sw, orc)
        costly = sw.LevenshteinDistances(*COSTS, capabilities=scope)
        for bound in (COSTS_BOUND, 10_000):
            check_csr(costly.within(q, c, scope, bound=bound), expected_csr(d_costs, bound), f"costs bound {bound}")
            check_csr(costly.within(sw.PreparedTape(scope, q), sw.PreparedTape(scope, c), scope, bound=bound), expected_csr(d_costs, bound),
                      f"prepared costs bound {bound}")
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["two_blocks_three_slices", "one_block_two_slices"])
def test_within_general_path_blocks(sw, orc, scope, shape):
    """The general path beyond one block, at the shapes of test_topk_general_path_blocks: 2^18 + 37 queries x 600 candidates are two query
    blocks (row_first != 0) of three slices (256, 256, 88 columns: a row's cursor carried from slice to slice); 9000 x 9000 is one block
    of 7456 + 1544 columns. Each slice is scored in both sweeps."""
    pool, items, queries, index, _, _ = _general_blocks_input(sw, shape)
    launches = {"two_blocks_three_slices": 2 * (6 * 2) + 2, "one_block_two_slices": 2 * (2 * 2) + 2}[shape]
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope)
    candidates = sw.Strs(items)
    d_pool = oracle_matrix(sw, orc, sw.Strs(pool), candidates, utf8=True)
    pq, pc = sw.PreparedTape(scope, queries, utf8=True), sw.PreparedTape(scope, candidates, utf8=True)
    for bound in (0, 1):
        want = expected_csr_pooled(d_pool, index, bound)
        scope.set_profiling(True)
        got = engine.within(pq, pc, scope, bound=bound, capacity=int(want[0][-1]))
        timing = scope.last_timing()
        scope.set_profiling(False)
        check_csr(got, want, f"{shape} bound {bound}")
        assert timing["dominant_name"].startswith("within_select/") and timing["kernels"] >= launches, timing


def _raw_call(sw, scope, engine, q, c, bound, offsets, indices, distances, capacity):
    from stringwars_amd import _native as N
    from stringwars_amd.engines import _c_tape
    tq, _, keep_q = _c_tape(q, want64=True)
    tc, _, keep_c = _c_tape(c, want64=True)
    err = C.c_char_p()
    pointer = lambda a: C.c_void_p(a.ctypes.data if a is not None else None)
    return N.lib.swh_levenshtein_within_u64tape(engine._handle, scope.handle, C.byref(tq), C.byref(tc), C.c_uint32(bound), pointer(offsets),
                                                pointer(indices), pointer(distances), capacity, C.byref(err))


@pytest.mark.gpu
def test_within_counting_protocol(sw, scope):
    from stringwars_amd import _native as N
    q, c, d, _ = _fused_case("staircase")
    engine = sw.LevenshteinDistances(capabilities=scope)
    want = expected_csr(d, 3)
    total = int(want[0][-1])
    SENTINEL = 0xABABABAB
    fresh = lambda n: (np.full(n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32))
    # the counting call: NULL, NULL, 0 gives the offsets of the full call
    offsets = np.full(34, 77, np.uint64)
    assert _raw_call(sw, scope, engine, q, c, 3, offsets, None, None, 0) == N.SUCCESS and (offsets == want[0]).all()
    # one entry too few: success, full offsets, the arrays untouched
    offsets = np.full(34, 77, np.uint64)
    indices, distances = fresh(total)
    assert _raw_call(sw, scope, engine, q, c, 3, offsets, indices, distances, total - 1) == N.SUCCESS
    assert (offsets == want[0]).all() and (indices == SENTINEL).all() and (distances == SENTINEL).all()
    # exactly enough
    offsets = np.full(34, 77, np.uint64)
    assert _raw_call(sw, scope, engine, q, c, 3, offsets, indices, distances, total) == N.SUCCESS
    check_csr((offsets, indices, distances), want, "capacity == total")
    # more than enough: the entries beyond the total stay as they were
    indices, distances = fresh(total + 9)
    assert _raw_call(sw, scope, engine, q, c, 3, offsets, indices, distances, total + 9) == N.SUCCESS
    check_csr((offsets, indices, distances), want, "capacity > total")
    assert (indices[total:] == SENTINEL).all() and (distances[total:] == SENTINEL).all()
    # refused, with nothing written: no bound, one array without the other, arrays without offsets, a capacity without arrays
    for bound, use_offsets, use_indices, use_distances, capacity in ((sw.UNBOUNDED, True, True, True, total), (3, True, True, False, total),
                                                                     (3, True, False, True, total), (3, False, True, True, total),
                                                                     (3, True, False, False, total)):
        offsets = np.full(34, 77, np.uint64)
        indices, distances = fresh(total)
        status = _raw_call(sw, scope, engine, q, c, bound, offsets if use_offsets else None, indices if use_indices else None,
                           distances if use_distances else None, capacity)
        assert status != N.SUCCESS, (bound, use_offsets, use_indices, use_distances)
        assert (offsets == 77).all() and (indices == SENTINEL).all() and (distances == SENTINEL).all()
    with pytest.raises(sw.StringWarsError) as info:   # the same refusal through the C ABI's error path, by name
        err = C.c_char_p()
        N.check(_raw_call(sw, scope, engine, q, c, sw.UNBOUNDED, np.zeros(34, np.uint64), *fresh(total), total), err)
    assert info.value.status == "invalid_argument"
    with pytest.raises(ValueError):
        engine.within(q, c, scope, bound=None)
    # the wrapper's retry: a first call with room for one hit, a second with the exact size
    check_csr(engine.within(q, c, scope, bound=3, capacity=1), want, "capacity=1")
    check_csr(engine.within(q, c, scope, bound=3), want, "default capacity")
    assert len(engine.within(q, c, scope, bound=3, capacity=1).indices) == total


@pytest.mark.gpu
def test_within_outputs_on_host_and_device(sw, scope):
    import torch
    q, c, d, _ = _fused_case("heavy_ties")
    engine = sw.LevenshteinDistances(capabilities=scope)
    general = sw.LevenshteinDistances(capabilities=scope, algorithm="wavefront")   # never the fused kernel
    pq, pc = sw.PreparedTape(scope, q), sw.PreparedTape(scope, c)
    want = expected_csr(d, 1)
    total = int(want[0][-1])
    for where in range(8):   # each of the three outputs on the device or on the host, independently
        def make(bit, n, host_dtype, device_dtype):
            return torch.full((n,), 7, dtype=device_dtype, device="cuda") if where >> bit & 1 else np.full(n, 7, host_dtype)
        for which in (engine, general):
            out = make(0, 34, np.uint64, torch.int64), make(1, total + 5, np.uint32, torch.int32), make(2, total + 5, np.uint32, torch.int32)
            got = which.within(pq, pc, scope, bound=1, out=out)
            check_csr(got, want, f"out {where:03b}")
            check_csr(out, want, f"out {where:03b}, the arrays themselves")
            assert (_host(out[1])[total:] == 7).all() and (_host(out[2])[total:] == 7).all()
            assert got.row(32)[0].tolist() == want[1][int(want[0][32]):].tolist()
    # too small: the offsets are written, the arrays are not, and the wrapper says so
    out = np.full(34, 7, np.uint64), torch.full((total - 1,), 7, dtype=torch.int32, device="cuda"), np.full(total - 1, 7, np.uint32)
    with pytest.raises(ValueError):
        engine.within(pq, pc, scope, bound=1, out=out)
    assert (out[0] == want[0]).all() and (_host(out[1]) == 7).all() and (out[2] == 7).all()
    # the counting call through the wrapper
    out = torch.zeros(34, dtype=torch.int64, device="cuda"), None, None
    counted = engine.within(pq, pc, scope, bound=1, out=out)
    assert (_host(out[0]).view(np.uint64) == want[0]).all() and (counted.counts == np.diff(want[0])).all() and counted.indices is None
    with pytest.raises(ValueError):
        counted.row(0)


@pytest.mark.gpu
def test_within_offset_widths_views_and_self(sw, orc, scope):
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = sw.generate_pairs("short_words", 1500, seed=47)
    queries = queries[:200]
    d = oracle_matrix(sw, orc, queries, candidates)
    tapes = {(w, side): sw.PreparedTape(scope, strs.with_offsets(w)) for w in (np.uint32, np.uint64) for side, strs in (("q", queries), ("c", candidates))}
    scope.set_profiling(True)
    try:
        for w in (np.uint32, np.uint64):
            for bound in (0, 2, 4):
                check_csr(engine.within(tapes[(w, "q")], tapes[(w, "c")], scope, bound=bound), expected_csr(d, bound), f"{w.__name__} bound {bound}")
                assert scope.last_timing()["dominant_name"] == "cross_within", (w, scope.last_timing())
            # sub-views at the start, in the middle and at the tail of the prepared tapes
            for (q0, q1), (c0, c1) in (((0, 50), (0, 700)), ((37, 170), (69, 1000)), ((150, 200), (801, 1500))):
                check_csr(engine.within(tapes[(w, "q")][q0:q1], tapes[(w, "c")][c0:c1], scope, bound=2), expected_csr(d[q0:q1, c0:c1], 2),
                          f"{w.__name__} views {q0}:{q1} x {c0}:{c1}")
        for wq, wc in ((np.uint32, np.uint64), (np.uint64, np.uint32)):   # mixed widths of byte tapes: refused, nothing written
            out = np.full(201, 77, np.uint64), np.full(100, 77, np.uint32), np.full(100, 77, np.uint32)
            with pytest.raises(sw.StringWarsError) as info:
                engine.within(tapes[(wq, "q")], tapes[(wc, "c")], scope, bound=1, out=out)
            assert info.value.status == "invalid_argument" and all((a == 77).all() for a in out)
    finally:
        scope.set_profiling(False)
    # the self-search equals the search with the tape passed twice; pairs(upper=True) is its i < j half
    d_self = oracle_matrix(sw, orc, queries, queries)
    want = expected_csr(d_self, 2)
    for tape in (queries, tapes[(np.uint32, "q")], tapes[(np.uint64, "q")]):
        alone, twice = engine.within(tape, None, scope, bound=2), engine.within(tape, tape, scope, bound=2)
        check_csr(alone, want, "self")
        check_csr(twice, want, "the tape twice")
        i, j, dist = alone.pairs(upper=True)
        rows, columns = np.nonzero(np.triu(d_self <= 2, k=1))
        assert (i == rows).all() and (j == columns).all() and (dist == d_self[rows, columns]).all()
        assert (alone.counts >= 1).all()   # the diagonal


@pytest.mark.gpu
def test_within_prepared_tape_changed_after_it_was_measured(sw, orc, scope):
    """A candidate of a prepared DEVICE tape has grown beyond 32 bytes since it was measured: the count pass reports it and the search is
    redone on the general path, as top-k does."""
    from stringwars_amd import _native as N
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = sw.generate_pairs("short_words", 2000, seed=53)
    queries = queries[:300]
    device = candidates.to_device(scope)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, device)
    scope.set_profiling(True)
    try:
        check_csr(engine.within(pq, pc, scope, bound=2), expected_csr(oracle_matrix(sw, orc, queries, candidates), 2), "before the change")
        assert scope.last_timing()["dominant_name"] == "cross_within"
        changed = candidates.offsets.copy()
        at = 700
        while int(changed[at + 12]) - int(changed[at]) <= 32:
            at += 1
        changed[at + 1:at + 12] = changed[at + 12]   # candidate `at` now spans twelve words, the eleven behind it are empty
        N.check(N.lib.swh_copy_to_device(scope.handle, C.c_void_p(device.offsets_ptr), changed.ctypes.data, changed.nbytes, None), C.c_char_p())
        now = sw.Strs(data=candidates.data, offsets=changed)
        check_csr(engine.within(pq, pc, scope, bound=2), expected_csr(oracle_matrix(sw, orc, queries, now), 2), "after the change")
        assert scope.last_timing()["dominant_name"].startswith("within_select/"), scope.last_timing()
    finally:
        scope.set_profiling(False)
    scope.synchronize()


@pytest.mark.gpu
def test_within_agrees_with_the_dense_product_and_topk(sw, scope):
    """1024 x 100 000 words, bound 2, no oracle: the rows equal the dense product filtered (in slabs of 128 queries), and every row with
    at most 64 hits equals topk(k=64, bound=2) put back into candidate order."""
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, _ = sw.generate_pairs("short_words", 1024, seed=17)
    _, candidates = sw.generate_pairs("short_words", 100_000, seed=18)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    got = engine.within(pq, pc, scope, bound=2)
    offsets = got.offsets.astype(np.int64)
    for first in range(0, 1024, 128):
        dense = engine(pq[first:first + 128], pc, scope)
        want = expected_csr(dense.astype(np.int64), 2)
        lo, hi = offsets[first], offsets[first + 128]
        assert (offsets[first:first + 129] - lo == want[0].astype(np.int64)).all(), first
        assert (got.indices[lo:hi] == want[1]).all() and (got.distances[lo:hi] == want[2]).all(), first
    indices, distances = engine.topk(pq, pc, scope, k=64, bound=2)
    counts = got.counts
    assert (counts <= 64).any() and (counts > 64).any()
    for i in np.flatnonzero(counts <= 64):
        n = int(counts[i])
        order = np.argsort(indices[i, :n], kind="stable")
        ri, rd = got.row(int(i))
        assert (indices[i, :n][order] == ri).all() and (distances[i, :n][order] == rd).all() and (indices[i, n:] == 0xFFFFFFFF).all(), i


@pytest.mark.gpu
def test_within_beyond_the_dense_reach(sw, orc, scope):
    """66 000 x 66 000 words: 4.36e9 pairs -- more than one dense call takes -- in one range search (the wrapper's second call holds the hits)."""
    engine = sw.LevenshteinDistances(capabilities=scope)
    words, _ = sw.generate_pairs("short_words", 66_000, seed=23)
    prepared = sw.PreparedTape(scope, words)
    got = engine.within(prepared, None, scope, bound=1)
    assert len(got) == 66_000 and int(got.offsets[-1]) == len(got.indices) > 66_000
    rows = np.random.default_rng(1).choice(len(words), 16, replace=False)
    d = oracle_matrix(sw, orc, gather(sw, words, rows), words)
    for at, row in enumerate(rows):
        want = np.flatnonzero(d[at] <= 1)
        ri, rd = got.row(int(row))
        assert (ri == want).all() and (rd == d[at][want]).all(), row
