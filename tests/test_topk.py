"""Levenshtein top-k search (swh_levenshtein_topk_*): the k nearest candidates of every query.

Expected rows come from the CPU oracle over the expanded queries x candidates pairs, ordered by (distance, candidate index),
filtered by d <= bound, cut to k and padded with 0xFFFFFFFF (`expected_topk`)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 0xFFFFFFFF


def expected_topk(d: np.ndarray, k: int, bound=None):
    """Rows of (indices, distances) from a dense (nq, nc) distance matrix: np.lexsort((j, d)) per row, d <= bound, k, padding."""
    nq, nc = d.shape
    indices = np.full((nq, k), PAD, dtype=np.uint32)
    distances = np.full((nq, k), PAD, dtype=np.uint32)
    j = np.arange(nc)
    for i in range(nq):
        order = np.lexsort((j, d[i]))
        if bound is not None:
            order = order[d[i][order] <= bound]
        order = order[:k]
        indices[i, :len(order)] = order
        distances[i, :len(order)] = d[i][order]
    return indices, distances


def gather(sw, strs, idx):
    """A host tape holding strs[idx[0]], strs[idx[1]], ... (vectorised: the oracle's pairs are expanded products)."""
    idx = np.asarray(idx, dtype=np.int64)
    starts = strs.offsets[:-1].astype(np.int64)[idx]
    lengths = np.diff(strs.offsets.astype(np.int64))[idx]
    offsets = np.zeros(len(idx) + 1, dtype=np.uint64)
    np.cumsum(lengths, out=offsets[1:])
    total = int(offsets[-1])
    within = np.arange(total, dtype=np.int64) - np.repeat(offsets[:-1].astype(np.int64), lengths)
    data = strs.data[np.repeat(starts, lengths) + within] if total else np.zeros(0, np.uint8)
    return sw.Strs(data=data, offsets=offsets)


def oracle_matrix(sw, orc, queries, candidates, utf8=False, costs=None, algo="hyyro"):
    nq, nc = len(queries), len(candidates)
    a = gather(sw, queries, np.repeat(np.arange(nq), nc))
    b = gather(sw, candidates, np.tile(np.arange(nc), nq))
    if costs is not None:
        d = orc.levenshtein_costs_pairs(a, b, *costs)
    else:
        d = orc.levenshtein_pairs(a, b, utf8=utf8, algo=algo if not utf8 else "wf")
    return np.asarray(d, dtype=np.int64).reshape(nq, nc)


def check_rows(got, want, what=""):
    gi, gd = (np.asarray(x).reshape(want[0].shape).astype(np.uint32) for x in got)
    assert (gd == want[1]).all(), f"distances differ {what}: first bad row {np.argwhere(gd != want[1])[0]}"
    assert (gi == want[0]).all(), f"indices differ {what}: first bad row {np.argwhere(gi != want[0])[0]}"


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_topk_symbols_exported_and_announced(sw):
    from stringwars_amd import _native as N
    for name in ("swh_levenshtein_topk_u64tape", "swh_levenshtein_utf8_topk_u64tape", "swh_levenshtein_topk_prepared"):
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    assert "topk" in sw.capabilities().split(",")
    assert callable(getattr(sw.LevenshteinDistances, "topk")) and callable(getattr(sw.LevenshteinDistancesUTF8, "topk"))


def test_topk_limit_matches_header(sw):
    header = open(os.path.join(ROOT, "include", "stringwars_amd.h")).read()
    found = re.search(r"#define\s+SWH_TOPK_MAX\s+(\d+)", header)
    assert found and int(found.group(1)) == sw.TOPK_MAX == 64


def test_expected_rows_helper_on_ties():
    d = np.array([[3, 1, 1, 0, 2, 1],
                  [5, 5, 5, 5, 5, 5],
                  [0, 9, 0, 9, 0, 9]])
    indices, distances = expected_topk(d, 4)
    assert indices.tolist() == [[3, 1, 2, 5], [0, 1, 2, 3], [0, 2, 4, 1]]
    assert distances.tolist() == [[0, 1, 1, 1], [5, 5, 5, 5], [0, 0, 0, 9]]
    indices, distances = expected_topk(d, 8, bound=1)
    assert indices.tolist() == [[3, 1, 2, 5] + [PAD] * 4, [PAD] * 8, [0, 2, 4] + [PAD] * 5]
    assert distances[0].tolist() == [0, 1, 1, 1] + [PAD] * 4


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _device_out(nq, k):
    import torch
    return torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.int32, device="cuda")


def _host(t):
    return t.cpu().numpy().view(np.uint32) if hasattr(t, "cpu") else t


def _utf8_words(sw, count, seed):
    """Word-sized code-point tokens: the generated multilingual lines cut into pieces of 1 .. 10 code points."""
    lines, _ = sw.generate_pairs("utf8_lines", 64, seed=seed)
    rng = np.random.default_rng(seed)
    words = []
    for i in range(len(lines)):
        text = lines[i].decode("utf-8")
        at = 0
        while at < len(text) and len(words) < count:
            n = int(rng.integers(1, 11))
            words.append(text[at:at + n])
            at += n
    return sw.Strs(words[:count])


CASES = {   # workload -> (queries, candidates, bounds)
    "short_words": (200, 3000, (None, 0, 3)),
    "words16": (200, 3000, (None, 0, 3)),
    "tokens64": (32, 200, (None, 0, 3)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("workload", sorted(CASES))
def test_topk_bytes_match_oracle(sw, orc, scope, workload):
    nq, nc, bounds = CASES[workload]
    queries, candidates = sw.generate_pairs(workload, max(nq, nc) + 16, seed=7)
    q, c = queries[:nq], candidates[:nc]
    d = oracle_matrix(sw, orc, q, c)
    engine = sw.LevenshteinDistances(capabilities=scope)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    for k in (1, 5, 64):
        for bound in bounds:
            want = expected_topk(d, k, bound)
            check_rows(engine.topk(q, c, scope, k=k, bound=bound), want, f"raw {workload} k={k} bound={bound}")
            check_rows(engine.topk(pq[:nq], pc[:nc], scope, k=k, bound=bound), want, f"prepared {workload} k={k} bound={bound}")
            out = _device_out(nq, k)
            engine.topk(pq[:nq], pc[:nc], scope, k=k, bound=bound, out=out)
            check_rows(tuple(_host(t) for t in out), want, f"device out {workload} k={k} bound={bound}")
    # a sub-view that does not start at the tape's first string
    d_sub = oracle_matrix(sw, orc, queries[8:8 + nq // 2], candidates[16:16 + nc // 2])
    check_rows(engine.topk(pq[8:8 + nq // 2], pc[16:16 + nc // 2], scope, k=5, bound=3), expected_topk(d_sub, 5, 3), "sub-views")


@pytest.mark.gpu
def test_topk_utf8_matches_oracle(sw, orc, scope):
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope)
    lines, others = sw.generate_pairs("utf8_lines", 200, seed=9)
    q, c = lines[:32], others[:200]
    d = oracle_matrix(sw, orc, q, c, utf8=True)
    pq, pc = sw.PreparedTape(scope, q, utf8=True), sw.PreparedTape(scope, c, utf8=True)
    for k in (1, 5, 64):
        for bound in (None, 0, 3, 32):
            want = expected_topk(d, k, bound)
            check_rows(engine.topk(q, c, scope, k=k, bound=bound), want, f"lines k={k} bound={bound}")
            check_rows(engine.topk(pq, pc, scope, k=k, bound=bound), want, f"prepared lines k={k} bound={bound}")
    words = _utf8_words(sw, 3200, seed=11)
    q, c = words[:200], words[200:3200]
    d = oracle_matrix(sw, orc, q, c, utf8=True)
    pq, pc = sw.PreparedTape(scope, words, utf8=True), None
    for k in (1, 5, 64):
        for bound in (None, 0, 3):
            want = expected_topk(d, k, bound)
            check_rows(engine.topk(q, c, scope, k=k, bound=bound), want, f"words k={k} bound={bound}")
            check_rows(engine.topk(pq[:200], pq[200:3200], scope, k=k, bound=bound), want, f"prepared words k={k} bound={bound}")


@pytest.mark.gpu
def test_topk_heavy_ties_follow_the_index_rule(sw, orc, scope):
    every = [b""] + [bytes(s) for n in range(1, 5) for s in np.array(np.meshgrid(*[[97, 98]] * n)).T.reshape(-1, n).astype(np.uint8)]
    rng = np.random.default_rng(3)
    q = sw.Strs(every)
    c = sw.Strs([every[i] for i in rng.integers(0, len(every), 700)])
    d = oracle_matrix(sw, orc, q, c)
    fused = sw.LevenshteinDistances(capabilities=scope)
    general = sw.LevenshteinDistances(capabilities=scope, algorithm="wavefront")   # never the fused kernel
    pq, pc = sw.PreparedTape(scope, q), sw.PreparedTape(scope, c)
    for k in (1, 5, 64):
        for bound in (None, 0, 2):
            want = expected_topk(d, k, bound)
            check_rows(fused.topk(pq, pc, scope, k=k, bound=bound), want, f"fused k={k} bound={bound}")
            check_rows(general.topk(q, c, scope, k=k, bound=bound), want, f"general k={k} bound={bound}")


@pytest.mark.gpu
def test_topk_edges(sw, orc, scope):
    engine = sw.LevenshteinDistances(capabilities=scope)
    words, others = sw.generate_pairs("short_words", 300, seed=5)
    q, c = words[:40], others[:20]
    # k beyond the candidates: the rest of every row is padding
    d = oracle_matrix(sw, orc, q, c)
    check_rows(engine.topk(q, c, scope, k=64), expected_topk(d, 64), "k > candidates")
    check_rows(engine.topk(sw.PreparedTape(scope, q), sw.PreparedTape(scope, c), scope, k=30, bound=2), expected_topk(d, 30, 2), "prepared k > candidates")
    # zero candidates, zero queries
    indices, distances = engine.topk(q, sw.Strs([]), scope, k=3)
    assert (indices == PAD).all() and (distances == PAD).all()
    indices, distances = engine.topk(sw.Strs([]), c, scope, k=3)
    assert indices.shape == (0, 3)
    # the self-product: column i of row i at distance 0 (the first of the ties at 0)
    d_self = oracle_matrix(sw, orc, words, words)
    indices, distances = engine.topk(words, None, scope, k=4)
    check_rows((indices, distances), expected_topk(d_self, 4), "self")
    assert (distances[:, 0] == 0).all()
    check_rows(engine.topk(sw.PreparedTape(scope, words), None, scope, k=4), expected_topk(d_self, 4), "prepared self")
    # a 40-byte string among the words of raw tapes
    items = [c[i] for i in range(len(c))]
    items[7] = b"x" * 40
    misfit = sw.Strs(items)
    d = oracle_matrix(sw, orc, q, misfit)
    for k in (1, 5):
        check_rows(engine.topk(q, misfit, scope, k=k), expected_topk(d, k), f"misfit k={k}")
    # invalid k
    for k in (0, sw.TOPK_MAX + 1):
        with pytest.raises(sw.StringWarsError) as info:
            engine.topk(q, c, scope, k=k)
        assert info.value.status == "invalid_argument"


@pytest.mark.gpu
def test_topk_general_costs_long_strings(sw, orc, scope):
    rng = np.random.default_rng(21)
    def strings(count):
        return sw.Strs([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n))) for n in rng.integers(33, 601, count)])
    q, c = strings(16), strings(120)
    costs = (0, 2, 3, 1)
    d = oracle_matrix(sw, orc, q, c, costs=costs)
    engine = sw.LevenshteinDistances(*costs, capabilities=scope)
    pq, pc = sw.PreparedTape(scope, q), sw.PreparedTape(scope, c)
    for k in (1, 5, 64):
        for bound in (None, 400):
            want = expected_topk(d, k, bound)
            check_rows(engine.topk(q, c, scope, k=k, bound=bound), want, f"costs k={k} bound={bound}")
            check_rows(engine.topk(pq, pc, scope, k=k, bound=bound), want, f"prepared costs k={k} bound={bound}")


@pytest.mark.gpu
def test_topk_route_and_profile(sw, orc, scope):
    engine = sw.LevenshteinDistances(capabilities=scope)
    words, others = sw.generate_pairs("short_words", 2048, seed=13)
    lines, more = sw.generate_pairs("tokens64", 64, seed=13)
    scope.set_profiling(True)
    try:
        engine.topk(sw.PreparedTape(scope, words), sw.PreparedTape(scope, others), scope, k=8)
        timing = scope.last_timing()
        assert timing["dominant_name"] == "cross_topk" or "cross_topk" in timing["dominant_name"], timing
        assert timing["cells"] == int(words.lengths.sum()) * int(others.lengths.sum())
        engine.topk(sw.PreparedTape(scope, lines), sw.PreparedTape(scope, more), scope, k=8)
        timing = scope.last_timing()
        assert timing["dominant_name"].startswith("topk_select/"), timing
        assert timing["cells"] == int(lines.lengths.sum()) * int(more.lengths.sum())
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
def test_topk_agrees_with_the_dense_product(sw, scope):
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, _ = sw.generate_pairs("short_words", 1024, seed=17)
    _, candidates = sw.generate_pairs("short_words", 100_000, seed=18)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    k = 16
    indices, distances = engine.topk(pq, pc, scope, k=k, bound=4)
    j = np.arange(len(candidates), dtype=np.uint64)
    for first in range(0, 1024, 128):
        dense = engine(pq[first:first + 128], pc, scope)
        keys = np.sort((dense.astype(np.uint64) << np.uint64(32)) | j, axis=1)[:, :k]
        want_d = (keys >> np.uint64(32)).astype(np.int64)
        want_i = (keys & np.uint64(PAD)).astype(np.int64)
        keep = want_d <= 4
        want_i, want_d = np.where(keep, want_i, PAD), np.where(keep, want_d, PAD)
        assert (distances[first:first + 128] == want_d).all() and (indices[first:first + 128] == want_i).all(), first


@pytest.mark.gpu
def test_topk_beyond_the_dense_reach(sw, orc, scope):
    """66 000 x 66 000 words: 4.36e9 pairs -- more than one dense call takes -- in one top-k call."""
    import torch
    engine = sw.LevenshteinDistances(capabilities=scope)
    words, _ = sw.generate_pairs("short_words", 66_000, seed=23)
    prepared = sw.PreparedTape(scope, words)
    with pytest.raises(sw.StringWarsError) as info:   # refused before anything is written: the output is never touched
        engine(prepared, prepared, scope, out=torch.empty(1, dtype=torch.int64, device="cuda"))
    assert info.value.status == "unsupported_length"
    k = 8
    indices, distances = engine.topk(prepared, None, scope, k=k)
    rows = np.random.default_rng(1).choice(len(words), 16, replace=False)
    d = oracle_matrix(sw, orc, gather(sw, words, rows), words)
    want = expected_topk(d, k)
    check_rows((indices[rows], distances[rows]), want, "66 000 x 66 000")
