"""Levenshtein top-k search (swh_levenshtein_topk_*): the k nearest candidates of every query.

Expected rows come from the CPU oracle over the expanded queries x candidates pairs, ordered by (distance, candidate index),
filtered by d <= bound, cut to k and padded with 0xFFFFFFFF (`expected_topk`)."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child

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


POOL_MAX = 64


def expected_topk_pooled(d_pool: np.ndarray, pool_index: np.ndarray, k: int, bound=None):
    """The rows of a search whose query i is string pool_index[i] of a small pool of distinct strings: `expected_topk` once per pool
    string (d_pool is the pool x candidates matrix), broadcast by the pool index. 10^5 queries cost the oracle what 64 do."""
    assert d_pool.shape[0] <= POOL_MAX and (np.asarray(pool_index) < d_pool.shape[0]).all()
    indices, distances = expected_topk(d_pool, k, bound)
    return indices[pool_index], distances[pool_index]


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


# ---- adversarial inputs: what each is for is asserted by the CPU tests below, on the oracle alone ---------------------------------------
CENTRE = bytes(range(0x41, 0x41 + 30))               # 30 distinct symbols
FOREIGN = np.arange(0x61, 0x7B, dtype=np.uint8)      # symbols the centre does not hold
LEVELS3 = list(range(30, -1, -3))                    # 11 distances to the centre, 3 apart: strings one edit from the centre see them disjoint
LEVELS1 = list(range(30, -1, -1))                    # 31 levels, 1 apart: neighbouring chunks share distances
AB_STRINGS = [b""] + [bytes(s) for n in range(1, 5) for s in np.array(np.meshgrid(*[[97, 98]] * n)).T.reshape(-1, n).astype(np.uint8)]
KS = (1, 2, 17, 33, 63, 64)
BOUNDS = (None, 0, 1, 3)


def centre_pool(size=48, seed=1):
    """The centre string and distinct strings one edit away from it (at most 31 bytes)."""
    rng = np.random.default_rng(seed)
    pool = {CENTRE}
    while len(pool) < size:
        s = bytearray(CENTRE)
        at, op = int(rng.integers(0, len(s))), int(rng.integers(0, 3))
        if op == 0:
            s[at] = int(rng.choice(FOREIGN))
        elif op == 1:
            s.insert(at, int(rng.choice(FOREIGN)))
        else:
            del s[at]
        pool.add(bytes(s))
    return sorted(pool)


def at_distance(rng, level):
    """The centre with `level` symbols replaced by foreign ones: its distance to the centre is `level` (the centre's symbols are
    distinct, so the longest common subsequence is what was kept), and to a string one edit from the centre level - 1 .. level + 1."""
    s = np.frombuffer(CENTRE, np.uint8).copy()
    s[rng.choice(len(s), level, replace=False)] = rng.choice(FOREIGN, level)
    return s.tobytes()


def staircase(count, levels, seed=2):
    """Chunk c (candidates 64 c .. 64 c + 63, one wave of the fused kernel) lies at distance levels[c % len(levels)] from the centre."""
    rng = np.random.default_rng(seed)
    return [at_distance(rng, levels[(j // 64) % len(levels)]) for j in range(count)]


def ordered_candidates(order, count, seed=2):
    """(pool, candidates) of one candidate order."""
    rng = np.random.default_rng(seed)
    if order == "heavy_ties":
        return AB_STRINGS, [AB_STRINGS[i] for i in rng.integers(0, len(AB_STRINGS), count)]
    if order == "descending":            # every chunk is nearer than everything before it: admitted whole into a full list
        items = staircase(count, LEVELS3, seed)
    elif order == "ascending":           # nothing is admitted once the list is full
        items = staircase(count, LEVELS3[::-1], seed)
    elif order == "descending_overlap":  # admitted keys tie with list entries of the chunk before; wraps every 31 chunks
        items = staircase(count, LEVELS1, seed)
    elif order == "ascending_overlap":
        items = staircase(count, LEVELS1[::-1], seed)
    elif order == "identical":
        items = [centre_pool()[7]] * count   # (a string of the pool: distances 0, 1 and 2, so every bound cuts some rows)
    elif order == "two_levels":          # lane by lane: near, far, near, ... and the other way round in the second half
        near, far = at_distance(rng, 2), at_distance(rng, 5)
        items = [near if (j + (j >= count // 2)) % 2 == 0 else far for j in range(count)]
    else:
        raise KeyError(order)
    return centre_pool(), items


def prefix_family(count, seed=4):
    """(pool, pool base, candidates, candidate base): prefixes of two base strings of 32 distinct symbols. Two prefixes of one base
    are at distance |m - n| exactly -- where the length-gap pruning (gap << 32 < T) is tight."""
    rng = np.random.default_rng(seed)
    bases = [bytes(rng.permutation(np.arange(0x30, 0x30 + 40, dtype=np.uint8))[:32]) for _ in range(2)]
    pool = [(bases[0][:n], 0) for n in range(33)] + [(bases[1][:n], 1) for n in range(1, 32)]
    which, lengths = rng.integers(0, 2, count), rng.integers(0, 33, count)
    lengths[:33] = np.arange(33)
    candidates = [bases[w][:n] for w, n in zip(which, lengths)]
    return [p for p, _ in pool], np.array([w for _, w in pool]), candidates, which


def pooled_queries(sw, pool, count, seed=6):
    """`count` queries drawn from the pool (every string of it among the first len(pool)): the tape and the pool index of each."""
    rng = np.random.default_rng(seed)
    index = rng.integers(0, len(pool), count)
    index[:len(pool)] = np.arange(len(pool))[:count]
    return gather(sw, sw.Strs(pool), index), index


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_pooled_rows_equal_the_unbroadcast_rows(sw, orc):
    rng = np.random.default_rng(8)
    pool = AB_STRINGS[:9]
    candidates = sw.Strs([AB_STRINGS[i] for i in rng.integers(0, len(AB_STRINGS), 90)])   # ties on every row
    queries, index = pooled_queries(sw, pool, 300)
    assert sorted(set(index.tolist())) == list(range(9))
    d_pool = oracle_matrix(sw, orc, sw.Strs(pool), candidates)
    d_full = oracle_matrix(sw, orc, queries, candidates)
    assert (d_full == d_pool[index]).all()
    for k in (1, 4, 64):
        for bound in (None, 0, 1):
            want = expected_topk(d_full, k, bound)
            got = expected_topk_pooled(d_pool, index, k, bound)
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (k, bound)
    tied = expected_topk_pooled(d_pool, index, 4, None)
    assert (np.diff(tied[1].astype(np.int64), axis=1) == 0).any() and (expected_topk_pooled(d_pool, index, 64, 0)[0] == PAD).any()


def test_candidate_orders_are_what_they_are_for(sw, orc):
    pool = centre_pool()
    assert len(set(pool)) == len(pool) <= POOL_MAX and CENTRE in pool and max(map(len, pool)) <= 32
    to_centre = oracle_matrix(sw, orc, sw.Strs(pool), sw.Strs([CENTRE]))
    assert (to_centre[:, 0] <= 1).all()

    def chunks(order, count):
        p, items = ordered_candidates(order, count)
        d = oracle_matrix(sw, orc, sw.Strs(p), sw.Strs(items))
        full = count // 64 * 64
        return d, d[:, :full].reshape(len(p), -1, 64)

    # strictly descending / ascending chunk by chunk, for every string of the pool
    d, c = chunks("descending", 700)
    assert c.shape[1] == 10 and (c.min(axis=2)[:, :-1] > c.max(axis=2)[:, 1:]).all()
    assert (d[:, 640:].max(axis=1) < c[:, -1].min(axis=1)).all()
    d, c = chunks("ascending", 700)
    assert (c.max(axis=2)[:, :-1] < c.min(axis=2)[:, 1:]).all() and (d[:, 640:].min(axis=1) > c[:, -1].max(axis=1)).all()
    # the overlapping staircase: a chunk is never farther than the one before by more than its spread, and shares distances with it
    for order, sign in (("descending_overlap", 1), ("ascending_overlap", -1)):
        _, c = chunks(order, 1984)
        assert c.shape[1] == 31
        near, far = (c[:, 1:], c[:, :-1]) if sign > 0 else (c[:, :-1], c[:, 1:])
        assert (near.max(axis=2) <= far.min(axis=2) + 1).all()
        shared = sum(np.intersect1d(c[q, i], c[q, i + 1]).size > 0 for q in range(len(pool)) for i in range(30))
        assert shared >= len(pool) * 30 // 2, shared
    d, _ = chunks("identical", 1000)
    assert (d == d[:, :1]).all() and d.min() == 0 and d.max() == 2
    d, _ = chunks("two_levels", 1500)
    assert (d[:, 0] < d[:, 1]).all() and (d[:, 0:750:2] == d[:, :1]).all() and (d[:, 1:750:2] == d[:, 1:2]).all()
    assert (d[:, 750::2] == d[:, 1:2]).all() and (d[:, 751::2] == d[:, :1]).all()
    assert (d[:, 0] <= 3).all() and (d[:, 1] >= 4).all()          # bound 3 separates the levels, bounds 0 and 1 cut into the near one
    # heavy ties: every row of every k <= 64 is ties at distance 0, ordered by candidate index alone
    d, _ = chunks("heavy_ties", 4000)
    assert len(AB_STRINGS) == 31 and (d == 0).sum(axis=1).min() >= 64


def test_prefix_family_sits_on_the_length_gap(sw, orc):
    pool, pool_base, candidates, base = prefix_family(3000)
    assert len(set(pool)) == len(pool) == POOL_MAX
    assert sorted(set(map(len, pool))) == list(range(33)) and sorted(set(map(len, candidates))) == list(range(33))
    d = oracle_matrix(sw, orc, sw.Strs(pool), sw.Strs(candidates))
    m, n = np.array(list(map(len, pool)))[:, None], np.array(list(map(len, candidates)))[None, :]
    same = pool_base[:, None] == base[None, :]
    assert (d[same] == np.abs(m - n)[same]).all() and same.sum() > 90_000
    assert (d >= np.abs(m - n)).all() and (d[~same] > np.abs(m - n)[~same]).mean() > 0.9


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


# ---- adversarial cases: warm-list folds, pruning, both routes, the general path's blocking, edges ---------------------------------------
def _search_and_check(scope, engine, queries, candidates, d_pool, index, what, *, kernels=None, fused=None, ks=KS, bounds=BOUNDS, out=None):
    """Every (k, bound) of one input: all rows against the pooled oracle rows; under profiling, the route (`fused`: k_cross_topk or the
    general path) and the number of kernels the call launched."""
    scope.set_profiling(True)
    try:
        for k in ks:
            for bound in bounds:
                want = expected_topk_pooled(d_pool, index, k, bound)
                if out is None:
                    got = engine.topk(queries, candidates, scope, k=k, bound=bound)
                else:
                    tensors = out(len(index), k)
                    engine.topk(queries, candidates, scope, k=k, bound=bound, out=tensors)
                    got = tuple(_host(t) for t in tensors)
                timing = scope.last_timing()
                check_rows(got, want, f"{what} k={k} bound={bound}")
                if fused is True:
                    assert "cross_topk" in timing["dominant_name"], (what, timing)
                elif fused is False:
                    assert timing["dominant_name"].startswith("topk_select/"), (what, timing)
                if kernels is not None:
                    assert timing["kernels"] == kernels, (what, k, bound, timing)
    finally:
        scope.set_profiling(False)


WARM_CASES = {   # regime -> (queries, kernels of the call, {order: candidates})
    # >= 32 x 256 blocks of 16 queries: one slice, every item folds all the chunks into one list, no merge kernel
    "one_slice": (131_072, 1, {"descending": 700, "ascending": 700, "descending_overlap": 1984, "identical": 1000, "two_levels": 1500,
                               "heavy_ties": 4000}),
    # 256 blocks: several slices of several chunks, then k_topk_merge (the staircases wrap: a slice starts anywhere on them)
    "several_slices": (4096, 2, {"descending_overlap": 40_000, "ascending_overlap": 40_000, "identical": 40_000, "two_levels": 40_000,
                                 "heavy_ties": 40_000}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("regime,order", [(r, o) for r in WARM_CASES for o in WARM_CASES[r][2]])
def test_topk_folds_into_a_warm_list(sw, orc, scope, regime, order):
    """The fused kernel's per-level rank counting (topk_fold_chunk) on lists that are full when a chunk arrives. That the regime was
    reached is read from the call itself: one kernel (no merge) for one slice, two for several."""
    nq, kernels, orders = WARM_CASES[regime]
    pool, items = ordered_candidates(order, orders[order])
    queries, index = pooled_queries(sw, pool, nq)
    candidates = sw.Strs(items)
    d_pool = oracle_matrix(sw, orc, sw.Strs(pool), candidates)
    engine = sw.LevenshteinDistances(capabilities=scope)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    _search_and_check(scope, engine, pq, pc, d_pool, index, f"{regime} {order}", kernels=kernels, fused=True)
    if order == "identical":   # the rows are candidates 0 .. k - 1
        indices, _ = engine.topk(pq, pc, scope, k=64)
        assert (indices == np.arange(64, dtype=np.uint32)).all()


def _pruning_inputs(sw, orc, nq):
    pool, _, items, _ = prefix_family(3000)
    queries, index = pooled_queries(sw, pool, nq)
    candidates = sw.Strs(items)
    return queries, candidates, oracle_matrix(sw, orc, sw.Strs(pool), candidates), index


@pytest.mark.gpu
def test_topk_pruned_and_unpruned_walks_agree(request, sw, orc, scope):
    """d == |m - n| on prefixes of one string: the pruning test is tight. The walk with pruning (this process) and the walk of every
    chunk (STRINGWARS_AMD_TOPK_PRUNE=0, a child on the test library) both equal the oracle, on one slice and on several."""
    in_child = run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_TOPK_PRUNE="0"), test_library=True)
    if in_child:
        assert os.environ["STRINGWARS_AMD_TOPK_PRUNE"] == "0" and sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    else:
        assert "STRINGWARS_AMD_TOPK_PRUNE" not in os.environ
    engine = sw.LevenshteinDistances(capabilities=scope)
    for nq, kernels in ((131_072, 1), (2048, 2)):
        queries, candidates, d_pool, index = _pruning_inputs(sw, orc, nq)
        pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
        _search_and_check(scope, engine, pq, pc, d_pool, index, f"prefixes x {nq}", kernels=kernels, fused=True, ks=(1, 5, 33, 64))


@pytest.mark.gpu
def test_topk_fused_and_select_routes_agree(request, sw, orc, scope):
    """The inputs of the warm-list and the pruning cases at 2048 queries, on the fused kernel (this process) and on the general path
    (STRINGWARS_AMD_TOPK_ROUTE=select, a child on the test library): the same rows -- the oracle's -- from both."""
    in_child = run_in_child(request, env=dict(TEST_LIBRARY_ENV, STRINGWARS_AMD_TOPK_ROUTE="select"), test_library=True)
    if in_child:
        assert os.environ["STRINGWARS_AMD_TOPK_ROUTE"] == "select" and sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    engine = sw.LevenshteinDistances(capabilities=scope)
    for order, count in WARM_CASES["one_slice"][2].items():
        pool, items = ordered_candidates(order, count)
        queries, index = pooled_queries(sw, pool, 2048)
        candidates = sw.Strs(items)
        d_pool = oracle_matrix(sw, orc, sw.Strs(pool), candidates)
        _search_and_check(scope, engine, sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates), d_pool, index,
                          f"{'select' if in_child else 'fused'} {order}", fused=not in_child)
    queries, candidates, d_pool, index = _pruning_inputs(sw, orc, 2048)
    _search_and_check(scope, engine, sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates), d_pool, index,
                      f"{'select' if in_child else 'fused'} prefixes", fused=not in_child)


def _code_point_words(count, seed, alphabet="aé中ж😀bc"):
    """Distinct non-ASCII words of 1 .. 6 code points (every word holds a non-ASCII symbol: the UTF-8 engine cannot take them as bytes)."""
    rng = np.random.default_rng(seed)
    words = set()
    while len(words) < count:
        word = "".join(rng.choice(list(alphabet), int(rng.integers(1, 7))))
        if not word.isascii():
            words.add(word)
    return sorted(words)


def _pool_and_words(count, seed=31):
    """40 pool words and `count` other words, all distinct."""
    every = _code_point_words(count + 40, seed)
    chosen = set(np.random.default_rng(seed).choice(len(every), 40, replace=False).tolist())
    return [w for i, w in enumerate(every) if i in chosen], [w for i, w in enumerate(every) if i not in chosen]


AE_STRINGS = [s.decode().replace("b", "é") for s in AB_STRINGS]   # the heavy-ties strings over {a, é}


def _planted(words, pool, first, last):
    """`words` with the first half of the pool planted inside [0, first) and the second half inside [last, len(words)): a query's
    nearest candidate (distance 0) then sits in the first slice for some queries and in the last for others."""
    items = list(words)
    half = len(pool) // 2
    step = (len(items) - last) // (len(pool) - half)
    assert step >= 1 and 3 + 7 * half < first
    for i, word in enumerate(pool):
        items[3 + 7 * i if i < half else last + 1 + step * (i - half)] = word
    return items


def test_planted_candidates_sit_in_the_first_and_last_slice(sw, orc):
    for count, first, last in ((600, 256, 512), (9000, 7456, 7456)):
        pool, words = _pool_and_words(count)
        items = _planted(words, pool, first, last)
        assert len(items) == count and len(pool) == 40 and not set(pool) & set(words)
        d = oracle_matrix(sw, orc, sw.Strs(pool), sw.Strs(items), utf8=True)
        nearest = expected_topk(d, 1)[0][:, 0]
        assert (d.min(axis=1) == 0).all() and (nearest[:20] < first).all() and (nearest[20:] >= last).all()
    # the heavy-ties rows have ties on both sides of the slice edges at 256 and 512
    rng = np.random.default_rng(33)
    items = [AE_STRINGS[i] for i in rng.integers(0, len(AE_STRINGS), 600)]
    d = oracle_matrix(sw, orc, sw.Strs(AE_STRINGS), sw.Strs(items), utf8=True)
    indices, distances = expected_topk(d, 64)
    for edge in (256, 512):
        straddles = [any((indices[q][distances[q] == v] < edge).any() and (indices[q][distances[q] == v] >= edge).any()
                         for v in np.unique(distances[q])) for q in range(len(AE_STRINGS))]
        assert sum(straddles) >= 10, (edge, sum(straddles))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["two_blocks_three_slices", "one_block_two_slices"])
def test_topk_general_path_blocks(sw, orc, scope, shape):
    """The general path beyond one block: query blocks of 2^18 rows x candidate slices of 2^26 / rows columns (non-ASCII words on the
    UTF-8 engine never take the fused kernel). 2^18 + 37 queries x 600 candidates are two query blocks (row_first != 0) of three
    slices (256, 256, 88 columns: col_first != 0, lists carried through scratch); 9000 x 9000 is one block of 7456 + 1544 columns.
    Every slice is at least one scoring kernel and one k_topk_select."""
    nq, nc, first, last, launches = {"two_blocks_three_slices": ((1 << 18) + 37, 600, 256, 512, 12),
                                     "one_block_two_slices": (9000, 9000, 7456, 7456, 4)}[shape]
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope)
    pool, words = _pool_and_words(nc)
    inputs = [("planted", pool, _planted(words, pool, first, last))]
    rng = np.random.default_rng(33)
    inputs.append(("heavy ties", AE_STRINGS, [AE_STRINGS[i] for i in rng.integers(0, len(AE_STRINGS), nc)]))
    for name, pool, items in inputs:
        queries, index = pooled_queries(sw, pool, nq)
        candidates = sw.Strs(items)
        d_pool = oracle_matrix(sw, orc, sw.Strs(pool), candidates, utf8=True)
        pq, pc = sw.PreparedTape(scope, queries, utf8=True), sw.PreparedTape(scope, candidates, utf8=True)
        scope.set_profiling(True)
        engine.topk(pq, pc, scope, k=5)
        timing = scope.last_timing()
        scope.set_profiling(False)
        assert timing["dominant_name"].startswith("topk_select/") and timing["kernels"] >= launches, timing
        for out in (None, _device_out):
            _search_and_check(scope, engine, pq, pc, d_pool, index, f"{shape} {name} {'host' if out is None else 'device'}", fused=False,
                              ks=(1, 5, 64), bounds=(None, 1), out=out)
    if shape == "one_block_two_slices":   # the byte engine's general path (algorithm="wavefront"), fewer queries: the slices are 2^26 / 1200 wide
        pool, items = ordered_candidates("heavy_ties", 60_000)
        queries, index = pooled_queries(sw, pool, 1200)
        candidates = sw.Strs(items)
        d_pool = oracle_matrix(sw, orc, sw.Strs(pool), candidates)
        general = sw.LevenshteinDistances(capabilities=scope, algorithm="wavefront")
        _search_and_check(scope, general, queries, candidates, d_pool, index, "wavefront heavy ties", fused=False, ks=(5, 64), bounds=(None, 1))


@pytest.mark.gpu
def test_topk_small_candidate_tapes(sw, orc, scope):
    """Candidate tapes of 0 .. 40 bytes in 1 .. 5 strings: under 16 bytes the fused kernel reads its text with clamped 4-byte loads,
    under 4 bytes byte by byte; the first and last strings touch the tape's ends."""
    rng = np.random.default_rng(41)
    engine = sw.LevenshteinDistances(capabilities=scope)
    words = [b"", b"a", b"ab", b"abc", b"bcad", b"dcbaabcd", b"abcdabcdabcdabcd", b"d" * 32]
    queries = sw.Strs(words)
    pq = sw.PreparedTape(scope, queries)
    for total in range(41):
        for count in range(1, 6):
            cuts = np.sort(rng.integers(0, total + 1, count - 1))
            lengths = np.diff(np.concatenate([[0], cuts, [total]])).astype(int)
            items = [bytes(rng.integers(97, 101, n).astype(np.uint8)) for n in lengths]
            candidates = sw.Strs(items)
            d = oracle_matrix(sw, orc, queries, candidates)
            for k, bound in ((1, None), (3, 2), (64, None)):
                want = expected_topk(d, k, bound)
                check_rows(engine.topk(queries, candidates, scope, k=k, bound=bound), want, f"raw {items} k={k}")
                check_rows(engine.topk(pq, sw.PreparedTape(scope, candidates), scope, k=k, bound=bound), want, f"prepared {items} k={k}")


@pytest.mark.gpu
def test_topk_empty_strings_and_high_bytes(sw, orc, scope):
    engine = sw.LevenshteinDistances(capabilities=scope)
    words, _ = sw.generate_pairs("short_words", 300, seed=43)
    empties = sw.Strs([b""] * 130)
    for queries, candidates, what in ((words, empties, "all-empty candidates"), (empties, words, "all-empty queries"), (empties, empties, "all empty")):
        d = np.tile(candidates.lengths, (len(queries), 1)) if what != "all-empty candidates" else np.tile(queries.lengths[:, None], (1, len(candidates)))
        assert (d == oracle_matrix(sw, orc, queries, candidates)).all()
        for k, bound in ((1, None), (5, 3), (64, None), (64, 0)):
            want = expected_topk(d, k, bound)
            check_rows(engine.topk(queries, candidates, scope, k=k, bound=bound), want, f"{what} k={k} bound={bound}")
            check_rows(engine.topk(sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates), scope, k=k, bound=bound), want,
                       f"prepared {what} k={k} bound={bound}")
    # bytes >= 0x80 and the full byte range in word-sized strings: the fused kernel's high-nibble tables
    rng = np.random.default_rng(44)
    scope.set_profiling(True)
    try:
        for lo, hi in ((0x80, 0x100), (0xF0, 0x100), (0, 0x100)):
            # (mostly six symbols of the range, so that near candidates exist; the rest anywhere in it)
            symbols = rng.integers(lo, hi, 6).astype(np.uint8)
            make = lambda n: [bytes(np.where(rng.random(m) < 0.7, rng.choice(symbols, m), rng.integers(lo, hi, m)).astype(np.uint8))
                              for m in rng.integers(0, 33, n)]
            queries, candidates = sw.Strs(make(200)), sw.Strs(make(3000))
            d = oracle_matrix(sw, orc, queries, candidates)
            pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
            for k, bound in ((1, None), (5, 3), (64, None), (17, 12)):
                check_rows(engine.topk(pq, pc, scope, k=k, bound=bound), expected_topk(d, k, bound), f"bytes {lo:#x}..{hi:#x} k={k} bound={bound}")
                assert "cross_topk" in scope.last_timing()["dominant_name"]
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
def test_topk_offset_widths(sw, orc, scope):
    """Prepared tapes with 32-bit offsets run k_cross_topk<uint32_t>. One 32-bit and one 64-bit byte tape are refused, as the dense
    cross-product refuses them: invalid_argument, and the outputs are not touched -- never rows read at the
    wrong width. Tapes prepared as UTF-8 carry 64-bit code-point offsets, so there either mix is searched."""
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = sw.generate_pairs("short_words", 3000, seed=47)
    queries = queries[:500]
    d = oracle_matrix(sw, orc, queries, candidates)
    tapes = {(w, side): sw.PreparedTape(scope, strs.with_offsets(w)) for w in (np.uint32, np.uint64) for side, strs in (("q", queries), ("c", candidates))}
    scope.set_profiling(True)
    try:
        for w in (np.uint32, np.uint64):
            for k, bound in ((1, None), (5, 3), (64, None), (33, 1)):
                check_rows(engine.topk(tapes[(w, "q")], tapes[(w, "c")], scope, k=k, bound=bound), expected_topk(d, k, bound), f"{w.__name__} k={k} bound={bound}")
                assert "cross_topk" in scope.last_timing()["dominant_name"], (w, scope.last_timing())
            # sub-views that do not start at the tape's first string
            check_rows(engine.topk(tapes[(w, "q")][100:400], tapes[(w, "c")][69:2000], scope, k=7, bound=4), expected_topk(d[100:400, 69:2000], 7, 4), "sub-views")
        for wq, wc in ((np.uint32, np.uint64), (np.uint64, np.uint32)):
            out = np.full((500, 5), 77, np.uint32), np.full((500, 5), 77, np.uint32)
            with pytest.raises(sw.StringWarsError) as info:
                engine.topk(tapes[(wq, "q")], tapes[(wc, "c")], scope, k=5, out=out)
            assert info.value.status == "invalid_argument" and (out[0] == 77).all() and (out[1] == 77).all()
        # code points: the same mix of byte-offset widths is searched (non-ASCII words: the general path)
        words = _code_point_words(700, seed=48)
        uq, uc = sw.Strs(words[:100]), sw.Strs(words[100:])
        d8 = oracle_matrix(sw, orc, uq, uc, utf8=True)
        engine8 = sw.LevenshteinDistancesUTF8(capabilities=scope)
        for wq, wc in itertools.product((np.uint32, np.uint64), repeat=2):
            got = engine8.topk(sw.PreparedTape(scope, uq.with_offsets(wq), utf8=True), sw.PreparedTape(scope, uc.with_offsets(wc), utf8=True), scope, k=9, bound=3)
            check_rows(got, expected_topk(d8, 9, 3), f"code points {wq.__name__} x {wc.__name__}")
            assert scope.last_timing()["dominant_name"].startswith("topk_select/")
        # the self-search on a 32-bit tape
        d_self = oracle_matrix(sw, orc, queries, queries)
        check_rows(engine.topk(tapes[(np.uint32, "q")], None, scope, k=4), expected_topk(d_self, 4), "self, 32-bit offsets")
    finally:
        scope.set_profiling(False)


@pytest.mark.gpu
def test_topk_refuses_device_tensors_of_the_wrong_size(sw, scope):
    """3 queries, 4 candidates, k = 2: six entries. A device tensor of 5 or 7 int32, of 6 int64, or a ``[::2]`` view of 12 int32, as the
    indices or as the distances, is a ValueError before the library -- which cannot know a tensor's size -- sees its address: both
    tensors keep their sentinel. A right pair then gives the rows of the numpy call."""
    import torch
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = sw.Strs(["kitten", "lawn", ""]), sw.Strs(["sitting", "flaw", "law", "kitchen"])
    want = engine.topk(queries, candidates, scope, k=2)
    assert want[1].tolist() == [[2, 3], [1, 2], [3, 4]] and want[0].tolist() == [[3, 0], [2, 1], [2, 1]]
    wrong = {"five": lambda: torch.full((5,), -7, dtype=torch.int32, device="cuda"), "seven": lambda: torch.full((7,), -7, dtype=torch.int32, device="cuda"),
             "int64": lambda: torch.full((6,), -7, dtype=torch.int64, device="cuda"),
             "strided": lambda: torch.full((12,), -7, dtype=torch.int32, device="cuda")[::2]}
    for name, make in wrong.items():
        for slot in (0, 1):
            out = [torch.full((3, 2), -7, dtype=torch.int32, device="cuda"), torch.full((3, 2), -7, dtype=torch.int32, device="cuda")]
            out[slot] = make()
            with pytest.raises(ValueError):
                engine.topk(queries, candidates, scope, k=2, out=tuple(out))
            torch.cuda.synchronize()
            assert all(bool((t == -7).all()) for t in out), (name, slot)
    out = torch.full((6,), -7, dtype=torch.int32, device="cuda"), torch.full((3, 2), -7, dtype=torch.int32, device="cuda")
    got = engine.topk(queries, candidates, scope, k=2, out=out)
    assert got[0] is out[0] and (_host(out[0]).reshape(3, 2) == want[0]).all() and (_host(out[1]) == want[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("width", [np.uint32, np.uint64])
def test_topk_prepared_tape_changed_after_it_was_measured(sw, orc, scope, width):
    """A prepared DEVICE tape is measured once and its memory stays the caller's. When a candidate has grown beyond 32 bytes since, the
    fused kernel reports it and the search is redone on the general path: the rows are those of the tapes as they are now."""
    import ctypes as C
    from stringwars_amd import _native as N
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = sw.generate_pairs("short_words", 2000, seed=53)
    queries, candidates = queries[:300].with_offsets(width), candidates.with_offsets(width)
    device = candidates.to_device(scope)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, device)
    d = oracle_matrix(sw, orc, queries, candidates)
    scope.set_profiling(True)
    try:
        check_rows(engine.topk(pq, pc, scope, k=8, bound=5), expected_topk(d, 8, 5), "before the change")
        assert "cross_topk" in scope.last_timing()["dominant_name"]
        changed = candidates.offsets.copy()
        at = 700
        while int(changed[at + 12]) - int(changed[at]) <= 32:
            at += 1
        changed[at + 1:at + 12] = changed[at + 12]   # candidate `at` now spans twelve words (more than 32 bytes), the eleven behind it are empty
        N.check(N.lib.swh_copy_to_device(scope.handle, C.c_void_p(device.offsets_ptr), changed.ctypes.data, changed.nbytes, None), C.c_char_p())
        now = sw.Strs(data=candidates.data, offsets=changed)
        assert now.lengths.max() > 32 and len(now) == len(candidates)
        d = oracle_matrix(sw, orc, queries, now)
        for k, bound in ((1, None), (8, 5), (64, None)):
            check_rows(engine.topk(pq, pc, scope, k=k, bound=bound), expected_topk(d, k, bound), f"after the change k={k} bound={bound}")
            assert scope.last_timing()["dominant_name"].startswith("topk_select/"), scope.last_timing()
    finally:
        scope.set_profiling(False)
    scope.synchronize()   # nothing is left behind for a later synchronisation
