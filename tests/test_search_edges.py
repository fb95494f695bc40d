"""The two score searches (engine.extract, engine.extract_within) where the dense calls are already tested and the searches were not:
tapes of 0..80 bytes, slices that end on the tape's last byte, column counts around the select kernel's trips, strings of up to 2048
(and 3000) symbols.

Both searches hand the OSA, LCS and Jaro kernels one candidate slice at a time (two_tape.hip, ExtractSweep::walk): a view of the two
tapes cut by scored_view, measured on its own, and `scored_wide(t, got)` -- both byte totals of the VIEW at 16 or more: 128-bit loads;
a total under 4: byte by byte; else dwords; code-point tapes under four symbols on a path of their own -- is decided again for every
slice. The lengths m and n of the score come from the WHOLE tapes at row_first + r and col_first + c.

  1. the size sweep of test_tape_edges.py (queries = case.a, candidates = case.b) through both searches, every scorer;
  2. one batch of 8 x 23 whose slices, with the slice lowered by the test library's hook, fall in all three reader classes within one
     call, the last slice one candidate of 2 bytes that ends where the tape ends -- alone, and as sub-views of larger prepared tapes
     whose neighbours continue the strings;
  3. 1 .. 513 candidates: k_extract_select takes 4 chunks of 64 columns per trip;
  4. queries of 1 .. 2048 symbols against candidates of 1 .. 3000: items of 2 .. 64 blocks as a cross-product, the searches' own
     refusal rule (ExtractSweep::lengths).

The counts come from test_tape_edges.expected (the references of test_osa.py, test_lcs.py and test_jaro.py, each pair computed once),
the scores from test_extract.reference_scores, the rows from test_extract.expected_rows and test_extract_within.expected_within. Every
comparison is exact: indices as uint32, scores as their 64-bit patterns, CSR offsets as integers. The CPU tests run the generators and
the references alone and assert what the batches are meant to reach, and count the calls the GPU tests issue."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import TEST_LIBRARY_ENV, run_in_child
from test_extract import HOOK, LARGER_IS_BETTER, PAD_INDEX, SCORERS, assert_rows, expected_rows, raw_extract, reference_scores
from test_extract_within import SENTINEL32, SENTINEL64, assert_csr, batch_cutoffs, expected_within, raw_within
from test_osa import mutated
from test_tape_edges import (LETTERS, LONG_LENGTHS, OTHERS, SIZES, SYMBOL_OTHERS, SYMBOL_TOTALS, TO_CODE_POINTS, cross_sweep, expanded, expected,
                             letters, remember, symbol_cross_sweep)

gpu = pytest.mark.gpu

# a cutoff that admits every candidate: 0 for a similarity; for a distance the largest finite one (the range search refuses +inf as
# "the dense cross-product": test_extract_within.test_edges_and_refusals)
EVERYTHING = {True: 0.0, False: sys.float_info.max}


# ---- the references -------------------------------------------------------------------------------------------------------------------
def counts_of(queries, candidates, utf8):
    """test_extract.reference_counts' tuple -- osa, lcs, M, t, prefix as (queries, candidates) arrays, m, n -- from
    test_tape_edges.expected on the expanded pairs. The items are bytes, or str on a code-point tape: len() counts symbols."""
    x, y = expanded(queries, candidates)
    shape = (len(queries), len(candidates))
    osa = expected("osa", x, y, utf8)[:, 0].reshape(shape)
    lcs = expected("lcs", x, y, utf8)[:, 0].reshape(shape)
    jaro = expected("jaro", x, y, utf8).reshape(shape + (3,))
    m, n = (np.array([len(s) for s in side], dtype=np.int64) for side in (queries, candidates))
    return osa, lcs, jaro[..., 0], jaro[..., 1], jaro[..., 2], m, n


def extract_rows(engine, scope, q, c, **kw):
    indices, scores = engine.extract(q, c, scope, **kw)
    return indices, scores.view(np.uint64)


def within_csr(engine, scope, q, c, **kw):
    found = engine.extract_within(q, c, scope, **kw)
    return np.asarray(found.offsets), found.indices, found.scores.view(np.uint64)


def hooked(value):
    """Sets (or, with None, removes) the slice hook that the test library reads at every call."""
    os.environ.pop(HOOK, None)
    if value is not None:
        os.environ[HOOK] = str(value)


# ---- 1. the tape-size sweep -------------------------------------------------------------------------------------------------------------
SWEEP_KINDS = ("bytes", "utf8", "symbols", "encoded")


@functools.lru_cache(maxsize=None)
def sweep_cases(kind):
    """(cases, utf8): test_tape_edges' cross sweeps with a as the queries and b as the candidates. `encoded`: every third case of the
    multi-byte sweep as its UTF-8 bytes, for the byte engine."""
    if kind == "bytes":
        return cross_sweep(False), False
    if kind == "utf8":
        return cross_sweep(True), True
    if kind == "symbols":
        return symbol_cross_sweep(), True
    return [c._replace(a=[s.encode() for s in c.a], b=[s.encode() for s in c.b]) for c in cross_sweep(True)[::3]], False


@functools.lru_cache(maxsize=None)
def sweep_counts(kind):
    """Per case (counts of a x b, counts of a x a or None off the diagonal); the references of the whole sweep in one batch."""
    cases, utf8 = sweep_cases(kind)
    for call in ("osa", "lcs", "jaro"):
        remember(call, cases, utf8, cross=True)
    return [(counts_of(c.a, c.b, utf8), counts_of(c.a, c.a, utf8) if c.total_a == c.total_b else None) for c in cases]


def sweep_calls(case, scores, own_scores, larger):
    """What the GPU test calls on one case: (search, form, self-search, k or cutoff). extract with k = 1 and one more than there are
    candidates (the last place is padding) on Strs and on prepared tapes; extract_within at the median of the case's scores and at a
    cutoff that admits everything; on the diagonal the self-search (candidates None) the same way."""
    for own, reference, count in ((False, scores, len(case.b)),) + (((True, own_scores, len(case.a)),) if own_scores is not None else ()):
        for form in ("strs", "prepared"):
            for k in (1, count + 1):
                yield "extract", form, own, k
        yield "within", "strs", own, batch_cutoffs(reference, larger)[0]
        yield "within", "prepared", own, EVERYTHING[larger]


def test_the_sweep_compares_every_case():
    """The generators and the references alone: every (total, other) combination of the size lists is there twice, empty first and
    last strings on either side, every case is called 6 times per scorer (12 on the diagonal), the padding place is padding, and
    the median cutoff admits some candidates and rejects others in more than a third of its calls."""
    issued = 0
    for kind in SWEEP_KINDS:
        cases, utf8 = sweep_cases(kind)
        sizes, others = (SYMBOL_TOTALS, SYMBOL_OTHERS) if kind == "symbols" else (SIZES, OTHERS)
        totals = [(c.total_a, c.total_b) for c in cases]
        if kind != "encoded":
            wanted = {(s, s) for s in sizes} | {(s, o) for s in sizes for o in others} | {(o, s) for s in sizes for o in others}
            assert set(totals) == wanted and len(totals) == 2 * len(wanted), kind
            assert {0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 80} <= set(sizes) or kind == "symbols"
        assert {c.empty_side for c in cases} == {None, "a", "b"}, kind
        assert all(len(c.a) >= 1 and len(c.b) >= 1 for c in cases)
        diagonal = sum(c.total_a == c.total_b for c in cases)
        assert diagonal == 2 * len(sizes) or (kind == "encoded" and diagonal >= len(sizes) // 2)
        split = planned = 0
        for scorer in SCORERS:
            larger = LARGER_IS_BETTER[scorer]
            for case, (counts, own) in zip(cases, sweep_counts(kind)):
                scores = reference_scores(scorer, counts)
                own_scores = None if own is None else reference_scores(scorer, own)
                calls = list(sweep_calls(case, scores, own_scores, larger))
                assert len(calls) == (12 if case.total_a == case.total_b else 6)
                planned += len(calls)
                for search, form, is_own, arg in calls:
                    reference = own_scores if is_own else scores
                    if search == "extract" and arg > 1:
                        indices, bits = expected_rows(reference, larger, arg)
                        assert (indices[:, -1] == PAD_INDEX).all() and (indices[:, :-1] != PAD_INDEX).all()
                    if search == "within" and arg == EVERYTHING[larger]:
                        assert int(expected_within(reference, larger, arg)[0][-1]) == reference.size
                    elif search == "within":
                        split += 0 < int(expected_within(reference, larger, arg)[0][-1]) < reference.size
        assert planned == 6 * (6 * len(cases) + 6 * diagonal), kind
        # (of 6 scorers x the cases and the diagonal's self-searches; tapes of a few symbols have one score, or one string, only)
        assert 3 * split > 6 * (len(cases) + diagonal), (kind, split, len(cases))
        issued += planned
    assert issued == sum(sweep_census(kind) for kind in SWEEP_KINDS) * len(SCORERS)


def sweep_census(kind):
    """The calls of one (kind, scorer) of the GPU test."""
    cases, _ = sweep_cases(kind)
    return 6 * len(cases) + 6 * sum(c.total_a == c.total_b for c in cases)


@pytest.fixture(scope="module")
def lev(sw, scope):
    return sw.LevenshteinDistances(capabilities=scope)


@pytest.fixture(scope="module")
def lev8(sw, scope):
    return sw.LevenshteinDistancesUTF8(capabilities=scope)


@gpu
@pytest.mark.parametrize("kind", SWEEP_KINDS)
@pytest.mark.parametrize("scorer", SCORERS)
def test_tape_size_sweep(sw, scope, lev, lev8, scorer, kind):
    """Query tapes of 0 .. 40, 47 .. 49, 63 .. 65 and 80 bytes against candidate tapes of the same size and of 3, 15, 16 and 80, in
    both orders (four-byte symbols: 0 .. 8 against 1, 3, 4 and 8): the reader of the scoring kernel follows the two totals, the first
    string starts on the tape's first byte and the last ends on its last."""
    cases, utf8 = sweep_cases(kind)
    engine, larger = lev8 if utf8 else lev, LARGER_IS_BETTER[scorer]
    issued = 0
    for case, (counts, own) in zip(cases, sweep_counts(kind)):
        scores = reference_scores(scorer, counts)
        own_scores = None if own is None else reference_scores(scorer, own)
        strs = sw.Strs(case.a), sw.Strs(case.b)
        sides = {"strs": strs, "prepared": tuple(sw.PreparedTape(scope, s, utf8=utf8) for s in strs)}
        for search, form, is_own, arg in sweep_calls(case, scores, own_scores, larger):
            q, c = sides[form][0], None if is_own else sides[form][1]
            reference = own_scores if is_own else scores
            what = (scorer, kind, search, form, "self" if is_own else "cross", arg, case.total_a, case.total_b, case.trial, case.a, case.b)
            if search == "extract":
                assert_rows(extract_rows(engine, scope, q, c, scorer=scorer, k=arg), expected_rows(reference, larger, arg), what)
            else:
                assert_csr(within_csr(engine, scope, q, c, scorer=scorer, cutoff=arg), expected_within(reference, larger, arg), what)
            issued += 1
        for tape in sides["prepared"]:
            tape.free()
    assert issued == sweep_census(kind)


# ---- 2. slice seams at the tape's end ---------------------------------------------------------------------------------------------------
# The slice hook in pairs. ExtractSweep's constructor: q_step = min(nq, max(1, min(4096, chunk >> 6))), c_step = max(1, min(nc,
# chunk / q_step)). With 8 queries and 23 candidates, 8, 11, 16, 22 and 64 pairs give blocks of one query and slices of 8, 11, 16, 22
# and 23 (all) candidates -- 11 and 22 leave the last candidate a slice of its own -- and 192 pairs blocks of 3, 3 and 2 queries.
SEAM_HOOKS = (8, 11, 16, 22, 64, 192)
SEAM_QUERY_LENGTHS = (0, 1, 3, 4, 9, 15, 16, 20)
SEAM_CANDIDATE_LENGTHS = (5, 0, 7, 3, 9, 2, 6, 4) + (0,) * 8 + (2, 0, 3, 1, 0, 4, 2)
SEAM_QUERY_VIEW, SEAM_CANDIDATE_VIEW = (3, 11), (5, 28)
kScoredChunkPairs = 1 << 21


def sweep_steps(nq, nc, hook):
    """(q_step, c_step) as ExtractSweep's constructor computes them; `hook` None: the shipped slice."""
    chunk = max(1, min(kScoredChunkPairs if hook is None else hook, kScoredChunkPairs))
    q_step = min(nq, max(1, min(4096, chunk >> 6)))
    return q_step, max(1, min(nc, chunk // q_step))


def slice_views(query_bytes, candidate_bytes, hook):
    """(rows, columns, the view's query bytes, its candidate bytes) of every slice of the walk, in its order."""
    nq, nc = len(query_bytes), len(candidate_bytes)
    q_step, c_step = sweep_steps(nq, nc, hook)
    return [(min(q_step, nq - q0), min(c_step, nc - c0), sum(query_bytes[q0:q0 + q_step]), sum(candidate_bytes[c0:c0 + c_step]))
            for q0 in range(0, nq, q_step) for c0 in range(0, nc, c_step)]


def seam_cutoff(scores, larger_is_better):
    """The score at the best quarter of the batch (half of its candidates are empty: the median is the score against those)."""
    ranked = np.sort(np.asarray(scores).ravel())
    return float((ranked[::-1] if larger_is_better else ranked)[ranked.size // 4])


def total_class(total):
    return "under 4" if total < 4 else "4..15" if total < 16 else "16 and over"


@functools.lru_cache(maxsize=None)
def seam_tapes():
    """(query tape, candidate tape): consecutive pieces of one text over `abc` and of a copy with one edit in ten symbols, so what
    follows a string in its tape continues it. The views SEAM_QUERY_VIEW and SEAM_CANDIDATE_VIEW hold the batch: strings of
    SEAM_QUERY_LENGTHS and SEAM_CANDIDATE_LENGTHS bytes."""
    rng = np.random.default_rng(9040)
    text = letters(rng, 200)
    other = "".join(mutated(rng, text, 20, lambda: LETTERS[int(rng.integers(0, 3))]))

    def pieces(source, start, lengths):
        ends = start + np.cumsum((0,) + lengths)
        return [source[s:e] for s, e in zip(ends, ends[1:])]

    return pieces(text, 0, (6, 2, 5) + SEAM_QUERY_LENGTHS + (7, 3, 4)), pieces(other, 3, (4, 9, 1, 6, 3) + SEAM_CANDIDATE_LENGTHS + (8, 2, 5, 7))


def seam_batch():
    qt, ct = seam_tapes()
    return [s.encode() for s in qt[slice(*SEAM_QUERY_VIEW)]], [s.encode() for s in ct[slice(*SEAM_CANDIDATE_VIEW)]]


@functools.lru_cache(maxsize=None)
def seam_counts():
    return counts_of(*seam_batch(), False)


def test_the_seam_batch_reaches_every_reader_class():
    """ExtractSweep's blocks x slices arithmetic on the batch: within ONE call (the hook at 11 pairs) the candidate slices' byte totals
    fall under 4, in 4..15 and at 16 or over, against query blocks of all three classes, so `wide` is true for some slices and false
    for others; the last slice is one candidate of 2 bytes, the tape's last; one slice (hook 8) holds empty candidates only; a hook
    gives query blocks of more than one row and a ragged last block; and reading 3 bytes past every string's end into its neighbour
    would change rows of every scorer."""
    queries, candidates = seam_batch()
    qb, cb = [len(s) for s in queries], [len(s) for s in candidates]
    assert tuple(qb) == SEAM_QUERY_LENGTHS and tuple(cb) == SEAM_CANDIDATE_LENGTHS and (len(qb), len(cb)) == (8, 23)
    assert [sweep_steps(8, 23, hook) for hook in SEAM_HOOKS] == [(1, 8), (1, 11), (1, 16), (1, 22), (1, 23), (3, 23)]
    assert sweep_steps(8, 23, None) == (8, 23) and sweep_steps(70, 300, 4096) == (64, 64) and sweep_steps(70, 300, 640) == (10, 64)
    views = {hook: slice_views(qb, cb, hook) for hook in SEAM_HOOKS}
    classes = {hook: {(total_class(a), total_class(b)) for _, _, a, b in views[hook]} for hook in SEAM_HOOKS}
    every = {"under 4", "4..15", "16 and over"}
    assert classes[11] == {(a, b) for a in every for b in every}                      # all nine in one call: wide only for one of them
    assert {b for _, b in classes[8]} == every and {b for _, b in classes[22]} == {"under 4", "16 and over"}
    for hook in (11, 22):                                                             # the last slice: one candidate of 1..3 bytes
        assert all(columns == 1 and 1 <= total <= 3 for _, columns, _, total in views[hook][len(views[hook]) // 8 - 1::len(views[hook]) // 8])
    assert cb[-1] == 2 and cb[8:16] == [0] * 8 and views[8][1][1:] == (8, 0, 0)       # a slice of empty candidates only
    assert [rows for rows, _, _, _ in views[192]] == [3, 3, 2] and len(views[8]) == 8 * 3
    qt, ct = seam_tapes()
    (q0, q1), (c0, c1) = SEAM_QUERY_VIEW, SEAM_CANDIDATE_VIEW
    past_q = [(qt[k] + "".join(qt[k + 1:]))[:len(qt[k]) + 3].encode() for k in range(q0, q1)]
    past_c = [(ct[k] + "".join(ct[k + 1:]))[:len(ct[k]) + 3].encode() for k in range(c0, c1)]
    for scorer in SCORERS:
        true = reference_scores(scorer, seam_counts())
        for wrong in (counts_of(past_q, candidates, False), counts_of(queries, past_c, False)):
            assert (expected_rows(reference_scores(scorer, wrong), LARGER_IS_BETTER[scorer], 5)[1] != expected_rows(true, LARGER_IS_BETTER[scorer], 5)[1]).any()
        cutoff = seam_cutoff(true, LARGER_IS_BETTER[scorer])
        assert 1 < int(expected_within(true, LARGER_IS_BETTER[scorer], cutoff)[0][-1]) < true.size


def fill_within(engine, scope, q, c, rows, total, room, **kw):
    """extract_within into host arrays of `room` entries, sentinel-filled: with room for the total the hits and nothing after them;
    one short, the offsets alone -- the arrays stay as they were and the call says so."""
    offsets = np.full(rows + 1, SENTINEL64, dtype=np.uint64)
    indices, values = np.full(room + 4, SENTINEL32, dtype=np.uint32), np.full(room + 4, SENTINEL64, dtype=np.uint64)
    out = (offsets, indices[:room], values[:room].view(np.float64))
    if room >= total:
        engine.extract_within(q, c, scope, out=out, **kw)
        assert (indices[total:] == SENTINEL32).all() and (values[total:] == SENTINEL64).all(), "written at or beyond the total"
    else:
        with pytest.raises(ValueError):
            engine.extract_within(q, c, scope, out=out, **kw)
        assert (indices == SENTINEL32).all() and (values == SENTINEL64).all(), "written without room for the total"
    return offsets, indices[:min(room, total)], values[:min(room, total)]


@gpu
def test_slice_seams_at_the_tapes_end(request, sw, scope):
    """The batch above with the slice lowered to 8, 11, 16, 22, 64 and 192 pairs (the test library's hook): sliced rows equal whole
    rows equal the reference, for every scorer, extract (k = 1, 5) and extract_within with room for exactly the total and for one
    less. Once as raw host tapes -- the last candidate ends where the tape ends -- and once as the views [3:11] and [5:28] of prepared
    tapes whose neighbours continue the strings."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV), test_library=True):
        return
    assert sw.LIBRARY_PATH.endswith("libstringwars_amd_test.so")
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries, candidates = seam_batch()
    qt, ct = seam_tapes()
    pq, pc = (sw.PreparedTape(scope, sw.Strs([s.encode() for s in side])) for side in (qt, ct))
    forms = {"raw": (sw.Strs(queries), sw.Strs(candidates)), "views": (pq[slice(*SEAM_QUERY_VIEW)], pc[slice(*SEAM_CANDIDATE_VIEW)])}
    try:
        for scorer in SCORERS:
            larger = LARGER_IS_BETTER[scorer]
            scores = reference_scores(scorer, seam_counts())
            cutoff = seam_cutoff(scores, larger)
            want_within = expected_within(scores, larger, cutoff)
            total = int(want_within[0][-1])
            for form, (q, c) in forms.items():
                whole = {}
                for hook in (None,) + SEAM_HOOKS:
                    hooked(hook)
                    what = (scorer, form, hook)
                    for k in (1, 5):
                        got = extract_rows(engine, scope, q, c, scorer=scorer, k=k)
                        assert_rows(got, whole.setdefault(k, got), (what, k, "sliced against whole"))
                        assert_rows(got, expected_rows(scores, larger, k), (what, k, "against the reference"))
                    got = fill_within(engine, scope, q, c, len(queries), total, total, scorer=scorer, cutoff=cutoff)
                    assert_csr(got, whole.setdefault("within", got), (what, "sliced against whole"))
                    assert_csr(got, want_within, (what, "against the reference"))
                    short = fill_within(engine, scope, q, c, len(queries), total, total - 1, scorer=scorer, cutoff=cutoff)
                    assert np.array_equal(short[0], want_within[0]), (what, "one short: the offsets")
    finally:
        hooked(None)


# ---- 3. column counts around the select kernel's trips ------------------------------------------------------------------------------------
SELECT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
SELECT_RUN = range(250, 262)   # columns of one repeated word: equal scores on both sides of column 255 / 256


@functools.lru_cache(maxsize=None)
def select_batch(count):
    """3 queries of 7, 5 and 9 symbols against `count` words of 3 .. 6 (the same words for every count). The first query stands at
    column count - 1, one substitution away from it at column 0 and two away in SELECT_RUN; no other word shares more than two
    letters with it."""
    rng = np.random.default_rng(9050)
    queries = ["abcdefg", letters(rng, 5, "abuvw"), letters(rng, 9, "abuvw")]
    words = [letters(rng, rng.integers(3, 7), "abuvwxyz") for _ in range(max(SELECT_COUNTS))][:count]
    for at in SELECT_RUN:
        if at < count:
            words[at] = "abcdeyz"
    words[0] = "abcdefz"
    words[count - 1] = "abcdefg"
    return [q.encode() for q in queries], [w.encode() for w in words]


@functools.lru_cache(maxsize=None)
def select_counts(count):
    return counts_of(*select_batch(count), False)


def test_the_select_batch_plants_what_it_says():
    for count in SELECT_COUNTS:
        for scorer in SCORERS:
            indices, bits = expected_rows(reference_scores(scorer, select_counts(count)), LARGER_IS_BETTER[scorer], 64)
            head = [count - 1, 0] + [at for at in SELECT_RUN if at < count - 1]
            assert indices[0, :min(len(head), count)].tolist() == list(dict.fromkeys(head))[:count], (count, scorer)
            if count > SELECT_RUN[-1] + 1:
                assert len(set(bits[0, 2:2 + len(SELECT_RUN)].tolist())) == 1 and bits[0, 1] != bits[0, 2] != bits[0, 2 + len(SELECT_RUN)]
            assert (indices[:, min(count, 64):] == PAD_INDEX).all() and (indices[:, :min(count, 64)] != PAD_INDEX).all()


@gpu
@pytest.mark.parametrize("count", SELECT_COUNTS)
def test_column_counts_around_the_select_trips(sw, scope, lev, count):
    """1, 63 .. 65, 255 .. 257 and 511 .. 513 candidates: the last chunk of 64 columns and the last trip of 4 chunks full, one short
    and one over; the best candidate in the last column, the runner-up in the first, a run of equal scores across column 255 / 256.
    extract_within on the same: every row's candidates ascend."""
    queries, candidates = select_batch(count)
    strs = sw.Strs(queries), sw.Strs(candidates)
    prepared = tuple(sw.PreparedTape(scope, s) for s in strs)
    for scorer in SCORERS:
        larger = LARGER_IS_BETTER[scorer]
        scores = reference_scores(scorer, select_counts(count))
        for k in (1, 64):
            for form, (q, c) in (("strs", strs), ("prepared", prepared)):
                assert_rows(extract_rows(lev, scope, q, c, scorer=scorer, k=k), expected_rows(scores, larger, k), (scorer, count, k, form))
        for cutoff in (batch_cutoffs(scores, larger)[0], EVERYTHING[larger]):
            got = within_csr(lev, scope, *prepared, scorer=scorer, cutoff=cutoff)
            assert_csr(got, expected_within(scores, larger, cutoff), (scorer, count, cutoff))
            for row in range(3):
                assert (np.diff(got[1][int(got[0][row]):int(got[0][row + 1])].astype(np.int64)) > 0).all(), (scorer, count, row)


# ---- 4. long strings ------------------------------------------------------------------------------------------------------------------------
LONG_QUERY_LENGTHS = (1, 64, 65, 2047, 2048)
# the candidates' lengths (test_tape_edges.LONG_LENGTHS and 64 again) and the query each is a mutated repetition of; the three
# longest stand last: with the slice lowered to 3 pairs they are a slice of their own (blocks of one query x slices of 3 candidates)
LONG_CANDIDATES = tuple(zip(LONG_LENGTHS[:8] + (64,) + LONG_LENGTHS[8:], (0, 1, 2, 1, 2, 1, 2, 2, 0, 3, 4, 4)))
LONG_HOOK = 3
OVER = 2049


@functools.lru_cache(maxsize=None)
def long_batch():
    """(queries, candidates) as str over `abc`. A candidate is its query repeated to the candidate's length with 1 .. 5 edits, as
    test_tape_edges.lopsided_distance_cases builds them: no answer is a length difference."""
    rng = np.random.default_rng(9060)
    draw = lambda: LETTERS[int(rng.integers(0, 3))]
    queries = [letters(rng, n) for n in LONG_QUERY_LENGTHS]
    candidates = []
    for length, of in LONG_CANDIDATES:
        base = (queries[of] * (length // len(queries[of]) + 1))[:length]
        candidates.append(("".join(mutated(rng, base, int(rng.integers(1, 6)), draw)) + letters(rng, length))[:length])
    assert [len(c) for c in candidates] == [n for n, _ in LONG_CANDIDATES] and sorted(set(len(c) for c in candidates)) == sorted(LONG_LENGTHS)
    return queries, candidates


@functools.lru_cache(maxsize=None)
def long_counts(with_3000):
    queries, candidates = long_batch()
    return counts_of([q.encode() for q in queries], [c.encode() for c in candidates[:None if with_3000 else -1]], False)


def long_scores(scorer):
    """The reference scores of the long batch: the Jaro scorers without the 3000-symbol candidate (either string over 2048 is refused)."""
    return reference_scores(scorer, long_counts(not scorer.startswith("jaro")))


def test_the_long_batch_reaches_what_it_is_for():
    """For every scorer the best candidate of at least two rows holds more than 64 symbols (an item of several blocks decides the
    row), and the 3000-symbol candidate is ranked strictly inside some row of the four scorers that take it. The slices of the lowered
    hook: the three longest candidates alone. The transliteration to code points keeps every symbol apart."""
    assert LONG_CANDIDATES[-1][0] == 3000 and [n for n, _ in LONG_CANDIDATES[-3:]] == [2047, 2048, 3000]
    assert sweep_steps(5, 12, LONG_HOOK) == (1, 3) and sweep_steps(5, 11, LONG_HOOK) == (1, 3)
    lengths = np.array([n for n, _ in LONG_CANDIDATES])
    for scorer in SCORERS:
        scores = long_scores(scorer)
        indices, _ = expected_rows(scores, LARGER_IS_BETTER[scorer], scores.shape[1])
        assert (lengths[indices[:, 0]] > 64).sum() >= 2, (scorer, indices[:, 0])
        if not scorer.startswith("jaro"):
            places = [int(np.nonzero(row == 11)[0][0]) for row in indices]
            assert any(0 < place < 11 for place in places), (scorer, places)
    assert len({"abc".translate(TO_CODE_POINTS)[k] for k in range(3)}) == 3 and len("abc".translate(TO_CODE_POINTS).encode()) == 7


def refused_untouched(sw, scope, engine, queries, candidates, scorer_id, cutoff, utf8, words):
    """Both searches refuse the call with unsupported_length, name the pair and its lengths, and leave sentinel-filled outputs alone."""
    indices, values = np.full((len(queries), 4), SENTINEL32, dtype=np.uint32), np.full((len(queries), 4), SENTINEL64, dtype=np.uint64)
    status, message = raw_extract(sw, engine, scope, queries, candidates, scorer_id, 4, EVERYTHING[True] if scorer_id >= 2 else float("inf"), 0.1,
                                  indices, values, utf8)
    assert status == "unsupported_length" and all(word in message for word in words), (status, message)
    assert (indices == SENTINEL32).all() and (values == SENTINEL64).all(), message
    offsets = np.full(len(queries) + 1, SENTINEL64, dtype=np.uint64)
    status, message = raw_within(sw, engine, scope, queries, candidates, scorer_id, cutoff, 0.1, offsets, indices.ravel(), values.ravel(), indices.size, utf8)
    assert status == "unsupported_length" and all(word in message for word in words), (status, message)
    assert (offsets == SENTINEL64).all() and (indices == SENTINEL32).all() and (values == SENTINEL64).all(), message


@gpu
@pytest.mark.parametrize("utf8", [False, True], ids=["bytes", "utf8"])
def test_long_strings(request, sw, scope, utf8):
    """5 queries of 1 .. 2048 symbols x 12 candidates of 1 .. 3000: OSA, Indel, LCS and ratio with the 3000-symbol candidate (no query
    is over 2048: the shorter side of every pair is within the limit), Jaro and Jaro-Winkler without it -- and refused with it, as
    OSA is once a query of 2049 symbols stands next to it; a refusal writes nothing and the engine goes on working. In one slice, and
    with the three longest candidates in slices of their own (the test library's hook). The code-point engine runs the batch
    transliterated symbol for symbol, which leaves every count as it is."""
    if not run_in_child(request, env=dict(TEST_LIBRARY_ENV), test_library=True):
        return
    engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
    items = lambda strs: [s.translate(TO_CODE_POINTS) for s in strs] if utf8 else [s.encode() for s in strs]
    queries, candidates = (items(side) for side in long_batch())
    try:
        for scorer_id, scorer in enumerate(SCORERS):
            larger, jaro = LARGER_IS_BETTER[scorer], scorer.startswith("jaro")
            scores = long_scores(scorer)
            taken = candidates[:-1] if jaro else candidates
            strs = sw.Strs(queries), sw.Strs(taken)
            prepared = tuple(sw.PreparedTape(scope, s, utf8=utf8) for s in strs)
            cutoff = batch_cutoffs(scores, larger)[0]
            for hook in (None, LONG_HOOK):
                hooked(hook)
                for form, (q, c) in (("strs", strs), ("prepared", prepared)):
                    for k in (1, 5, 13):
                        assert_rows(extract_rows(engine, scope, q, c, scorer=scorer, k=k), expected_rows(scores, larger, k), (scorer, utf8, hook, form, k))
                    for bar in (cutoff, EVERYTHING[larger]):
                        assert_csr(within_csr(engine, scope, q, c, scorer=scorer, cutoff=bar), expected_within(scores, larger, bar), (scorer, utf8, hook, form, bar))
            hooked(None)
            raw_items = lambda side: [s.encode() if isinstance(s, str) else s for s in side]
            over = items(["c" * OVER])
            if jaro:   # either string over the limit: the first query against the 3000-symbol candidate, and a query of 2049 against the first
                refused_untouched(sw, scope, engine, raw_items(queries), raw_items(candidates), scorer_id, cutoff, utf8, ("(0, 11)", "1 x 3000"))
                refused_untouched(sw, scope, engine, raw_items(queries + over), raw_items(taken), scorer_id, cutoff, utf8, ("(5, 0)", "2049 x 1"))
            else:      # only a query AND a candidate over the limit: the message names the two
                refused_untouched(sw, scope, engine, raw_items(queries + over), raw_items(candidates), scorer_id, cutoff, utf8, ("(5, 11)", "2049 x 3000"))
            assert_rows(extract_rows(engine, scope, *prepared, scorer=scorer, k=2), expected_rows(scores, larger, 2), (scorer, utf8, "after the refusals"))
            for tape in prepared:
                tape.free()
    finally:
        hooked(None)
