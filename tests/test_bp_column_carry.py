"""A column of the bit-parallel item (bp_item.hpp: `column`; bp_dense.hpp carries a copy) takes the horizontal deltas of the block below
it from the neighbouring lane: one DPP move per delta word with the splice folded into it, of which only BIT 31 is defined -- a pair's
first block ORs the boundary's +1 into the word its neighbour sent (the last block of ANOTHER pair) and ANDs the neighbour's -1 away. The
recurrence runs on the raw words of the two nibble tables. What can go wrong is the hand-over between lanes, so the batches aim there:

  * pair boundaries at every lane position: one batch per G = 1 .. 8 (32-row blocks per pattern) with patterns of 32 G, 32 G - 1 and
    32 (G - 1) + 1 symbols -- row 31 of the last block is a live row, the block is nearly empty, it is a single row. G = 1 makes every lane
    a first block; G = 3, 5, 6, 7 leave idle lanes at the wave's end; first blocks fall on lanes 0, 16, 32, 48 and between them. Texts are
    unrelated to their patterns over four letters, so deltas of +1 and of -1 both reach bit 31 of a pair's last block, next to the first
    block of the pair behind it;
  * a call of one pair and a call of 64 / G + 1 pairs per G: an item whose other slots are empty, and an item with one occupied slot behind
    a full one;
  * borrow chains through every block: x + S against S + y (and mirrored, with one to three symbols of offset): the optimal path runs off
    the diagonal and -1 horizontals cross every block boundary in most columns;
  * the bytes 0x00, 0x7F, 0x80, 0xFF; a code-point batch of one to four blocks; a dense-alphabet batch (patterns of 481 code points and
    more: bp_dense.hpp); a small cross-product call on the tiled route.

Which string the kernel takes as the pattern is its own choice (common.hpp: bp_pattern_is_a); the test repeats it and asserts on the CPU
that the batches reach every G of 1 .. 8 with each of the three pattern lengths, in both argument orders.

Every byte case runs in a child process against the TEST library with STRINGWARS_AMD_TILE=256 on each route of ROUTES (as in
test_bp_group_schedule.py) and compares EVERY distance with oracle.levenshtein_pairs(..., algo="hyyro")."""
import numpy as np
import pytest

from conftest import run_in_child

pytestmark = pytest.mark.gpu

TILE = 256
BLOCKS = tuple(range(1, 9))
LETTERS = bytes(range(97, 101))
EDGE_BYTES = bytes((0x00, 0x7F, 0x80, 0xFF))

ROUTES = {
    "side": ({"STRINGWARS_AMD_SIDE": "1", "STRINGWARS_AMD_TILED_WAVES": "16"}, "tiled"),
    "no_side": ({"STRINGWARS_AMD_SIDE": "0", "STRINGWARS_AMD_TILED_WAVES": "16"}, "tiled"),
    "clamped": ({"STRINGWARS_AMD_SIDE": "1", "STRINGWARS_AMD_TILED_WAVES": "16", "STRINGWARS_AMD_INTERIOR": "0"}, "tiled"),
    "waves8": ({"STRINGWARS_AMD_TILED_WAVES": "8"}, "tiled"),
    "waves4": ({"STRINGWARS_AMD_TILED_WAVES": "4"}, "tiled"),
    "planned": ({}, "bitparallel"),
}


def in_child(request, route):
    return run_in_child(request, env=dict(ROUTES[route][0], STRINGWARS_AMD_TILE=str(TILE)), test_library=True, timeout=600)


def blocks(length):
    return (length + 31) >> 5


def pattern_is_a(la, lb):
    """common.hpp: bp_pattern_is_a, for strings of at most 64 blocks."""
    ga, gb = blocks(la), blocks(lb)
    return ga * (lb + ga - 1) <= gb * (la + gb - 1)


def pattern_of(la, lb):
    """(G, m) of a pair as the kernel runs it: the blocks and the length of the string it takes as the pattern."""
    m = la if pattern_is_a(la, lb) else lb
    return blocks(m), m


def pattern_lengths(g):
    """The three pattern lengths of G blocks: the last block full, one row short of full, a single row."""
    return sorted({32 * g, 32 * g - 1, 32 * (g - 1) + 1})


def unlike_pair(rng, la, lb, alphabet):
    """Two strings over `alphabet` whose first symbols differ and whose last symbols differ: no common prefix or suffix to cut."""
    a = bytearray(alphabet[i] for i in rng.integers(0, len(alphabet), la))
    b = bytearray(alphabet[i] for i in rng.integers(0, len(alphabet), lb))
    a[0] = a[-1] = alphabet[0]
    b[0] = b[-1] = alphabet[1]
    return bytes(a), bytes(b)


def text_lengths(m):
    """Text lengths with which a pattern of m symbols stays the pattern in EITHER argument order: not longer than the pattern and of as
    many blocks (the longer string of equally many blocks is the cheaper pattern; of two equal strings either is a pattern of m)."""
    return [n for n in range(m, m - 4, -1) if n >= 1 and blocks(n) == blocks(m)]


def boundary_pairs(rng, g, count, alphabet=LETTERS):
    """`count` pairs of G blocks, the three pattern lengths in turn, texts of the pattern's length or up to three symbols shorter."""
    pairs = []
    lengths = pattern_lengths(g)
    for i in range(count):
        m = lengths[i % len(lengths)]
        texts = text_lengths(m)
        pairs.append(unlike_pair(rng, m, texts[(i // len(lengths)) % len(texts)], alphabet))
    return pairs


def reached(pairs):
    """The (G, m) the kernel runs, over both argument orders of every pair."""
    return {pattern_of(len(a), len(b)) for a, b in pairs} | {pattern_of(len(b), len(a)) for a, b in pairs}


def shuffled(rng, pairs):
    order = rng.permutation(len(pairs))
    return [pairs[i][0] for i in order], [pairs[i][1] for i in order]


def check(sw, orc, scope, route, items_a, items_b):
    """Two prepared tapes with 32-bit offsets, both orders, every distance against the oracle's Hyyro implementation."""
    a, b = sw.Strs(items_a).with_offsets(np.uint32), sw.Strs(items_b).with_offsets(np.uint32)
    want = orc.levenshtein_pairs(a, b, algo="hyyro")
    pa, pb = sw.PreparedTape(scope, a), sw.PreparedTape(scope, b)
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm=ROUTES[route][1])
    got = engine.pairs(pa, pb, scope)
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    got = engine.pairs(pb, pa, scope)
    assert (got == want).all(), ("swapped", np.flatnonzero(got != want)[:8])
    return want


def test_batches_reach_what_they_claim():
    """On the CPU: with the kernel's own choice of the pattern side, the boundary batches, the small calls, the borrow chains and the
    edge-byte batch each run every G of 1 .. 8; the first two with each of the three pattern lengths, in both argument orders."""
    rng = np.random.default_rng(95)
    wanted = {(g, m) for g in BLOCKS for m in pattern_lengths(g)}
    assert len(wanted) == 24
    hit = set()
    for g in BLOCKS:
        batch = reached(boundary_pairs(rng, g, 1008))
        assert batch == {(g, m) for m in pattern_lengths(g)}, (g, sorted(batch))
        hit |= batch
        for count in (1, 64 // g + 1):
            assert {k for k, _ in reached(boundary_pairs(rng, g, count))} == {g}
    assert hit == wanted
    assert {g for g, _ in reached(borrow_pairs(rng))} == set(BLOCKS)
    assert {g for g, _ in reached(edge_byte_pairs(rng))} == set(BLOCKS)


@pytest.mark.parametrize("route", list(ROUTES))
def test_pair_boundaries_at_every_lane(sw, orc, scope, request, route):
    """One batch of 1008 pairs per G (four tiles: the middle ones interior), every item full: floor(64 / G) pairs side by side, a
    first block behind every last block."""
    if not in_child(request, route):
        return
    rng = np.random.default_rng(96)
    for g in BLOCKS:
        check(sw, orc, scope, route, *shuffled(rng, boundary_pairs(rng, g, 1008)))


@pytest.mark.parametrize("route", list(ROUTES))
def test_lonely_pairs_and_one_past_a_full_item(sw, orc, scope, request, route):
    """Per G a call of ONE pair (its class holds nothing else: every other slot of the item is empty, the lanes behind it hold no
    pair) and a call of 64 / G + 1 pairs (a full item and an item with one slot taken). Then all of them in one call: classes of a
    few pairs each, which the tile plan may move up into the next class, where they run with more lanes than they need."""
    if not in_child(request, route):
        return
    rng = np.random.default_rng(97)
    everything = []
    for g in BLOCKS:
        for count in (1, 64 // g + 1):
            pairs = boundary_pairs(rng, g, count)
            everything += pairs
            check(sw, orc, scope, route, [a for a, _ in pairs], [b for _, b in pairs])
    check(sw, orc, scope, route, *shuffled(rng, everything))


def borrow_pairs(rng):
    """x + S against S + y and S + y against x + S, offsets of one to three symbols, S of random letters, x and y of symbols S does not
    hold (first and last symbols differ: nothing is cut): 20 of each per G, 960 pairs."""
    pairs = []
    for g in BLOCKS:
        for offset in (1, 2, 3):
            for i in range(20):
                total = pattern_lengths(g)[i % len(pattern_lengths(g))]
                if total <= offset:
                    total = 32
                shared = bytes(LETTERS[k] for k in rng.integers(0, len(LETTERS), total - offset))
                front, back = b"x" * offset + shared, shared + b"y" * offset
                pairs += [(front, back), (back, front)]
    return pairs


@pytest.mark.parametrize("route", list(ROUTES))
def test_borrow_chains_through_every_block(sw, orc, scope, request, route):
    if not in_child(request, route):
        return
    rng = np.random.default_rng(98)
    pairs = borrow_pairs(rng)
    want = check(sw, orc, scope, route, *shuffled(rng, pairs))
    assert want.max() <= 6 and want.min() >= 1   # at most delete x, insert y: the path hugs the diagonal, one to three cells off it


def edge_byte_pairs(rng):
    pairs = []
    for g in BLOCKS:
        pairs += boundary_pairs(rng, g, 126, alphabet=EDGE_BYTES)
    return pairs


@pytest.mark.parametrize("route", list(ROUTES))
def test_edge_bytes(sw, orc, scope, request, route):
    """0x00, 0x7F, 0x80 and 0xFF in both strings: both table words of a column are all-zero-nibble, all-one-nibble and mixed."""
    if not in_child(request, route):
        return
    rng = np.random.default_rng(99)
    check(sw, orc, scope, route, *shuffled(rng, edge_byte_pairs(rng)))


def test_code_points_one_to_four_blocks(sw, orc, scope, request):
    """The code-point item runs the same column on one looked-up word: two- to four-byte symbols, patterns of one to four blocks with
    the three lengths of each, tiled and planned."""
    if not run_in_child(request, env={"STRINGWARS_AMD_TILE": str(TILE)}, test_library=True, timeout=600):
        return
    rng = np.random.default_rng(100)
    symbols = ["a", "é", "ж", "中", "😀", "z", "ü", "я"]
    items_a, items_b = [], []
    for i in range(3 * TILE + 5):
        g = 1 + i % 4
        m = pattern_lengths(g)[(i // 4) % len(pattern_lengths(g))]
        n = text_lengths(m)[(i // 12) % len(text_lengths(m))]
        a = "".join(symbols[k] for k in rng.integers(0, len(symbols), m))
        b = "".join(symbols[k] for k in rng.integers(0, len(symbols), n))
        items_a.append(("a" + a[1:-1] + "a" if m > 1 else "a").encode())
        items_b.append(("z" + b[1:-1] + "z" if n > 1 else "z").encode())
    a, b = sw.Strs(items_a).with_offsets(np.uint32), sw.Strs(items_b).with_offsets(np.uint32)
    want = orc.levenshtein_pairs(a, b, utf8=True)
    for algorithm in ("tiled", "bitparallel"):
        engine = sw.LevenshteinDistancesUTF8(capabilities=scope, algorithm=algorithm)
        for got in (engine.pairs(a, b, scope), engine.pairs(b, a, scope)):
            assert (got == want).all(), (algorithm, np.flatnonzero(got != want)[:8])


def test_dense_alphabet_long_patterns(sw, orc, scope, request):
    """bp_dense.hpp's copy of the column: patterns of 481 to 700 code points (items of 16 to 22 blocks, four, three and two pairs per
    wave with idle lanes behind them) over forty distinct symbols, which a pair's dictionary takes; 48 pairs, the planned kernel."""
    rng = np.random.default_rng(101)
    symbols = [chr(c) for c in list(range(0x430, 0x444)) + list(range(0x4E00, 0x4E0A)) + list(range(0x1F600, 0x1F60A))]
    lengths = [481, 512, 513, 543, 544, 545, 576, 577, 608, 640, 672, 700]
    items_a, items_b = [], []
    for i in range(48):
        m = lengths[i % len(lengths)]
        n = m + (i // len(lengths))
        a = "".join(symbols[k] for k in rng.integers(0, len(symbols), m))
        b = "".join(symbols[k] for k in rng.integers(0, len(symbols), n))
        items_a.append(("a" + a[1:-1] + "a").encode())
        items_b.append(("z" + b[1:-1] + "z").encode())
    assert all(blocks(len(s.decode())) >= 16 for s in items_a + items_b)
    a, b = sw.Strs(items_a).with_offsets(np.uint32), sw.Strs(items_b).with_offsets(np.uint32)
    want = orc.levenshtein_pairs(a, b, utf8=True)
    engine = sw.LevenshteinDistancesUTF8(capabilities=scope, algorithm="bitparallel")
    for got in (engine.pairs(a, b, scope), engine.pairs(b, a, scope)):
        assert (got == want).all(), np.flatnonzero(got != want)[:8]


def test_small_cross_product(sw, orc, scope, request):
    """40 queries x 36 candidates of about a hundred bytes (four blocks) as one cross-product call on the tiled route."""
    if not run_in_child(request, env={"STRINGWARS_AMD_TILE": str(TILE)}, test_library=True, timeout=600):
        return
    rng = np.random.default_rng(102)
    queries = [unlike_pair(rng, int(n), 1, LETTERS)[0] for n in rng.integers(97, 129, 40)]
    candidates = [unlike_pair(rng, 1, int(n), LETTERS)[1] for n in rng.integers(90, 129, 36)]
    got = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")(sw.Strs(queries), sw.Strs(candidates), scope)
    flat_q = sw.Strs([q for q in queries for _ in candidates]).with_offsets(np.uint32)
    flat_c = sw.Strs([c for _ in queries for c in candidates]).with_offsets(np.uint32)
    want = orc.levenshtein_pairs(flat_q, flat_c, algo="hyyro").reshape(len(queries), len(candidates))
    assert (np.asarray(got) == want).all(), np.argwhere(np.asarray(got) != want)[:8]
