"""The tiled Levenshtein kernel's two items: tiles away from both ends of both tapes read their strings through unclamped windows
(bp_item.hpp: kBpInterior), the tiles that hold a tape's first or last strings, and tapes shorter than the margins, through the clamped
ones. Every case runs against the TEST library with STRINGWARS_AMD_TILE=256 and algorithm="tiled", so that a small batch spans
several tiles (first = edge, middle = interior, last = edge), compares EVERY distance with the oracle, and runs three times: as
shipped, with the interior variant forced off (STRINGWARS_AMD_INTERIOR=0: the same outputs, since both equal the oracle's), and as
shipped on the sixteen-wave workgroup of the headline configuration."""
import numpy as np
import pytest

from conftest import run_in_child

pytestmark = pytest.mark.gpu

MARGIN_LO, MARGIN_HI = 64, 32   # bp_item.hpp: kBpMarginLo, kBpMarginHi
TILE = 256

MODES = {"interior": {}, "forced_off": {"STRINGWARS_AMD_INTERIOR": "0"}, "sixteen_waves": {"STRINGWARS_AMD_TILED_WAVES": "16"}}


def in_child(request, mode):
    return run_in_child(request, env=dict(MODES[mode], STRINGWARS_AMD_TILE=str(TILE)), test_library=True, timeout=600)


def mutated(rng, s, edits):
    b = bytearray(s)
    for _ in range(edits):
        op, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(b) + 1))
        if op == 0 and pos < len(b):
            b[pos] = int(rng.integers(97, 101))
        elif op == 1:
            b.insert(pos, int(rng.integers(97, 101)))
        elif pos < len(b):
            del b[pos]
    return bytes(b)


def token_pairs(rng, count, longest=96):
    """Lengths 0 .. longest with empty and equal strings among them; half mutated copies, half unrelated."""
    items_a, items_b = [], []
    for i in range(count):
        a = rng.integers(97, 101, int(rng.integers(0, longest + 1)), dtype=np.uint8).tobytes()
        kind = i % 8
        if kind == 0:
            b = a
        elif kind == 1:
            b = b"" if i % 16 == 1 else a[: len(a) // 2]
        elif kind < 4:
            b = mutated(rng, a, int(rng.integers(1, 7)))
        else:
            b = rng.integers(97, 101, int(rng.integers(0, longest + 1)), dtype=np.uint8).tobytes()
        if kind == 7 and i % 16 == 7:
            a = b""
        items_a.append(a)
        items_b.append(b)
    return items_a, items_b


def check_pairs(sw, orc, scope, items_a, items_b, widths=(np.uint32,)):
    a, b = sw.Strs(items_a), sw.Strs(items_b)
    want = orc.levenshtein_pairs(a, b)
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")
    for width in widths:
        # (device tapes: the kernel sees exactly these bytes and offsets, nothing re-staged)
        wa, wb = a.with_offsets(width).to_device(scope), b.with_offsets(width).to_device(scope)
        got = engine.pairs(wa, wb, scope)
        assert (got == want).all(), (width, np.flatnonzero(got != want)[:8])
        got = engine.pairs(wb, wa, scope)
        assert (got == want).all(), (width, "swapped", np.flatnonzero(got != want)[:8])
    return want


@pytest.mark.parametrize("mode", list(MODES))
def test_tokens_across_edge_and_interior_tiles(sw, orc, scope, request, mode):
    """1536 byte pairs = six tiles; the first string starts at byte 0 of its tape and the last one ends at the tape's end."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(71)
    items_a, items_b = token_pairs(rng, 1536)
    items_a[0], items_b[0] = b"abcabcabc", b"abdabcab"
    items_a[-1], items_b[-1] = b"dcbadcba", b"dcbaadcb"
    want = check_pairs(sw, orc, scope, items_a, items_b)
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")
    a, b = sw.Strs(items_a).with_offsets(np.uint32), sw.Strs(items_b).with_offsets(np.uint32)
    assert (engine.pairs(a, b, scope) == want).all()   # host tapes, staged by the call
    for bound in (0, 3, 40):
        assert (engine.pairs(a, b, scope, bound=bound) == np.minimum(want, bound + 1)).all()
    pa, pb = sw.PreparedTape(scope, a), sw.PreparedTape(scope, b)
    assert (engine.pairs(pa, pb, scope) == want).all()
    assert (engine.pairs(pa[300:1300], pb[300:1300], scope) == want[300:1300]).all()   # a view: its tapes end where the view ends


@pytest.mark.parametrize("mode", list(MODES))
def test_the_switch_is_exact_at_both_margins(sw, orc, scope, request, mode):
    """The first tile is one pad string and 255 empty ones, so the second tile's lowest start lies exactly margin - 1, margin and
    margin + 1 bytes behind the tape's start; the mirror image in front of the tape's end; either tape alone at the threshold and
    both; and tapes shorter than either margin, which never take the interior variant."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(72)
    body_a, body_b = token_pairs(rng, 2 * TILE)
    far = b"z" * 200
    for delta in (-1, 0, 1):
        for lead_a, lead_b, tail_a, tail_b in (
                (MARGIN_LO + delta, MARGIN_LO + delta, 200, 200), (MARGIN_LO + delta, 200, 200, 200), (200, MARGIN_LO + delta, 200, 200),
                (200, 200, MARGIN_HI + delta, MARGIN_HI + delta), (200, 200, MARGIN_HI + delta, 200), (200, 200, 200, MARGIN_HI + delta),
                (MARGIN_LO + delta, MARGIN_LO - delta, MARGIN_HI - delta, MARGIN_HI + delta)):
            empties = [b""] * (TILE - 1)
            items_a = [far[:lead_a]] + empties + body_a + empties + [far[:tail_a]]
            items_b = [far[:lead_b]] + empties + body_b + empties + [far[:tail_b]]
            check_pairs(sw, orc, scope, items_a, items_b)
    # tapes shorter than a margin (16 bytes or more, so they are still read with 128-bit loads), against an ordinary tape and each other
    tiny = [b"ab" if i % 40 == 0 else b"" for i in range(3 * TILE)]   # 20 strings of two bytes: 40 bytes
    assert MARGIN_HI < sum(map(len, tiny)) < MARGIN_LO
    shorter = [b"abc" if i % 96 == 5 else b"" for i in range(3 * TILE)]   # 8 x 3 = 24 bytes: below both margins
    assert 16 <= sum(map(len, shorter)) < MARGIN_HI
    ordinary, _ = token_pairs(rng, 3 * TILE)
    check_pairs(sw, orc, scope, tiny, ordinary)
    check_pairs(sw, orc, scope, shorter, ordinary)
    check_pairs(sw, orc, scope, tiny, shorter)


def block_count_batch(rng, count):
    """Patterns of 1, 2, 3 and 64 blocks of 32 rows in one batch (2048 bytes: block 63 reads its text 63 bytes in front of the
    string's start), the long ones inside the batch and at both of its ends."""
    items_a, items_b = token_pairs(rng, count)
    long_at = {0, 1, count // 2 - 1, count // 2, count // 2 + 1, count - 2, count - 1} | set(range(TILE + 3, min(count, 2 * TILE), 37))
    for i in sorted(long_at):
        a = rng.integers(97, 101, 2048, dtype=np.uint8).tobytes()
        items_a[i] = a
        items_b[i] = mutated(rng, a, 9)[:2048] if i % 2 else rng.integers(97, 101, int(rng.integers(1, 2049)), dtype=np.uint8).tobytes()
    for i in range(5, count, 11):   # two and three blocks for certain
        if i not in long_at:
            items_a[i] = rng.integers(97, 101, 33 + i % 60, dtype=np.uint8).tobytes()
            items_b[i] = mutated(rng, items_a[i], 4)
    return items_a, items_b


@pytest.mark.parametrize("pairs", [512, 768])
@pytest.mark.parametrize("mode", list(MODES))
def test_block_counts_1_2_3_and_64_in_one_batch(sw, orc, scope, request, mode, pairs):
    """512 pairs are two tiles, each at one end of the tapes; 768 put a tile between them. With 32-bit and with 64-bit offsets."""
    if not in_child(request, mode):
        return
    items_a, items_b = block_count_batch(np.random.default_rng(73 + pairs), pairs)
    check_pairs(sw, orc, scope, items_a, items_b, widths=(np.uint32, np.uint64))


@pytest.mark.parametrize("mode", list(MODES))
def test_cross_product_tiles_scatter_their_candidates(sw, orc, scope, request, mode):
    """48 x 48 through the tiled route: a tile is five rows and a bit, so its candidates span their whole tape -- both ends -- while
    its queries are interior from the second tile on; and the reverse. Then rows longer than a tile (4 queries out of a longer
    tape x 768 candidates): the middle third of a row is interior on both tapes, with candidates that are NOT the tile's first and
    last pair's."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(74)
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")

    def check_cross(queries, candidates):
        got = engine(queries.to_device(scope), candidates.to_device(scope), scope)   # (a view's data goes up whole: its pad stays in front)
        q_items = [queries[i] for i in range(len(queries))]
        c_items = [candidates[j] for j in range(len(candidates))]
        want = orc.levenshtein_pairs(sw.Strs([q for q in q_items for _ in c_items]), sw.Strs(c_items * len(q_items)))
        assert (got.reshape(-1) == want).all(), np.flatnonzero(got.reshape(-1) != want)[:8]

    items_q, items_c = token_pairs(rng, 48, longest=80)
    check_cross(sw.Strs(items_q), sw.Strs(items_c))
    check_cross(sw.Strs(items_c), sw.Strs(items_q))
    wide_q, wide_c = token_pairs(rng, 768, longest=60)
    padded = sw.Strs([b"y" * 100] + [q + b"cd" for q in wide_q[:5]])
    check_cross(padded.subview(1, 5), sw.Strs(wide_c))
    check_cross(sw.Strs(wide_c), padded.subview(1, 5))
