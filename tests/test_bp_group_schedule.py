"""The byte path of the bit-parallel item's column loop (bp_item.hpp: `columns`) issues the eight match-table reads of a group of four
columns one group ahead: before the loop for an item's first group, above group 3 for the first group of the next sixteen columns, and
unconditionally, so words past the item's step count or outside a string are read and dropped. What can go wrong is at the seams: an item
that ends on, one before or one after a group or a super-step of sixteen columns, a lane whose text ends in the middle of a group while
its neighbours run on, and bytes that form any table address.

The step count of an item is n_eff = the wave maximum of n + G - 1 (n: text length, G: 32-row blocks of the pattern). Every batch here
is built for ONE value of n_eff: pairs of every pattern length of PATTERNS with texts of n_eff - G + 1 symbols, next to pairs whose texts
are one to three symbols shorter and fall into the same length bucket of the tile plan (a few pairs of a hundred symbols set the bucket
width to four), so that items mix them. Pairs share no prefix and no suffix, or the tiled kernel would cut it and shorten them.
Which string the kernel takes as the pattern is its own choice (common.hpp: bp_pattern_is_a); the test repeats it and asserts that the
batches reach every n_eff of SEAMS for G = 1 .. 4 that n >= 1 and that choice allow at all (45 of the 52 combinations).

Every case runs in a child process against the TEST library with STRINGWARS_AMD_TILE=256 (a batch spans edge tiles and interior tiles)
and compares EVERY distance with oracle.levenshtein_pairs(..., algo="hyyro"), on each route of ROUTES: prepared tapes with the side
arrays on and off, the clamped item forced, the eight- and four-wave workgroups, and the planned kernel, which runs the same item."""
import numpy as np
import pytest

from conftest import run_in_child

pytestmark = pytest.mark.gpu

TILE = 256
SEAMS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)
PATTERNS = (1, 31, 32, 33, 64, 65, 96, 97, 128)
LETTERS = bytes(range(97, 101))
ANY_BYTES = bytes((0x00, 0x7F, 0x80, 0xFF, 0x0F, 0xF0, 0x41, 0xC3))

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


def steps_of(la, lb):
    """(G, n + G - 1) of a pair as the kernel runs it; None for a pair with an empty string, which runs no item."""
    if not la or not lb:
        return None
    m, n = (la, lb) if pattern_is_a(la, lb) else (lb, la)
    return blocks(m), n + blocks(m) - 1


def unlike_pair(rng, la, lb, alphabet):
    """Two strings over `alphabet` whose first symbols differ and whose last symbols differ: no common prefix or suffix to cut."""
    a = bytearray(alphabet[i] for i in rng.integers(0, len(alphabet), la))
    b = bytearray(alphabet[i] for i in rng.integers(0, len(alphabet), lb))
    if la:
        a[0] = a[-1] = alphabet[0]
    if lb:
        b[0] = b[-1] = alphabet[1]
    return bytes(a), bytes(b)


def seam_batch(rng, n_eff, alphabet=LETTERS, per_pattern=96):
    """Pairs for one n_eff, shuffled: see the module's docstring. Returns (items_a, items_b, the set of (G, steps) they reach)."""
    pairs = []
    for m in PATTERNS:
        n = n_eff - blocks(m) + 1
        if n < 1:
            continue
        shorter = [k for k in range(n - n % 4, n) if k >= 1]   # the other lengths of n's bucket (bucket = n >> 2)
        for i in range(per_pattern):
            text = n if i % 2 == 0 or not shorter else shorter[(i // 2) % len(shorter)]
            pairs.append(unlike_pair(rng, m, text, alphabet))
    pairs += [unlike_pair(rng, 100, 100, alphabet) for _ in range(8)]   # longest text 100: buckets of four lengths
    order = rng.permutation(len(pairs))
    items_a, items_b = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    reached = {steps_of(len(a), len(b)) for a, b in pairs}
    return items_a, items_b, reached


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
    return want, pa, pb, engine


@pytest.mark.parametrize("route", list(ROUTES))
def test_group_and_super_step_seams(sw, orc, scope, request, route):
    """One batch per n_eff of SEAMS (about 800 pairs, four tiles: the middle ones interior). Items end on every seam of the schedule:
    after the first column, inside and at the end of the first group, around sixteen, thirty-two and forty-eight columns; odd values
    leave the last group partly beyond n_eff, and the shorter texts of a bucket end inside a group whose other lanes run on."""
    if not in_child(request, route):
        return
    rng = np.random.default_rng(91)
    reached = set()
    for n_eff in SEAMS:
        items_a, items_b, hit = seam_batch(rng, n_eff)
        assert len(items_a) > 3 * TILE or n_eff < 4
        reached |= hit
        check(sw, orc, scope, route, items_a, items_b)
    # every (G, n_eff) that any pattern of G blocks reaches at all: at n_eff = 33 a text of 33 - G + 1 symbols is the cheaper PATTERN
    # for every pattern of two to four blocks, so the kernel never runs those three
    wanted = {(g, t) for g in (1, 2, 3, 4) for t in SEAMS
              if t >= g and any(steps_of(m, t - g + 1) == (g, t) for m in range(32 * g - 31, 32 * g + 1))}
    assert len(wanted) == 45 and not wanted - reached, sorted(wanted - reached)   # 52 less four with n < 1 and those three


@pytest.mark.parametrize("route", list(ROUTES))
def test_any_byte_forms_an_address(sw, orc, scope, request, route):
    """Strings over 0x00, 0x7F, 0x80, 0xFF and bytes with one nibble empty: both nibbles of any byte index the tables. Then a batch
    of identical pairs (the tiled kernel cuts them to nothing, the planned one walks them) and a batch whose strings share no byte."""
    if not in_child(request, route):
        return
    rng = np.random.default_rng(92)
    for n_eff in (5, 17, 33, 48):
        items_a, items_b, _ = seam_batch(rng, n_eff, alphabet=ANY_BYTES, per_pattern=64)
        check(sw, orc, scope, route, items_a, items_b)
    lengths = rng.integers(1, 130, 3 * TILE + 7)
    same = [bytes(ANY_BYTES[i] for i in rng.integers(0, len(ANY_BYTES), int(n))) for n in lengths]
    want, _, _, _ = check(sw, orc, scope, route, same, list(same))
    assert (want == 0).all()
    low = [bytes(rng.integers(0x00, 0x40, int(n), dtype=np.uint8)) for n in lengths]
    high = [bytes(rng.integers(0xC0, 0x100, int(n), dtype=np.uint8)) for n in lengths[::-1]]
    want, _, _, _ = check(sw, orc, scope, route, low, high)
    assert (want == np.maximum(lengths, lengths[::-1])).all()


@pytest.mark.parametrize("route", list(ROUTES))
def test_tape_edges_and_narrow_windows(sw, orc, scope, request, route):
    """The first and the last strings of both tapes (edge tiles: clamped windows, the reads one group ahead run past the tape's data
    there) as pairs that end on a seam; views, whose tapes end where the view ends; and a tape of fewer than sixteen bytes in all,
    which is read through the narrow windows, against an ordinary one and against itself."""
    if not in_child(request, route):
        return
    rng = np.random.default_rng(93)
    for n_eff in (4, 16, 17, 49):
        items_a, items_b, _ = seam_batch(rng, n_eff)
        for at in (0, 1, -2, -1):
            m = PATTERNS[(at + n_eff) % len(PATTERNS)]
            items_a[at], items_b[at] = unlike_pair(rng, m, max(n_eff - blocks(m) + 1, 1), LETTERS)
        want, pa, pb, engine = check(sw, orc, scope, route, items_a, items_b)
        last = len(items_a)
        for lo, hi in ((0, 300), (last - 300, last), (259, last - 259)):
            assert (engine.pairs(pa[lo:hi], pb[lo:hi], scope) == want[lo:hi]).all(), (n_eff, lo, hi)
    ordinary, _, _ = seam_batch(rng, 15, per_pattern=57)
    ordinary = ordinary[:2 * TILE]
    narrow = [b"acb" if i % 128 == 5 else b"" for i in range(2 * TILE)]   # 4 x 3 = 12 bytes: shorter than one 16-byte window
    assert sum(map(len, narrow)) < 16 and len(ordinary) == len(narrow)
    for items_a, items_b in ((narrow, ordinary), (narrow, narrow), (narrow, narrow[::-1])):
        check(sw, orc, scope, route, items_a, items_b)


def test_code_points_keep_their_schedule(sw, orc, scope, request):
    """The code-point item (seven group reads per column) is the same lambda with its old schedule: one batch around the seams through
    LevenshteinDistancesUTF8, two- to four-byte symbols, tiled and planned."""
    if not run_in_child(request, env={"STRINGWARS_AMD_TILE": str(TILE)}, test_library=True, timeout=600):
        return
    rng = np.random.default_rng(94)
    symbols = ["a", "é", "ж", "中", "😀", "z", "ü", "я"]
    items_a, items_b = [], []
    for i in range(3 * TILE + 5):
        m, n_eff = PATTERNS[i % len(PATTERNS)], SEAMS[i % len(SEAMS)]
        n = max(n_eff - blocks(m) + 1, 1)
        a = "".join(symbols[k] for k in rng.integers(0, len(symbols), m))
        b = "".join(symbols[k] for k in rng.integers(0, len(symbols), n))
        items_a.append(("a" + a[1:-1] + "a" if m > 1 else "a").encode())
        items_b.append(("z" + b[1:-1] + "z" if n > 1 else "z").encode())
    a, b = sw.Strs(items_a).with_offsets(np.uint32), sw.Strs(items_b).with_offsets(np.uint32)
    want = orc.levenshtein_pairs(a, b, utf8=True)
    for algorithm in ("tiled", "bitparallel"):
        got = sw.LevenshteinDistancesUTF8(capabilities=scope, algorithm=algorithm).pairs(a, b, scope)
        assert (got == want).all(), (algorithm, np.flatnonzero(got != want)[:8])
