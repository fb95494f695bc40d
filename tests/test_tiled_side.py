"""The headline tiled kernel plans a tile from the side arrays of two prepared byte tapes (tiled.hip: kSide; api.hip: k_tape_side):
per string its first and its last sixteen bytes, positions outside the tape as zero, the neighbouring strings' bytes included.
Every case runs in a child process against the TEST library with STRINGWARS_AMD_TILE=256 and STRINGWARS_AMD_TILED_WAVES=16, so that a
small batch spans several tiles of the sixteen-wave workgroup, with algorithm="tiled"; it compares EVERY distance with the oracle, and it
runs twice: with STRINGWARS_AMD_SIDE=1 (the arrays are built for tapes of any size and the kernel reads them) and with
STRINGWARS_AMD_SIDE=0 (never built: the windows are read from the tapes as before). Both must equal the oracle, so they equal each other.
Whether a prepared tape carries the arrays is read back through the test library's swh_debug_prepared_side, and how often
k_bitparallel_tiled_side was launched through its swh_debug_tiled_side_launches, so neither mode can pass by running the other one's path."""
import ctypes as C

import numpy as np
import pytest

from conftest import run_in_child

pytestmark = pytest.mark.gpu

TILE = 256
MODES = {"side": "1", "no_side": "0"}
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 96, 256)


def in_child(request, mode):
    env = {"STRINGWARS_AMD_TILE": str(TILE), "STRINGWARS_AMD_TILED_WAVES": "16", "STRINGWARS_AMD_SIDE": MODES[mode]}
    return run_in_child(request, env=env, test_library=True, timeout=600)


def side_arrays(prepared, count):
    """(count, 2, 16) bytes: head and tail of the tape's first `count` strings, or None where the tape has no side arrays."""
    from stringwars_amd import _native as N
    fn = N.lib.swh_debug_prepared_side
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_size_t], C.c_size_t
    out = np.zeros((max(count, 1), 2, 16), np.uint8)
    got = fn(prepared._handle, out.ctypes.data, count)
    return out[:count] if got == count and count else None


def side_launches():
    """How often this process has launched k_bitparallel_tiled_side (the test library counts it where it chooses the kernel)."""
    from stringwars_amd import _native as N
    fn = N.lib.swh_debug_tiled_side_launches
    fn.argtypes, fn.restype = [], C.c_ulonglong
    return int(fn())


def random_bytes(rng, n, letters=4):
    return rng.integers(97, 97 + letters, n, dtype=np.uint8).tobytes()


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
    """Lengths 0 .. longest; equal strings, prefixes, mutated copies (long common affixes) and unrelated strings."""
    items_a, items_b = [], []
    for i in range(count):
        a = random_bytes(rng, int(rng.integers(0, longest + 1)))
        kind = i % 8
        if kind == 0:
            b = a
        elif kind == 1:
            b = a[: len(a) // 2] if i % 16 == 1 else a[len(a) // 3:]
        elif kind < 5:
            b = mutated(rng, a, int(rng.integers(1, 5)))
        else:
            b = random_bytes(rng, int(rng.integers(0, longest + 1)))
        items_a.append(a)
        items_b.append(b)
    return items_a, items_b


def check_prepared(sw, orc, scope, mode, items_a, items_b):
    """Two prepared tapes with 32-bit offsets, both orders, every distance against the oracle. Returns (want, pa, pb)."""
    a, b = sw.Strs(items_a).with_offsets(np.uint32), sw.Strs(items_b).with_offsets(np.uint32)
    want = orc.levenshtein_pairs(a, b)
    pa, pb = sw.PreparedTape(scope, a), sw.PreparedTape(scope, b)
    for tape in (pa, pb):
        assert (side_arrays(tape, 1) is not None) == (mode == "side"), "the mode decides whether a tape carries side arrays"
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")
    before = side_launches()
    got = engine.pairs(pa, pb, scope)
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    got = engine.pairs(pb, pa, scope)
    assert (got == want).all(), ("swapped", np.flatnonzero(got != want)[:8])
    # which kernel the two calls ran on: tapes shorter than a window cut no affixes, but are still launched on the side kernel
    assert side_launches() - before == (2 if mode == "side" else 0), "the mode decides which kernel a call on two prepared tapes runs on"
    return want, pa, pb


@pytest.mark.parametrize("mode", list(MODES))
def test_lengths_on_both_sides(sw, orc, scope, request, mode):
    """Every length of LENGTHS against every other: unrelated strings, one string a prefix and a suffix of the other (equal strings where
    the lengths are equal: the affix is the whole string), copies with one symbol changed in the middle (affixes of sixteen and more),
    and pairs whose common prefix and suffix overlap, so that both clamps bind. 470 pairs: two tiles."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(81)
    items_a, items_b = [], []
    for la in LENGTHS:
        for lb in LENGTHS:
            a, b = random_bytes(rng, la), random_bytes(rng, lb)
            longer = a if la >= lb else b
            short = min(la, lb)
            edited = bytearray(longer)
            if edited:
                edited[len(edited) // 2] = ord("z")
            for x, y in ((a, b), (longer, longer[:short]), (longer[len(longer) - short:], longer), (longer, bytes(edited))):
                items_a.append(x)
                items_b.append(y)
    for x, y in ((b"aaaa", b"aaaaaa"), (b"a" * 20, b"a" * 30), (b"ab" * 10, b"ab" * 9), (b"a" * 16, b"a" * 17), (b"a" * 33, b"a" * 31),
                 (b"abcabc", b"abc"), (b"x", b"x"), (b"", b""), (b"ba" * 8, b"ba" * 8 + b"b"), (b"a" * 256, b"a" * 255)) * 7:
        items_a.append(x)
        items_b.append(y)
    assert 400 < len(items_a) < 2 * TILE
    check_prepared(sw, orc, scope, mode, items_a, items_b)


@pytest.mark.parametrize("mode", list(MODES))
def test_tape_edges(sw, orc, scope, request, mode):
    """The first and the last strings of both tapes are shorter than sixteen bytes, so their head and tail windows run past the tapes' ends
    and the padding is read -- equal, prefix and unrelated ones --; then tapes of fewer than sixteen bytes in all, and of sixteen to
    thirty-one, against an ordinary tape and each other."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(82)
    for first_a, first_b, last_a, last_b in ((b"abc", b"abd", b"dcba", b"dcb"), (b"abcabc", b"abcabc", b"ab", b"ab"), (b"", b"abc", b"abc", b""),
                                             (b"a", b"aa", b"aaa", b"a"), (b"abcdefghijklmno", b"abcdefghijklmn", b"zabcdefghijklmn", b"abcdefghijklmn")):
        items_a, items_b = token_pairs(rng, 3 * TILE)
        items_a[0], items_b[0], items_a[-1], items_b[-1] = first_a, first_b, last_a, last_b
        items_a[1], items_b[1] = first_a[:2], first_a[:2]      # the second string starts inside the first sixteen bytes, too
        items_a[-2], items_b[-2] = last_b[-2:], last_b[-2:]
        check_prepared(sw, orc, scope, mode, items_a, items_b)
    tiny = [b"ab" if i % 60 == 0 else b"" for i in range(2 * TILE)]       # 9 strings of two bytes: 18 bytes
    tiny[-1] = b""
    tinier = [b"abc" if i % 128 == 5 else b"" for i in range(2 * TILE)]   # 4 x 3 = 12 bytes: a tape shorter than one window
    assert 16 <= sum(map(len, tiny)) < 32 and sum(map(len, tinier)) < 16
    ordinary, _ = token_pairs(rng, 2 * TILE)
    for items_a, items_b in ((tiny, ordinary), (tinier, ordinary), (tiny, tinier), (tinier, tinier), (tiny, tiny)):
        check_prepared(sw, orc, scope, mode, items_a, items_b)


@pytest.mark.parametrize("mode", list(MODES))
def test_planted_neighbours(sw, orc, scope, request, mode):
    """A string's windows show its neighbours' bytes. Here the strings after a pair go on with the same bytes on both tapes, and the
    strings before it end with the same bytes, so that the pair's common prefix and suffix would come out longer than its shorter string
    if they were not clamped to the pair's own lengths; and words over two letters, where that happens by chance everywhere."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(83)
    items_a, items_b = [], []
    for i in range(TILE):
        core = random_bytes(rng, int(rng.integers(0, 9)))
        # prefix plant: head(a) = core + "xyQrs...", head(b) = core + "xy" + "Qrs..."
        items_a += [core, b"xyQrs" + core]
        items_b += [core + b"xy", b"Qrs" + core]
        # suffix plant: tail(a) = "...rsPxy" + core, tail(b) = "...rsP" + "xy" + core
        items_a += [b"rsPxy", core]
        items_b += [b"rsP", b"xy" + core]
    for i in range(2 * TILE):
        items_a.append(random_bytes(rng, int(rng.integers(0, 7)), letters=2))
        items_b.append(random_bytes(rng, int(rng.integers(0, 7)), letters=2))
    check_prepared(sw, orc, scope, mode, items_a, items_b)


@pytest.mark.parametrize("mode", list(MODES))
def test_views_and_one_tape_against_itself(sw, orc, scope, request, mode):
    """Sub-views with the same and with different first strings on the two sides (the side arrays move with the offsets), and one prepared
    tape against itself, whole and as two views."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(84)
    items_a, items_b = token_pairs(rng, 6 * TILE)
    want, pa, pb = check_prepared(sw, orc, scope, mode, items_a, items_b)
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")
    assert (engine.pairs(pa[300:1300], pb[300:1300], scope) == want[300:1300]).all()
    shifted = orc.levenshtein_pairs(sw.Strs(items_a[100:900]), sw.Strs(items_b[500:1300]))
    assert (engine.pairs(pa[100:900], pb[500:1300], scope) == shifted).all()
    assert (engine.pairs(pb[500:1300], pa[100:900], scope) == shifted).all()
    assert (engine.pairs(pa, pa, scope) == 0).all()
    halves = orc.levenshtein_pairs(sw.Strs(items_a[:700]), sw.Strs(items_a[700:1400]))
    assert (engine.pairs(pa[:700], pa[700:1400], scope) == halves).all()
    assert (engine.pairs(pa[1:701], pa[700:1400], scope) == orc.levenshtein_pairs(sw.Strs(items_a[1:701]), sw.Strs(items_a[700:1400]))).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_calls_that_do_not_read_the_arrays(sw, orc, scope, request, mode):
    """With the arrays present, the calls that must not use them still equal the oracle: a bound, a cross-product, tapes with 64-bit
    offsets (which never carry the arrays) and raw device tapes. (A prepared tape against a raw one is no call: the engines refuse it.)
    And a UTF-8 engine on prepared tapes that are pure ASCII, which runs on the byte kernels and does read them."""
    if not in_child(request, mode):
        return
    rng = np.random.default_rng(85)
    items_a, items_b = token_pairs(rng, 3 * TILE)
    want, pa, pb = check_prepared(sw, orc, scope, mode, items_a, items_b)
    engine = sw.LevenshteinDistances(capabilities=scope, algorithm="tiled")
    for bound in (0, 3, 40):
        assert (engine.pairs(pa, pb, scope, bound=bound) == np.minimum(want, bound + 1)).all(), bound
    got = engine(pa[5:45], pb[700:748], scope)
    cross_want = orc.levenshtein_pairs(sw.Strs([q for q in items_a[5:45] for _ in range(48)]), sw.Strs(items_b[700:748] * 40))
    assert (got.reshape(-1) == cross_want).all()
    a, b = sw.Strs(items_a), sw.Strs(items_b)
    wide_a, wide_b = sw.PreparedTape(scope, a.with_offsets(np.uint64)), sw.PreparedTape(scope, b.with_offsets(np.uint64))
    assert side_arrays(wide_a, 1) is None and side_arrays(wide_b, 1) is None
    assert (engine.pairs(wide_a, wide_b, scope) == want).all()
    raw_a, raw_b = a.with_offsets(np.uint32).to_device(scope), b.with_offsets(np.uint32).to_device(scope)
    assert (engine.pairs(raw_a, raw_b, scope) == want).all()
    assert (engine.pairs(raw_b, raw_a, scope) == want).all()
    with pytest.raises(TypeError):
        engine.pairs(pa, raw_b, scope)
    # tapes prepared from device tapes are used in place: no pad behind their data
    placed_a, placed_b = sw.PreparedTape(scope, raw_a), sw.PreparedTape(scope, raw_b)
    assert (engine.pairs(placed_a, placed_b, scope) == want).all()
    utf8_engine = sw.LevenshteinDistancesUTF8(capabilities=scope, algorithm="tiled")
    ua, ub = sw.PreparedTape(scope, a.with_offsets(np.uint32), utf8=True), sw.PreparedTape(scope, b.with_offsets(np.uint32), utf8=True)
    assert ua.info["ascii"] and (side_arrays(ua, 1) is not None) == (mode == "side")
    assert (utf8_engine.pairs(ua, ub, scope) == want).all()


def test_the_builder_against_numpy_slices(sw, scope, request):
    """The side arrays read back and compared with slices of the tape: head = bytes [start, start + 16), tail = [end - 16, end), zero
    outside the tape -- an ordinary tape, one whose first and last strings are shorter than a window, one shorter than a window in all,
    one that ends in empty strings, and a single string."""
    if not in_child(request, "side"):
        return
    rng = np.random.default_rng(86)
    ordinary, _ = token_pairs(rng, 700)
    short_ends = [b"abc", b"", b"de"] + ordinary[:300] + [b"fgh", b"", b"i"]
    cases = (ordinary, short_ends, [b"ab", b"", b"cde", b"", b"f"], ordinary[:50] + [b""] * 20, [b"abcdefghijklmnopqrstuvwxyz"], [b"abc"], [b""])
    for items in cases:
        tape = sw.Strs(items).with_offsets(np.uint32)
        prepared = sw.PreparedTape(scope, tape)
        got = side_arrays(prepared, len(items))
        assert got is not None
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in items])]).astype(np.int64)
        padded = np.concatenate([np.zeros(16, np.uint8), np.frombuffer(b"".join(items), np.uint8), np.zeros(16, np.uint8)])
        for i in range(len(items)):
            head, tail = padded[16 + offsets[i]: 32 + offsets[i]], padded[offsets[i + 1]: 16 + offsets[i + 1]]
            assert (got[i, 0] == head).all() and (got[i, 1] == tail).all(), (len(items), i)
