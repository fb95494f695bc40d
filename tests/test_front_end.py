"""The Python front end's shared parts: the CSR result base, the one judge of ``out=`` arrays, the offset-width agreement of two raw
tapes, and the u32 exports behind the one call path."""
import numpy as np
import pytest


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,values", [("RangeMatches", np.array([4, 0, 7], np.uint32)), ("ScoreMatches", np.array([0.5, 1.0, 0.25]))])
def test_csr_results_on_a_hand_made_csr(sw, name, values):
    """Three rows -- none, (1, 4), (0) -- through both subclasses of the CSR base."""
    cls = getattr(sw, name)
    attribute = {"RangeMatches": "distances", "ScoreMatches": "scores"}[name]
    r = cls(np.array([0, 0, 2, 3], np.uint64), np.array([1, 4, 0], np.uint32), values)
    assert getattr(r, attribute) is values and r.indices.tolist() == [1, 4, 0]
    assert len(r) == 3 and r.counts.tolist() == [0, 2, 1] and r.counts.dtype == np.uint64
    indices, got = r.row(-1)
    assert indices.tolist() == [0] and got.tolist() == values[2:].tolist() and got.dtype == values.dtype and indices.dtype == np.uint32
    assert [x.tolist() for x in r.row(0)] == [[], []] and [x.tolist() for x in r.row(1)] == [[1, 4], values[:2].tolist()]
    with pytest.raises(IndexError):
        r.row(3)
    assert [x.tolist() for x in r.pairs()] == [[1, 1, 2], [1, 4, 0], values.tolist()]
    assert [x.tolist() for x in r.pairs(upper=True)] == [[1], [4], values[1:2].tolist()]
    setattr(r, attribute, values[::-1].copy())   # the values stay assignable under their own name
    assert r.row(2)[1].tolist() == values[:1].tolist()
    counted = cls(np.array([0, 0, 2, 3], np.uint64), None, None)
    assert len(counted) == 3 and counted.counts.tolist() == [0, 2, 1] and counted.indices is None and getattr(counted, attribute) is None
    with pytest.raises(ValueError):
        counted.row(1)
    with pytest.raises(ValueError):
        counted.pairs()
    for bad in ((np.zeros(0, np.uint64), None, None), (np.zeros(2, np.uint64), np.zeros(1, np.uint32), None),
                (np.zeros(2, np.uint64), np.zeros(1, np.uint32), values[:2])):
        with pytest.raises(ValueError):
            cls(*bad)


def test_output_checker_judges_numpy_arrays(sw):
    """The top-k shape (3 queries, k = 2: 6 entries of 4 bytes) and the CSR shape (4 offsets of 8 bytes, 5 indices of 4, 5 scores of 8):
    a wrong item size, a wrong entry count and a non-contiguous view each raise ValueError; the right array, a bare address and None pass."""
    check = sw.engines._check_out
    for width, entries, dtype in ((4, 6, np.uint32), (8, 4, np.uint64), (4, 5, np.uint32), (8, 5, np.float64)):
        wrong_width = np.uint64 if width == 4 else np.uint32
        check(np.zeros(entries, dtype), width, entries)
        check(np.zeros(entries, dtype).ctypes.data, width, entries)
        check(None, width, entries)
        for bad in (np.zeros(entries, wrong_width), np.zeros(entries - 1, dtype), np.zeros(entries + 1, dtype), np.zeros(2 * entries, dtype)[::2]):
            with pytest.raises(ValueError):
                check(bad, width, entries)
    check(np.zeros((3, 2), np.int32), 4, 6)   # (len(queries), k) as a matrix; a signed type of the width holds the same bits
    with pytest.raises(ValueError):
        check(np.zeros((3, 4), np.uint32)[:, ::2], 4, 6)
    # the dense outputs: the shape and the width, any strides
    check(np.zeros((3, 8), np.uint64)[:, ::2], 8, shape=(3, 4), strided=True)
    check(np.zeros((6, 2), np.uint32)[:, 1], 4, shape=(6,), strided=True)
    check(np.zeros((3, 4), np.uint64), 8, shape=(3, 4))
    check(12345, 8, shape=(3, 4))
    with pytest.raises(ValueError):
        check(np.zeros((3, 8), np.uint64)[:, ::2], 8, shape=(3, 4))   # strides only where they are allowed
    for bad in (np.zeros((3, 4), np.uint32), np.zeros((4, 3), np.uint64), np.zeros(12, np.uint64)):
        with pytest.raises(ValueError):
            check(bad, 8, shape=(3, 4), strided=True)


def test_two_raw_tapes_agree_on_one_offset_width(sw):
    """Both u32 stay u32 where the call has that form; otherwise and on disagreement host tapes are widened, a u32 device tape refused."""
    from stringwars_amd import _native as N
    pair = sw.engines._c_tapes
    wide = sw.Strs(["ab", "", "abc"])
    narrow = wide.with_offsets(np.uint32)
    device = {w: sw.DeviceTape(4096, 8192, 3, w) for w in (np.uint32, np.uint64)}   # never dereferenced here
    for a, b, u32, want64 in ((narrow, narrow, True, False), (narrow, narrow, False, True), (narrow, wide, True, True), (wide, narrow, True, True),
                              (wide, wide, True, True), (device[np.uint32], narrow, True, False), (device[np.uint32], device[np.uint32], True, False),
                              (device[np.uint64], narrow, True, True), (wide, None, False, True)):
        ta, tb, is64, keep = pair(a, b, u32=u32)
        assert is64 == want64 and isinstance(ta, N.TapeU64 if want64 else N.TapeU32) and (tb is None) == (b is None), (u32, want64)
        assert tb is None or type(tb) is type(ta)
        assert ta.count == 3 and all(k.offsets.dtype == (np.uint64 if want64 else np.uint32) for k in keep if isinstance(k, sw.Strs))
    for a, b, u32 in ((device[np.uint32], device[np.uint64], True), (device[np.uint64], device[np.uint32], True), (device[np.uint32], wide, True),
                      (device[np.uint32], device[np.uint32], False)):
        with pytest.raises(TypeError):
            pair(a, b, u32=u32)
    assert N.U32_STEMS == {"pairs"}


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pairs_keep_their_u32_exports(sw, scope):
    """``pairs`` of Levenshtein and of Needleman-Wunsch on u32 host tapes, on u32 device tapes and on a u32 beside a u64 host tape give
    what the u64 call gives; two u32 sides go to the ``*_u32tape`` export, a mix to the u64 one; a u32 device tape beside a u64 one is
    a TypeError. (Levenshtein on u32 host and device tapes of 5000 pairs: test_gpu_parity.py::test_tape_widths_residency_and_strides.)"""
    from stringwars_amd import _native as N
    a, b = sw.Strs(["kitten", "", "flaw"]), sw.Strs(["sitting", "abc", "lawn"])
    a32, b32 = a.with_offsets(np.uint32), b.with_offsets(np.uint32)
    nw = sw.NeedlemanWunschScores(substitution_matrix=sw.substitution_matrix(7), open=-3, extend=-1, capabilities=scope)
    for engine, dtype, exports in ((sw.LevenshteinDistances(capabilities=scope), np.uint32, "swh_levenshtein_pairs_%s"),
                                   (sw.LevenshteinDistancesUTF8(capabilities=scope), np.uint32, "swh_levenshtein_utf8_pairs_%s"), (nw, np.int32, "swh_nw_pairs_%s")):
        want = engine.pairs(a, b, scope)
        assert want.dtype == dtype and want.shape == (3,)
        if dtype == np.uint32:
            assert want.tolist() == [3, 3, 2]
        da, db = a32.to_device(scope), b32.to_device(scope)
        for x, y, form in ((a32, b32, "u32tape"), (da, db, "u32tape"), (da, b32, "u32tape"), (a32, b, "u64tape"), (a, b32, "u64tape"), (a, b, "u64tape")):
            got = engine.pairs(x, y, scope)
            assert got.dtype == dtype and (got == want).all(), (exports, form)
            assert engine._two_tapes(x, y, scope, "pairs").func is getattr(N.lib, exports % form), (exports, form)
        d64 = a.to_device(scope)
        for x, y in ((da, d64), (d64, db)):
            with pytest.raises(TypeError):
                engine.pairs(x, y, scope)
        assert engine._two_tapes(a32, b32, scope, "osa_pairs" if dtype == np.uint32 else "cross").func.__name__.endswith("_u64tape")
