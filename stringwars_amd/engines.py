"""Host-side mirror of the engine interface the reference benchmarks drive.

Names, argument meaning and error behaviour follow the ``stringzillas`` Python surface used by
``similarities/bench.py`` (``szs.DeviceScope(gpu_device=0)`` :360, ``sz.Strs(list)`` :399,
``engine_class(capabilities=scope)`` :403, ``engine(queries, candidates, scope, out=matrix)``
:421-422, ``NeedlemanWunschScores(byte_to_class, costs, open=, extend=, capabilities=)``
:466-472) and the Rust ``szs`` types of ``similarities/bench.rs:79-82``. On top of the reference's
cross-product call every engine has the pairwise batch the north-star asks for
(``engine.pairs(a, b, scope, bound=..., out=...)``), the shape of the only pairwise batched call in
the reference, ``cudf ... str.edit_distance`` (``bench.py:596-604``).

Everything here is plumbing over the C ABI (``include/stringwars_amd.h``); all arithmetic happens
in the HIP kernels. Inputs may live on the host (numpy) or on the device (``DeviceTape``, torch
CUDA tensors); device-resident inputs are used in place.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from . import _native as N
from .results import Alignments, InfixMatches, InfixOccurrences, PartialAlignments, RangeMatches, ScoreMatches  # noqa: F401
from .tapes import (  # noqa: F401  (every name that was reachable as ``engines.X`` still is)
    DeviceScope, DeviceTape, PreparedTape, ShardedCross, ShardedPairs, Strs, TapeLike, shard_cuts,
    _as_tape, _c_tape, _c_tapes, _Owner, _pointer, _symbol_lengths,
)

__all__ = [
    "DeviceScope", "Strs", "DeviceTape", "PreparedTape", "ShardedPairs", "shard_cuts", "LevenshteinDistances", "LevenshteinDistancesUTF8",
    "NeedlemanWunschScores", "SmithWatermanScores", "edit_distance", "StringWarsError", "UNBOUNDED", "TOPK_MAX",
    "ALIGN_MAX_CELLS", "Alignments", "RangeMatches", "ScoreMatches", "INFIX_MAX_PATTERN", "INFIX_NONE", "InfixMatches", "InfixOccurrences", "OSA_MAX_SHORTER", "LCS_MAX_SHORTER", "PARTIAL_MAX_NEEDLE", "PartialAlignments",
    "JARO_MAX_LENGTH", "TOKEN_MAX_BYTES", "SCORERS",
]

StringWarsError = N.StringWarsError
UNBOUNDED = N.UNBOUNDED
TOPK_MAX = N.TOPK_MAX
ALIGN_MAX_CELLS = N.ALIGN_MAX_CELLS
INFIX_MAX_PATTERN = N.INFIX_MAX_PATTERN
INFIX_NONE = N.INFIX_NONE
OSA_MAX_SHORTER = N.OSA_MAX_SHORTER
LCS_MAX_SHORTER = N.LCS_MAX_SHORTER
PARTIAL_MAX_NEEDLE = N.PARTIAL_MAX_NEEDLE
JARO_MAX_LENGTH = N.JARO_MAX_LENGTH
TOKEN_MAX_BYTES = N.TOKEN_MAX_BYTES
SCORERS = tuple(N.SCORERS)   # the scorers of ``engine.extract``, by name


def _need_scope(scope) -> None:
    if scope is None:
        raise ValueError("a DeviceScope is required")


def _bound(bound: Optional[int]) -> C.c_uint32:
    """The bound of a call as the library takes it: ``UNBOUNDED`` for None."""
    return C.c_uint32(N.UNBOUNDED if bound is None else int(bound))


def _double_bits(x: float) -> C.c_uint64:
    """A float64 argument as the library takes it: the 64 bits that memcpy of the double gives."""
    return C.c_uint64(int(np.float64(x).view(np.uint64)))


def _check_out(out, width: int, entries: Optional[int] = None, *, shape: Optional[tuple] = None, strided: bool = False) -> None:
    """Judges one ``out=`` array or tensor before its address goes to the library, which cannot know its size; ``ValueError``.
    ``entries``: a flat output (top-k, extract, the CSR arrays) -- a numpy array or torch tensor of that many elements of ``width``
    bytes, contiguous. ``shape``: a dense output -- a numpy array of that shape and width, of any strides where ``strided``, else
    contiguous; a tensor there is taken as memory, as it always was (the dense calls take device memory by tensor or address).
    A bare address is unchecked everywhere, and so is an object that is neither array nor tensor (a ctypes pointer). None, an
    output that is not wanted, passes."""
    if out is None or isinstance(out, int):
        return
    if shape is not None:
        if isinstance(out, np.ndarray) and (out.dtype.itemsize != width or out.shape != shape or not (strided or out.flags.c_contiguous)):
            raise ValueError("an output must be a %s array of %d-bit entries" % (shape, 8 * width))
        return
    numel = getattr(out, "numel", None)   # torch.Tensor (this runs twice in a search of ~100 us: one lookup, not hasattr and another)
    if numel is not None:
        fits = numel() == entries and out.element_size() == width and out.is_contiguous()
    else:
        fits = not isinstance(out, np.ndarray) or (out.size == entries and out.dtype.itemsize == width and out.flags.c_contiguous)
    if not fits:
        raise ValueError("an output must hold %d contiguous %d-bit entries" % (entries, 8 * width))


def _stride(out, cross: bool) -> int:
    """The first-axis stride in bytes of a numpy output; 0, the library's "contiguous", for anything else and for a single pair."""
    if isinstance(out, np.ndarray) and (cross or (out.ndim == 1 and out.size > 1)):
        return out.strides[0]
    return 0


_EXPORTS = {}   # (engine type, stem, form) -> the export, as _Engine._two_tapes found it


class _Engine(_Owner):
    _utf8 = False
    _prefix = "swh_levenshtein"   # of every export of the engine: ``<prefix>_init``, ``<prefix>_free``, ``<prefix>_<stem>_<form>``
    _free = "swh_levenshtein_free"

    def _promoted(self, a, b, scope, at=()):
        """Both tapes as PreparedTapes where either is of a type in ``at`` (measured on the device, like the raw calls do internally);
        as they are otherwise. ``b`` may be None."""
        a = _as_tape(a)
        b = None if b is None else _as_tape(b)
        if isinstance(a, at) or isinstance(b, at):
            a = a if isinstance(a, PreparedTape) else PreparedTape(scope, a, utf8=self._utf8)
            if b is not None and not isinstance(b, PreparedTape):
                b = PreparedTape(scope, b, utf8=self._utf8)
        return a, b

    def _need_mode(self, tape: "PreparedTape") -> None:
        if self._utf8 != tape.utf8:
            raise ValueError("a %s engine needs tapes prepared with utf8=%s" % (type(self).__name__, self._utf8))

    def _export(self, stem, form):
        name = "%s_prepared" % stem if form == "prepared" else "%s%s_%s" % ("utf8_" if self._utf8 else "", stem, form)
        fn = _EXPORTS[type(self), stem, form] = getattr(N.lib, "%s_%s" % (self._prefix, name))
        return fn

    def _two_tapes(self, a, b, scope, stem):
        """The two sides of one ``<prefix>_<stem>_prepared`` / ``<prefix>_[utf8_]<stem>_u64tape`` / ``..._u32tape`` call, the one place
        where two tapes become the head of a C call: both prepared (the first in the engine's mode), or neither; ``b`` None is a null
        pointer. Raw tapes go in one offset width (``_c_tapes``): u64, or u32 where both have it and the stem has that form
        (``N.U32_STEMS``). Returns ``call``: ``call(*tail, byref(err))`` passes the engine, the scope, the two sides and the C arguments
        ``tail``, keeps the tapes alive meanwhile and returns the status for ``N.check``.
        A search of 2048 x 2048 words takes ~100 us, so a prepared call is held to what the inline calls cost (0.3 us more, on a
        stub export): the export is looked up by name once per (engine type, stem, form), and ``call`` is a ``partial`` of the export
        itself -- no Python frame between the caller and the library."""
        if isinstance(a, PreparedTape) or isinstance(b, PreparedTape):
            if not isinstance(a, PreparedTape) or not (b is None or isinstance(b, PreparedTape)):
                raise TypeError("both tapes of a call must be prepared, or neither")
            self._need_mode(a)
            fn = _EXPORTS.get((type(self), stem, "prepared")) or self._export(stem, "prepared")
            return functools.partial(fn, self._handle, scope.handle, C.byref(a.view()), None if b is None else C.byref(b.view()))
        ta, tb, is64, kept = _c_tapes(a, b, u32=stem in N.U32_STEMS)
        form = "u64tape" if is64 else "u32tape"
        fn = _EXPORTS.get((type(self), stem, form)) or self._export(stem, form)
        call = functools.partial(fn, self._handle, scope.handle, C.byref(ta), None if tb is None else C.byref(tb))
        call.kept = kept   # (the structs hold bare pointers into these arrays; prepared tapes are the caller's own arguments)
        return call

    def _dense(self, stem, a, b, scope, out, dtype, extra=(), cross=False):
        """A call with one output: ``stem`` scores ``a[i]`` against ``b[i]`` into ``len(a)`` entries of ``dtype``, or with ``cross`` every
        ``a[i]`` against every ``b[j]`` (``b`` None: against ``a``) into a matrix of 64-bit entries. ``extra`` are the C arguments
        between the tapes and the output. ``out`` may be strided; the slots of a pairwise ``out`` may be wider than an entry (a
        column of a matrix, a uint64 array: the stride says so), which is why only a matrix is judged."""
        a = _as_tape(a)
        if cross:
            b = a if b is None else _as_tape(b)
            shape = (len(a), len(b))
        else:
            b = _as_tape(b)
            if len(a) != len(b):
                raise ValueError("pairwise scoring needs two collections of equal length")
            shape = (len(a),)
        if cross:
            _check_out(out, 8, shape=shape, strided=True)   # (before the tapes are judged, as top-k and extract do)
        call = self._two_tapes(a, b, scope, stem)
        if out is None:   # a dense product starts from zeros; every pair of a pairwise call is written, and a fresh array of a
            out = (np.zeros if cross else np.empty)(shape, dtype=dtype)   # million pairs is not filled twice
        err = C.c_char_p()
        N.check(call(*extra, C.c_void_p(_pointer(out)), _stride(out, cross), C.byref(err)), err)
        return out

    def cross_sharded(self, product: "ShardedCross", scope: DeviceScope, out=None):
        """The dense matrix of a sharded product: every device of the scope fills its rows and copies them into `out` (host
        memory or memory of the first device; 64-bit entries)."""
        if self._utf8 != product.utf8:
            raise ValueError("engine and sharded product disagree on UTF-8")
        if out is None:
            out = np.zeros(product.shape, dtype=np.uint64 if self._prefix == "swh_levenshtein" else np.int64)
        _check_out(out, 8, shape=product.shape, strided=True)
        row_stride = out.strides[0] if isinstance(out, np.ndarray) else product.shape[1] * 8
        err = C.c_char_p()
        status = getattr(N.lib, self._prefix + "_cross_sharded")(self._handle, scope.handle, product._handle, C.c_void_p(_pointer(out)), row_stride, C.byref(err))
        N.check(status, err)
        return out

    def bind_pairs(self, a: "PreparedTape", b: "PreparedTape", scope: DeviceScope, out, bound: Optional[int] = None):
        """A pre-bound pairwise call on prepared views: every ctypes argument is built once, the returned callable
        only crosses the FFI (what a compiled harness pays per call; `pairs()` re-derives views, pointers and strides
        in Python each time, ~10 us). `out` must stay alive and in place."""
        if not isinstance(a, PreparedTape) or not isinstance(b, PreparedTape) or len(a) != len(b):
            raise TypeError("bind_pairs takes two prepared views of equal length")
        if self._utf8 != a.utf8:
            raise ValueError("engine and tapes disagree on UTF-8")
        va, vb, err = a.view(), b.view(), C.c_char_p()
        fn = getattr(N.lib, self._prefix + "_pairs_prepared")
        extra = (_bound(bound),) if self._prefix == "swh_levenshtein" else ()
        args = (self._handle, scope.handle, C.byref(va), C.byref(vb), *extra, C.c_void_p(_pointer(out)),
                out.strides[0] if isinstance(out, np.ndarray) and out.size > 1 else 0, C.byref(err))
        keep = (va, vb, err, a, b, out)

        def call(_fn=fn, _args=args, _keep=keep):
            status = _fn(*_args)
            if status != N.SUCCESS:
                N.check(status, _keep[2])
        return call


class LevenshteinDistances(_Engine):
    """``szs.LevenshteinDistances`` / ``LevenshteinDistances::new(&scope, 0, 1, 1, 1)`` (bench.rs:382).

    ``engine(queries, candidates, scope, out=matrix)`` is the reference's dense cross-product
    (bench.py:421-422, bench.rs:478-486); ``engine.pairs(a, b, scope, bound=k)`` scores
    ``a[i]`` against ``b[i]`` and returns ``min(d, k+1)``.
    """

    def __init__(self, match: int = 0, mismatch: int = 1, open: int = 1, extend: int = 1, *,
                 capabilities: Optional[DeviceScope] = None, algorithm: str = "auto"):
        if capabilities is None:
            raise ValueError("capabilities=DeviceScope(gpu_device=...) is required: there is no default CPU scope")
        handle, err = C.c_void_p(), C.c_char_p()
        N.check(N.lib.swh_levenshtein_init(capabilities.handle, match, mismatch, open, extend, C.byref(handle), C.byref(err)), err)
        self._handle = handle
        self.set_algorithm(algorithm)

    def set_algorithm(self, algorithm: str) -> None:
        code = {"auto": N.ALGORITHM_AUTO, "wavefront": N.ALGORITHM_WAVEFRONT, "bitparallel": N.ALGORITHM_BITPARALLEL,
                "tiled": N.ALGORITHM_TILED}[algorithm]
        N.lib.swh_levenshtein_set_algorithm(self._handle, code)

    def __call__(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        _need_scope(scope)
        return self._dense("cross", queries, candidates, scope, out, np.uint64, cross=True)

    def pairs(self, a: TapeLike, b: TapeLike, scope: DeviceScope, bound: Optional[int] = None, out=None):
        return self._dense("pairs", a, b, scope, out, np.uint32, (_bound(bound),))

    def topk(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, *, k: int,
             bound: Optional[int] = None, out=None):
        """The ``k`` nearest candidates of every query: ``(indices, distances)``, each ``(len(queries), k)`` of uint32, rows ordered
        by distance and then by candidate index, only candidates with ``d <= bound``, short rows padded with ``0xFFFFFFFF``.
        ``candidates=None`` searches the queries themselves (diagonal included). ``out=(indices, distances)`` fills given arrays
        or device tensors (contiguous, ``len(queries) * k`` uint32 / int32 each) instead of returning new numpy arrays.
        Two prepared byte tapes must share one offset width: one prepared from uint32 and one from uint64 offsets raise
        ``StringWarsError('invalid_argument')`` and nothing is written.
        rapidfuzz: ``process.extract(q, candidates, scorer=Levenshtein.distance, limit=k, score_cutoff=bound)`` per query."""
        _need_scope(scope)
        queries = _as_tape(queries)
        if candidates is not None:
            candidates = _as_tape(candidates)
        count = len(queries)
        if out is None:
            indices, distances = np.empty((count, int(k)), dtype=np.uint32), np.empty((count, int(k)), dtype=np.uint32)
        else:
            indices, distances = out
            _check_out(indices, 4, count * int(k))
            _check_out(distances, 4, count * int(k))
        err = C.c_char_p()
        N.check(self._two_tapes(queries, candidates, scope, "topk")(int(k), _bound(bound), C.c_void_p(_pointer(indices)),
                                                                    C.c_void_p(_pointer(distances)), C.byref(err)), err)
        return indices, distances

    @staticmethod
    def _csr_search(call, count, others, out, capacity, value_dtype, result):
        """The capacity protocol of the two range searches (``within``, ``extract_within``). ``call(offsets, indices, values, room)``
        runs the search and returns the hit total; ``values`` are the distances (uint32) or the scores (float64). With ``out`` the
        given arrays or tensors are checked and filled (too small: the offsets are written, then ``ValueError``); without, the first
        call has room for ``capacity`` hits and a second is made with the exact size only if they did not fit."""
        if out is not None:
            offsets, indices, values = out
            room = 0 if indices is None else int(indices.numel() if hasattr(indices, "numel") else indices.size)
            _check_out(offsets, 8, count + 1)
            _check_out(indices, 4, room)
            _check_out(values, np.dtype(value_dtype).itemsize, room)
            if (indices is None) != (values is None):
                raise ValueError("out needs both arrays, or None for both (the counting call)")
            total = call(offsets, indices, values, room)
            if indices is None:
                return result(offsets, None, None)
            if total > room:
                raise ValueError("out holds %d hits, the search found %d (the offsets are written)" % (room, total))
            return result(offsets, indices[:total], values[:total])
        room = max(1024, 4 * (count + others)) if capacity is None else max(int(capacity), 1)
        offsets = np.zeros(count + 1, dtype=np.uint64)
        indices, values = np.empty(room, dtype=np.uint32), np.empty(room, dtype=value_dtype)
        total = call(offsets, indices, values, room)
        if total > room:
            indices, values = np.empty(total, dtype=np.uint32), np.empty(total, dtype=value_dtype)
            call(offsets, indices, values, total)
        return result(offsets, indices[:total], values[:total])

    def within(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, *, bound: int,
               capacity: Optional[int] = None, out=None) -> "RangeMatches":
        """Every candidate within ``bound`` edits of every query (``swh_levenshtein_within_*``): a :class:`RangeMatches`, rows in
        candidate order with the true distances. ``candidates=None`` searches the queries themselves (diagonal and both orientations
        included; ``pairs(upper=True)`` of the result is the deduplication form). Nobody knows the number of hits in advance: the
        first call is made with room for ``capacity`` hits (default ``max(1024, 4 * (len(queries) + len(candidates)))``) and, only
        if they did not fit, a second with the exact size the first one counted. ``out=(offsets, indices, distances)`` fills given
        arrays or device tensors instead (``len(queries) + 1`` 64-bit offsets; 32-bit indices and distances of equal size); if they
        are too small the offsets are still written and ``ValueError`` is raised; ``out=(offsets, None, None)`` is the counting
        call (one walk, the offsets alone). Tapes are handled as in ``topk``.
        rapidfuzz: ``process.extract(q, candidates, scorer=Levenshtein.distance, score_cutoff=bound, limit=None)`` per query."""
        _need_scope(scope)
        if bound is None or not 0 <= int(bound) < N.UNBOUNDED:
            raise ValueError("a range search needs a bound; the unbounded form is the dense cross-product")
        queries = _as_tape(queries)
        if candidates is not None:
            candidates = _as_tape(candidates)
        count = len(queries)
        search = self._two_tapes(queries, candidates, scope, "within")

        def call(offsets, indices, distances, room):
            err = C.c_char_p()
            N.check(search(C.c_uint32(int(bound)), C.c_void_p(_pointer(offsets)), C.c_void_p(_pointer(indices)), C.c_void_p(_pointer(distances)),
                           int(room), C.byref(err)), err)
            return int(offsets[count])

        return self._csr_search(call, count, len(candidates if candidates is not None else queries), out, capacity, np.uint32, RangeMatches)

    def align(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, bound: Optional[int] = None) -> "Alignments":
        """The edit operations of every pair ``(a[i], b[i])`` on unit costs (``swh_levenshtein_align_*``): an :class:`Alignments` with
        ``distances`` (``min(d, bound + 1)``, equal to ``pairs``), ``offsets`` and ``ops``. ``a`` and ``b`` are tapes, or both
        ``PreparedTape``s. The script of each pair is the library's canonical one among the optimal ones (see ``Alignments``);
        rapidfuzz: ``Levenshtein.editops(a[i], b[i])`` up to the choice among optimal scripts."""
        _need_scope(scope)
        a, b = self._promoted(a, b, scope, at=DeviceTape)
        if len(a) != len(b):
            raise ValueError("a and b must hold the same number of strings")
        count = len(a)
        distances = np.empty(count, dtype=np.uint32)
        offsets = np.zeros(count + 1, dtype=np.uint64)
        call = self._two_tapes(a, b, scope, "align")
        if isinstance(a, PreparedTape):
            self._need_mode(b)
            # the symbols of a sub-view are not known on the host: the whole tapes' bound the view's, and np.empty only reserves the
            # pages -- the call writes (and touches) the view's ops alone; a result much smaller than the buffer is copied out below
            capacity = a._root.info["symbols"] + b._root.info["symbols"]
        else:   # both are Strs: _promoted has prepared every DeviceTape, and widening the offsets for the call changes no value
            capacity = int(a.offsets[-1]) - int(a.offsets[0]) + int(b.offsets[-1]) - int(b.offsets[0]) if count else 0
        ops = np.empty(max(capacity, 1), dtype=np.uint8)
        err = C.c_char_p()
        N.check(call(_bound(bound), C.c_void_p(distances.ctypes.data), C.c_void_p(offsets.ctypes.data), C.c_void_p(ops.ctypes.data), capacity,
                     C.byref(err)), err)
        used = int(offsets[-1])
        return Alignments(distances, offsets, ops[:used].copy() if 2 * used < len(ops) else ops[:used])

    def infix(self, patterns: TapeLike, texts: TapeLike, scope: Optional[DeviceScope] = None, bound: Optional[int] = None) -> "InfixMatches":
        """Where, and how well, ``patterns[i]`` approximately occurs in ``texts[i]`` on unit costs (``swh_levenshtein_infix_*``): an
        :class:`InfixMatches` with ``distances``, ``starts`` and ``ends``. Patterns hold at most ``INFIX_MAX_PATTERN`` symbols. The two
        sides are tapes, or both ``PreparedTape``s. edlib: ``align(p, t, mode="HW", k=bound)`` (``editDistance``, ``locations[0]`` with an
        inclusive end); rapidfuzz: ``partial_ratio_alignment`` (``dest_start`` / ``dest_end``)."""
        _need_scope(scope)
        patterns, texts = self._promoted(patterns, texts, scope, at=DeviceTape)
        if len(patterns) != len(texts):
            raise ValueError("patterns and texts must hold the same number of strings")
        count = len(patterns)
        distances, starts, ends = (np.empty(count, dtype=np.uint32) for _ in range(3))
        call = self._two_tapes(patterns, texts, scope, "infix")
        if isinstance(patterns, PreparedTape):
            self._need_mode(texts)
        err = C.c_char_p()
        N.check(call(_bound(bound), *(C.c_void_p(array.ctypes.data) for array in (distances, starts, ends)), C.byref(err)), err)
        return InfixMatches(distances, starts, ends)

    _INFIX_SELECT = {"all": N.INFIX_SELECT_ALL, "best": N.INFIX_SELECT_BEST, "minima": N.INFIX_SELECT_MINIMA}

    def infix_all(self, patterns: TapeLike, texts: TapeLike, scope: Optional[DeviceScope] = None, *, bound: Optional[int] = None,
                  select: str = "all", starts: bool = True, capacity: Optional[int] = None, out=None) -> "InfixOccurrences":
        """EVERY end at which ``patterns[i]`` occurs in ``texts[i]`` within ``bound`` edits (``swh_levenshtein_infix_all_*``): an
        :class:`InfixOccurrences`, rows ascending by end with the true distances. ``select`` keeps every such end (``"all"``), those
        that reach the pair's best distance (``"best"``: edlib's ``locations``, ends inclusive there) or one per dip of the score
        curve (``"minima"``: the first column of every plateau that is a weak local minimum). ``bound=None`` is no cutoff.
        ``starts=False`` skips the start pass and leaves ``.starts`` None. The hit total is not known in advance: as in ``within``
        the first call has room for ``capacity`` hits (default ``max(1024, 8 * len(patterns))``) and a second is made with the exact
        size only if they did not fit. ``out=(offsets, starts, ends, distances)`` fills given arrays or device tensors instead
        (``starts`` None where ``starts=False``); ``out=(offsets, None, None, None)`` is the counting call (one walk). The two
        sides are tapes, or both ``PreparedTape``s."""
        _need_scope(scope)
        if select not in self._INFIX_SELECT:
            raise ValueError("select must be one of %s" % ", ".join(map(repr, self._INFIX_SELECT)))
        patterns, texts = self._promoted(patterns, texts, scope, at=DeviceTape)
        if len(patterns) != len(texts):
            raise ValueError("patterns and texts must hold the same number of strings")
        count = len(patterns)
        search = self._two_tapes(patterns, texts, scope, "infix_all")
        if isinstance(patterns, PreparedTape):
            self._need_mode(texts)
        held = [None]   # the starts that go with the (ends, distances) of the latest call

        if out is not None:
            offsets, held[0], ends, distances = out
            if bool(starts) != (held[0] is not None) and ends is not None:
                raise ValueError("out holds starts exactly where starts=True")
            if held[0] is not None:
                _check_out(held[0], 4, 0 if ends is None else int(ends.numel() if hasattr(ends, "numel") else ends.size))
            out = (offsets, ends, distances)

        def call(offsets, ends, distances, room):
            if out is None and starts:
                held[0] = np.empty(room, dtype=np.uint32)
            err = C.c_char_p()
            N.check(search(_bound(bound), C.c_uint32(self._INFIX_SELECT[select]), C.c_void_p(_pointer(offsets)), C.c_void_p(_pointer(held[0])),
                           C.c_void_p(_pointer(ends)), C.c_void_p(_pointer(distances)), int(room), C.byref(err)), err)
            return int(offsets[count])

        def result(offsets, ends, distances):
            return InfixOccurrences(offsets, None if held[0] is None or ends is None else held[0][:len(ends)], ends, distances)

        return self._csr_search(call, count, count, out, capacity, np.uint32, result)

    def osa(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, bound: Optional[int] = None, out=None):
        """Damerau-Levenshtein distances in the optimal-string-alignment (OSA, restricted) form of every pair ``(a[i], b[i])``
        (``swh_levenshtein_osa_pairs_*``): ``min(d, bound + 1)`` as uint32, where a swap of two neighbouring symbols costs one edit
        and no substring is edited twice (``ab`` / ``ba``: 1; ``ca`` / ``abc``: 3, not the 2 of unrestricted Damerau-Levenshtein).
        The shorter string of a pair holds at most ``OSA_MAX_SHORTER`` symbols. The two sides are tapes, or both ``PreparedTape``s.
        rapidfuzz: ``OSA.distance(a[i], b[i], score_cutoff=bound)``."""
        _need_scope(scope)
        a, b = self._promoted(a, b, scope, at=DeviceTape)
        return self._dense("osa_pairs", a, b, scope, out, np.uint32, (_bound(bound),))

    def osa_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        """The dense OSA matrix ``out[i][j] = osa(queries[i], candidates[j])`` as uint64 (``swh_levenshtein_osa_cross_*``), the shape of
        ``engine(queries, candidates, scope)``; ``candidates=None`` is the self-product (symmetric, zero diagonal).
        rapidfuzz: ``process.cdist(queries, candidates, scorer=OSA.distance)``."""
        _need_scope(scope)
        queries, candidates = self._promoted(queries, candidates, scope, at=DeviceTape)
        return self._dense("osa_cross", queries, candidates, scope, out, np.uint64, cross=True)

    def _scored_call(self, family, a, b, scope, cross, outs, extra=()):
        """One ``swh_levenshtein_{lcs,jaro}_*`` call. ``outs``: for each output of the family, in the order of its exports, the array
        to fill, True for a fresh one, None where that output is not wanted; ``extra``: the C arguments between the tapes and the
        outputs (the bound of the pairwise LCS calls). Returns the arrays (None where not wanted) and the two tapes as called."""
        _need_scope(scope)
        a = _as_tape(a)
        b = None if b is None else _as_tape(b)
        if b is None and not cross:
            raise ValueError("pairwise scoring needs two collections")
        if not cross and len(a) != len(b):
            raise ValueError("pairwise scoring needs two collections of equal length")
        a, b = self._promoted(a, b, scope, at=(DeviceTape, PreparedTape))
        if isinstance(a, PreparedTape):
            self._need_mode(a)   # (_two_tapes asks again below: here the refusal comes before those of the outputs, as it always did)
        shape = (len(a), len(a if b is None else b)) if cross else (len(a),)
        dtype = np.uint64 if cross else np.uint32
        outs = [np.zeros(shape, dtype=dtype) if out is True else out for out in outs]
        for out in outs:
            _check_out(out, dtype().itemsize, shape=shape, strided=True)
        strides = {_stride(out, cross) for out in outs if isinstance(out, np.ndarray)}
        if len(strides) > 1:
            raise ValueError("the outputs share one stride")
        stride = strides.pop() if strides else 0
        call = self._two_tapes(a, b, scope, "%s_%s" % (family, "cross" if cross else "pairs"))
        err = C.c_char_p()
        N.check(call(*extra, *(C.c_void_p(None if out is None else _pointer(out)) for out in outs), stride, C.byref(err)), err)
        return outs, a, (a if b is None else b)

    def _lcs_call(self, a, b, scope, cross, bound, indel, lcs):
        """The Indel distances and the LCS lengths of one ``swh_levenshtein_lcs_*`` call, each as ``_scored_call`` takes and returns it."""
        extra = () if cross else (_bound(bound),)
        return self._scored_call("lcs", a, b, scope, cross, (indel, lcs), extra)[0]

    @staticmethod
    def _ratio(indel, lcs):
        """``200 L / (d + 2 L)`` as float64, 100 where both strings are empty: rapidfuzz's ``fuzz.ratio``, unrounded."""
        twice = 2.0 * lcs.astype(np.float64)
        total = indel.astype(np.float64) + twice
        return np.where(total > 0, 100.0 * twice / np.where(total > 0, total, 1.0), 100.0)

    def lcs(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, out=None):
        """The length of the longest common subsequence of every pair ``(a[i], b[i])`` as uint32 (``swh_levenshtein_lcs_pairs_*``).
        The shorter string of a pair holds at most ``LCS_MAX_SHORTER`` symbols. The two sides are tapes, lists or ``PreparedTape``s.
        rapidfuzz: ``distance.LCSseq.similarity(a[i], b[i])``."""
        return self._lcs_call(a, b, scope, False, None, None, True if out is None else out)[1]

    def indel(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, bound: Optional[int] = None, out=None):
        """The Indel distance of every pair, ``min(len(a[i]) + len(b[i]) - 2 LCS, bound + 1)`` as uint32: the edits between the two
        strings when only insertions and deletions count (``kitten`` / ``sitting``: 5). rapidfuzz:
        ``distance.Indel.distance(a[i], b[i], score_cutoff=bound)``."""
        return self._lcs_call(a, b, scope, False, bound, True if out is None else out, None)[0]

    def ratio(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None):
        """rapidfuzz's ``fuzz.ratio(a[i], b[i])``, unrounded, as float64: ``100 (1 - indel / (m + n)) = 200 LCS / (m + n)``, and 100 for
        two empty strings -- from one unbounded call with both outputs."""
        return self._ratio(*self._lcs_call(a, b, scope, False, None, True, True))

    def lcs_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        """The dense matrix ``out[i][j] = LCS(queries[i], candidates[j])`` as uint64 (``swh_levenshtein_lcs_cross_*``);
        ``candidates=None`` is the self-product (symmetric, the diagonal holds the lengths)."""
        return self._lcs_call(queries, candidates, scope, True, None, None, True if out is None else out)[1]

    def indel_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        """The dense matrix of Indel distances as uint64; ``candidates=None`` is the self-product (symmetric, zero diagonal).
        rapidfuzz: ``process.cdist(queries, candidates, scorer=distance.Indel.distance)``."""
        return self._lcs_call(queries, candidates, scope, True, None, True if out is None else out, None)[0]

    def ratio_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None):
        """The dense float64 matrix of ``fuzz.ratio``: rapidfuzz's ``process.cdist(queries, candidates, scorer=fuzz.ratio)``, unrounded."""
        return self._ratio(*self._lcs_call(queries, candidates, scope, True, None, True, True))

    def partial_counts(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, out=None):
        """The counts behind the partial ratio of every pair ``(a[i], b[i])`` as four uint32 arrays (``swh_levenshtein_partial_pairs_*``):
        ``lcs``, ``starts``, ``ends`` and ``sides``. The shorter string is the needle (at most ``PARTIAL_MAX_NEEDLE`` symbols); ``lcs`` is
        its LCS length with the best window ``[starts, ends)`` of the other string -- the largest ``lcs / (m + end - start)``, compared
        exactly, the smallest offset among equals; ``sides`` is 0 where the window lies in ``b[i]``, 1 where it lies in ``a[i]``.
        ``out``: four arrays to fill, None where an output is not wanted (not all)."""
        return tuple(self._scored_call("partial", a, b, scope, False, (True,) * 4 if out is None else tuple(out))[0])

    def partial_counts_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        """The four dense uint64 matrices of counts, ``[i][j]`` of ``(queries[i], candidates[j])`` (``swh_levenshtein_partial_cross_*``);
        ``candidates=None`` is the self-product."""
        return tuple(self._scored_call("partial", queries, candidates, scope, True, (True,) * 4 if out is None else tuple(out))[0])

    @staticmethod
    def _partial_score(lcs, starts, ends, m, n):
        """``100 (2 L) / (m + (end - start))`` as float64, evaluated as ``_ratio`` does, ``m`` the needle's and ``n`` the haystack's
        symbols; an empty needle scores 100 against an empty haystack and 0 against any other."""
        twice = 2.0 * lcs.astype(np.float64)
        total = np.asarray(m, dtype=np.float64) + (ends.astype(np.float64) - starts.astype(np.float64))
        return np.where(total > 0, 100.0 * twice / np.where(total > 0, total, 1.0), np.where(np.asarray(n) == 0, 100.0, 0.0))

    def _partial(self, a, b, scope, cross):
        (lcs, starts, ends, sides), a, b = self._scored_call("partial", a, b, scope, cross, (True,) * 4)
        la, lb = _symbol_lengths(a, self._utf8, scope), _symbol_lengths(b, self._utf8, scope)
        if cross:
            la, lb = la[:, None], lb[None, :]
        la, lb = np.broadcast_to(la, lcs.shape), np.broadcast_to(lb, lcs.shape)
        score = self._partial_score(lcs, starts, ends, np.minimum(la, lb), np.maximum(la, lb))
        return score, starts, ends, sides, la, lb

    def partial_ratio(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None):
        """rapidfuzz's ``fuzz.partial_ratio(a[i], b[i])``, unrounded, as float64: the best ``fuzz.ratio`` of the shorter string against
        the windows of its own length of the longer one, the shorter windows at both ends included (``lawn`` in ``flaw in law``:
        85.71...); with equal lengths both directions are tried. From one call's counts (``partial_counts``)."""
        return self._partial(a, b, scope, False)[0]

    def partial_ratio_alignment(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None) -> "PartialAlignments":
        """rapidfuzz's ``fuzz.partial_ratio_alignment(a[i], b[i])`` for every pair, as a :class:`PartialAlignments`: the score and the
        two substrings it was reached between. rapidfuzz filters windows by character set first and may report a later window of the
        same score; the scores correspond."""
        score, starts, ends, sides, la, lb = self._partial(a, b, scope, False)
        in_b = sides == 0
        zero = np.zeros_like(starts)
        return PartialAlignments(score, np.where(in_b, zero, starts), np.where(in_b, la, ends), np.where(in_b, starts, zero), np.where(in_b, ends, lb))

    def partial_ratio_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None):
        """The dense float64 matrix of ``fuzz.partial_ratio``: rapidfuzz's ``process.cdist(queries, candidates,
        scorer=fuzz.partial_ratio)``, unrounded; ``candidates=None`` is the self-product."""
        return self._partial(queries, candidates, scope, True)[0]

    def _token_sorted(self, tape, scope, unique=False):
        """The token-sorted form of one side of a call, and whether the call owns it: a ``PreparedTape`` is derived from as it stands;
        anything else is prepared in the engine's mode, derived from and freed again."""
        _need_scope(scope)
        tape = _as_tape(tape)
        if isinstance(tape, PreparedTape):
            self._need_mode(tape)
            return tape.token_sorted(unique)
        prepared = PreparedTape(scope, tape, utf8=self._utf8)
        try:
            return prepared.token_sorted(unique)
        finally:
            prepared.free()

    def _on_token_sorted(self, call, a, b, scope):
        """``call(sorted a, sorted b, scope)`` on the ``SWH_TOKENS_SORTED`` forms of the two sides (``b`` None stays None); the derived
        tapes are freed when it returns."""
        derived = [self._token_sorted(a, scope)]
        try:
            derived.append(None if b is None else self._token_sorted(b, scope))
            return call(derived[0], derived[1], scope)
        finally:
            for tape in derived:
                if tape is not None:
                    tape.free()

    def token_sort_ratio(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None):
        """rapidfuzz's ``fuzz.token_sort_ratio(a[i], b[i])``, unrounded, as float64: ``ratio`` of the two strings with their tokens
        (``split()``) sorted and joined by one space -- ``new york mets`` / ``mets york new``: 100. The forms are derived on the device
        (``PreparedTape.token_sorted``); a string holds at most ``TOKEN_MAX_BYTES`` bytes. The two sides are tapes, lists, device
        tapes or ``PreparedTape``s; to score one collection many times, derive its tape once and call ``ratio``."""
        if b is None:
            raise ValueError("pairwise scoring needs two collections")
        return self._on_token_sorted(self.ratio, a, b, scope)

    def token_sort_ratio_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None):
        """The dense float64 matrix of ``fuzz.token_sort_ratio``: rapidfuzz's ``process.cdist(queries, candidates,
        scorer=fuzz.token_sort_ratio)``, unrounded; ``candidates=None`` is the self-product."""
        return self._on_token_sorted(self.ratio_cross, queries, candidates, scope)

    def token_set_counts(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, out=None):
        """The counts behind the token set ratio of every pair ``(a[i], b[i])`` as four uint32 arrays
        (``swh_levenshtein_token_set_pairs_*``): with A and B the sets of the two strings' tokens, the symbols ``s`` of the sorted,
        space-joined A & B, ``x`` of A - B and ``y`` of B - A, and the LCS length of the last two. The call derives the unique
        token-sorted forms itself; a ``PreparedTape`` from ``token_sorted(unique=True)`` is used as it stands. ``out``: four arrays
        to fill, None where an output is not wanted (not all)."""
        return tuple(self._scored_call("token_set", a, b, scope, False, (True,) * 4 if out is None else tuple(out))[0])

    @staticmethod
    def _token_set_score(s, x, y, lcs):
        """rapidfuzz's ``fuzz.token_set_ratio`` from the four counts, as float64. With ``q(d, t) = 100.0 * (t - d) / t`` (100 where
        ``t`` is 0), the expression ``_ratio`` evaluates for ``t = m + n``: 0 where a side has no token, 100 where one token set holds
        the other, else ``max(q(x + y - 2 L, sab + sba), q(e + x, s + sab), q(e + y, s + sba))`` with ``e = 1`` for the separator behind
        a non-empty intersection, ``sab = s + e + x`` and ``sba = s + e + y`` -- the first term alone where nothing is shared."""
        s, x, y, lcs = (np.asarray(v).astype(np.float64) for v in (s, x, y, lcs))   # (counts: every sum below is exact)
        e = (s > 0).astype(np.float64)
        sab, sba = s + e + x, s + e + y
        with np.errstate(divide="ignore", invalid="ignore"):   # (a zero total only where the result is decided without it)
            t = sab + sba
            r = 100.0 * (t - (x + y - 2.0 * lcs)) / t
            t = s + sab
            q_ab = 100.0 * (t - (e + x)) / t
            t = s + sba
            q_ba = 100.0 * (t - (e + y)) / t
        score = np.where(s == 0, r, np.maximum(r, np.maximum(q_ab, q_ba)))
        return np.where((x == 0) | (y == 0), np.where(s == 0, 0.0, 100.0), score)

    def token_set_ratio(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None):
        """rapidfuzz's ``fuzz.token_set_ratio(a[i], b[i])``, unrounded, as float64 -- ``mariners vs angels`` /
        ``los angeles angels of anaheim at seattle mariners``: 90.909... -- from one call's counts (``token_set_counts``)."""
        return self._token_set_score(*self.token_set_counts(a, b, scope))

    @staticmethod
    def _jaro(matches, transpositions, m, n):
        """``(M / m + M / n + (M - t) / M) / 3.0`` as float64, evaluated as written; 1.0 where both strings are empty, 0.0 where
        nothing matches. ``m`` / ``n`` broadcast against the counts."""
        M, t = matches.astype(np.float64), transpositions.astype(np.float64)
        m, n = np.broadcast_to(np.asarray(m, dtype=np.float64), M.shape), np.broadcast_to(np.asarray(n, dtype=np.float64), M.shape)
        some = M > 0
        one = np.ones_like(M)
        Ms, ms, ns = np.where(some, M, one), np.where(some, m, one), np.where(some, n, one)
        value = (Ms / ms + Ms / ns + (Ms - t) / Ms) / 3.0
        return np.where(some, value, np.where((m == 0) & (n == 0), 1.0, 0.0))

    @staticmethod
    def _winkler(jaro, prefix, prefix_weight):
        """``jaro + l * p * (1.0 - jaro)`` where ``jaro > 0.7``, else ``jaro``, evaluated as written."""
        return np.where(jaro > 0.7, jaro + prefix.astype(np.float64) * prefix_weight * (1.0 - jaro), jaro)

    def _jaro_similarity(self, a, b, scope, cross, prefix_weight):
        if prefix_weight is not None:
            prefix_weight = float(prefix_weight)
            if not 0.0 <= prefix_weight <= 0.25:
                raise ValueError("prefix_weight must lie in [0, 0.25]")
        (matches, transpositions, prefix), a, b = self._scored_call("jaro", a, b, scope, cross, (True, True, None if prefix_weight is None else True))
        m, n = _symbol_lengths(a, self._utf8, scope), _symbol_lengths(b, self._utf8, scope)
        jaro = self._jaro(matches, transpositions, m[:, None] if cross else m, n[None, :] if cross else n)
        return jaro if prefix_weight is None else self._winkler(jaro, prefix, prefix_weight)

    def jaro_counts(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, out=None):
        """The counts behind the Jaro similarity of every pair ``(a[i], b[i])`` as three uint32 arrays (``swh_levenshtein_jaro_pairs_*``):
        the matches M, the transpositions t and the common prefix of at most four symbols. ``a[i]`` drives the matching and ``b[i]``
        is flagged; neither string holds more than ``JARO_MAX_LENGTH`` symbols. ``out``: a triple of arrays to fill, None where an
        output is not wanted (not all). The two sides are tapes, lists, device tapes or ``PreparedTape``s."""
        return tuple(self._scored_call("jaro", a, b, scope, False, (True, True, True) if out is None else tuple(out))[0])

    def jaro_counts_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        """The three dense uint64 matrices of counts, ``[i][j]`` of ``(queries[i], candidates[j])`` (``swh_levenshtein_jaro_cross_*``);
        ``candidates=None`` is the self-product (the diagonal holds M = len, t = 0, prefix = min(len, 4))."""
        return tuple(self._scored_call("jaro", queries, candidates, scope, True, (True, True, True) if out is None else tuple(out))[0])

    def jaro(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None):
        """The Jaro similarity of every pair as float64: ``(M / m + M / n + (M - t) / M) / 3``, 1 for two empty strings, 0 where nothing
        matches (``MARTHA`` / ``MARHTA``: 0.9444...) -- from one call's counts. rapidfuzz: ``distance.Jaro.similarity(a[i], b[i])``."""
        return self._jaro_similarity(a, b, scope, False, None)

    def jaro_winkler(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, prefix_weight: float = 0.1):
        """The Jaro-Winkler similarity of every pair as float64: ``jaro + l p (1 - jaro)`` where ``jaro > 0.7``, ``l`` the common prefix of
        at most four symbols and ``p = prefix_weight`` in [0, 0.25] (``MARTHA`` / ``MARHTA``: 0.9611...). rapidfuzz:
        ``distance.JaroWinkler.similarity(a[i], b[i], prefix_weight=p)``."""
        return self._jaro_similarity(a, b, scope, False, prefix_weight)

    def jaro_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None):
        """The dense float64 matrix of Jaro similarities: rapidfuzz's ``process.cdist(queries, candidates, scorer=distance.Jaro.similarity)``."""
        return self._jaro_similarity(queries, candidates, scope, True, None)

    def jaro_winkler_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None,
                           prefix_weight: float = 0.1):
        """The dense float64 matrix of Jaro-Winkler similarities."""
        return self._jaro_similarity(queries, candidates, scope, True, prefix_weight)

    def extract(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, *, scorer: str, k: int,
                cutoff: Optional[float] = None, prefix_weight: float = 0.1, out=None):
        """The ``k`` best candidates of every query under ``scorer`` (``swh_levenshtein_extract_*``): ``(indices, scores)``, each
        ``(len(queries), k)``, uint32 and float64. ``scorer`` is one of ``SCORERS``: ``"osa"`` and ``"indel"`` are distances (smaller is
        better, ``d <= cutoff`` is admitted), ``"lcs"``, ``"ratio"``, ``"jaro"`` and ``"jaro_winkler"`` similarities (larger is better,
        ``s >= cutoff``); ``cutoff=None`` admits everything. Rows are ordered best score first, equal float64 scores by the smaller
        candidate index; a row with fewer than ``k`` admitted candidates is padded with index ``0xFFFFFFFF`` and a NaN whose 64 bits
        are all ones. A score has the bits that ``osa``, ``indel``, ``lcs``, ``ratio``, ``jaro`` and ``jaro_winkler`` (with this
        ``prefix_weight``, in [0, 0.25]) return for that pair. ``candidates=None`` searches the queries themselves (diagonal included).
        ``out=(indices, scores)`` fills given arrays or device tensors (contiguous, ``len(queries) * k`` entries of 4 and 8 bytes).
        The two sides are tapes, or both ``PreparedTape``s.
        rapidfuzz: ``process.extract(q, candidates, scorer=fuzz.ratio, limit=k, score_cutoff=cutoff)`` per query."""
        _need_scope(scope)
        if scorer not in N.SCORERS:
            raise ValueError("scorer must be one of %s" % ", ".join(N.SCORERS))
        queries = _as_tape(queries)
        if candidates is not None:
            candidates = _as_tape(candidates)
        count = len(queries)
        if out is None:
            indices, scores = np.empty((count, int(k)), dtype=np.uint32), np.empty((count, int(k)), dtype=np.float64)
        else:
            indices, scores = out
            _check_out(indices, 4, count * int(k))
            _check_out(scores, 8, count * int(k))
        if cutoff is None:
            cutoff = 0.0 if N.SCORERS[scorer] >= N.SCORERS["lcs"] else float("inf")
        bits = _double_bits(cutoff), _double_bits(prefix_weight)
        err = C.c_char_p()
        N.check(self._two_tapes(queries, candidates, scope, "extract")(N.SCORERS[scorer], int(k), bits[0], bits[1], C.c_void_p(_pointer(indices)),
                                                                       C.c_void_p(_pointer(scores)), C.byref(err)), err)
        return indices, scores

    def extract_within(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, *, scorer: str,
                       cutoff: float, prefix_weight: float = 0.1, capacity: Optional[int] = None, out=None) -> "ScoreMatches":
        """Every candidate of every query whose score under ``scorer`` passes ``cutoff`` (``swh_levenshtein_extract_within_*``): a
        :class:`ScoreMatches`, rows in candidate order. Scorers, scores and admission are those of ``extract`` -- ``"osa"`` and
        ``"indel"`` admit ``d <= cutoff`` (a finite cutoff: ``inf`` would be the dense cross-product), ``"lcs"``, ``"ratio"``,
        ``"jaro"`` and ``"jaro_winkler"`` admit ``s >= cutoff``, a score at the cutoff is admitted, and a score has the bits
        ``extract`` returns for that pair. ``candidates=None`` searches the queries themselves (diagonal and both orientations
        included; ``pairs(upper=True)`` of the result is the deduplication form). Capacity and ``out=`` work as in ``within``: the
        first call is made with room for ``capacity`` hits (default ``max(1024, 4 * (len(queries) + len(candidates)))``) and, only if
        they did not fit, a second with the exact size the first one counted; ``out=(offsets, indices, scores)`` fills given arrays
        or device tensors instead (``len(queries) + 1`` 64-bit offsets; 32-bit indices and 64-bit scores of equal size); if they are
        too small the offsets are still written and ``ValueError`` is raised; ``out=(offsets, None, None)`` is the counting call.
        A filled call scores the pairs twice (once to count, once to fill), a counting call once.
        rapidfuzz: ``process.extract(q, candidates, scorer=fuzz.ratio, score_cutoff=cutoff, limit=None)`` per query."""
        _need_scope(scope)
        if scorer not in N.SCORERS:
            raise ValueError("scorer must be one of %s" % ", ".join(N.SCORERS))
        if cutoff is None:
            raise ValueError("a range search needs a cutoff; without one it is the dense cross-product")
        queries = _as_tape(queries)
        if candidates is not None:
            candidates = _as_tape(candidates)
        count = len(queries)
        search = self._two_tapes(queries, candidates, scope, "extract_within")
        bits = _double_bits(cutoff), _double_bits(prefix_weight)

        def call(offsets, indices, scores, room):
            err = C.c_char_p()
            N.check(search(N.SCORERS[scorer], bits[0], bits[1], C.c_void_p(_pointer(offsets)), C.c_void_p(_pointer(indices)),
                           C.c_void_p(_pointer(scores)), int(room), C.byref(err)), err)
            return int(offsets[count])

        return self._csr_search(call, count, len(candidates if candidates is not None else queries), out, capacity, np.float64, ScoreMatches)

    def pairs_sharded(self, batch: "ShardedPairs", scope: DeviceScope, bound: Optional[int] = None, out=None):
        """One batch over every GPU of a multi-device scope; the distances come back gathered, in pair order."""
        if self._utf8 != batch.utf8:
            raise ValueError("engine and sharded batch disagree on UTF-8")
        if out is None:
            out = np.zeros(batch.count, dtype=np.uint32)
        err = C.c_char_p()
        status = N.lib.swh_levenshtein_pairs_sharded(self._handle, scope.handle, batch._handle,
                                                     _bound(bound), C.c_void_p(_pointer(out)), C.byref(err))
        N.check(status, err)
        return out


class LevenshteinDistancesUTF8(LevenshteinDistances):
    """``szs.LevenshteinDistancesUTF8`` / ``LevenshteinDistancesUtf8`` (bench.rs:386-399): symbols are
    Unicode scalar values; invalid UTF-8 raises ``StringWarsError('invalid_utf8')``."""

    _utf8 = True


class NeedlemanWunschScores(_Engine):
    """``szs.NeedlemanWunschScores(byte_to_class, class_costs, open=, extend=, capabilities=)``
    (bench.py:466-472, bench.rs:658-662). ``substitution_matrix=`` takes a full 256x256 int8 table
    instead (config C4). gap(k) = open + (k-1)*extend."""

    _prefix, _free = "swh_nw", "swh_nw_free"

    def __init__(self, byte_to_class: Optional[np.ndarray] = None, class_costs: Optional[np.ndarray] = None, *,
                 open: int = -2, extend: int = -2, capabilities: Optional[DeviceScope] = None,
                 substitution_matrix: Optional[np.ndarray] = None):
        if capabilities is None:
            raise ValueError("capabilities=DeviceScope(gpu_device=...) is required")
        handle, err = C.c_void_p(), C.c_char_p()
        if substitution_matrix is not None:
            matrix = np.ascontiguousarray(substitution_matrix, dtype=np.int8)
            if matrix.shape != (256, 256):
                raise ValueError("substitution_matrix must be 256x256 int8")
            status = getattr(N.lib, self._prefix + "_init")(capabilities.handle, matrix.ctypes.data, open, extend, C.byref(handle), C.byref(err))
        else:
            classes = np.ascontiguousarray(byte_to_class, dtype=np.uint8)
            costs = np.ascontiguousarray(class_costs, dtype=np.int8)
            if classes.shape != (256,) or costs.shape != (32, 32):
                raise ValueError("byte_to_class must have 256 entries and class_costs must be 32x32")
            status = getattr(N.lib, self._prefix + "_init_classes")(capabilities.handle, classes.ctypes.data, costs.ctypes.data,
                                                                   open, extend, C.byref(handle), C.byref(err))
        N.check(status, err)
        self._handle = handle

    def __call__(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        _need_scope(scope)
        return self._dense("cross", queries, candidates, scope, out, np.int64, cross=True)

    def pairs(self, a: TapeLike, b: TapeLike, scope: DeviceScope, out=None):
        return self._dense("pairs", a, b, scope, out, np.int32)

    def pairs_sharded(self, batch: "ShardedPairs", scope: DeviceScope, out=None):
        """One batch over every GPU of a multi-device scope (the matrix is cloned to every device on first use); the scores
        come back gathered, in pair order."""
        if batch.utf8:
            raise ValueError("alignment engines score bytes: the sharded batch was prepared as UTF-8")
        if out is None:
            out = np.zeros(batch.count, dtype=np.int32)
        err = C.c_char_p()
        status = getattr(N.lib, self._prefix + "_pairs_sharded")(self._handle, scope.handle, batch._handle, C.c_void_p(_pointer(out)), C.byref(err))
        N.check(status, err)
        return out


class SmithWatermanScores(NeedlemanWunschScores):
    """``szs.SmithWatermanScores`` (bench.py:789, bench.rs:882-963): local alignment score, same arguments."""

    _prefix, _free = "swh_sw", "swh_sw_free"


def edit_distance(column_a: TapeLike, column_b: TapeLike, scope: DeviceScope, utf8: bool = True,
                  bound: Optional[int] = None) -> np.ndarray:
    """Element-wise edit distance of two equal-length string columns, the call shape of
    ``cudf.Series.str.edit_distance(other)`` (similarities/bench.py:602)."""
    engine = (LevenshteinDistancesUTF8 if utf8 else LevenshteinDistances)(capabilities=scope)
    return engine.pairs(column_a, column_b, scope, bound=bound)
