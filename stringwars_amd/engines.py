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
from typing import Iterable, Optional, Sequence, Union

import numpy as np

from . import _native as N

__all__ = [
    "DeviceScope", "Strs", "DeviceTape", "PreparedTape", "ShardedPairs", "shard_cuts", "LevenshteinDistances", "LevenshteinDistancesUTF8",
    "NeedlemanWunschScores", "SmithWatermanScores", "edit_distance", "StringWarsError", "UNBOUNDED", "TOPK_MAX",
    "ALIGN_MAX_CELLS", "Alignments", "RangeMatches", "ScoreMatches", "INFIX_MAX_PATTERN", "INFIX_NONE", "InfixMatches", "OSA_MAX_SHORTER", "LCS_MAX_SHORTER", "PARTIAL_MAX_NEEDLE", "PartialAlignments",
    "JARO_MAX_LENGTH", "SCORERS",
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
SCORERS = tuple(N.SCORERS)   # the scorers of ``engine.extract``, by name


def _pointer(obj) -> int:
    """Raw address of a numpy array, torch tensor, ctypes pointer or int."""
    if obj is None:
        return 0
    if isinstance(obj, int):
        return obj
    if isinstance(obj, np.ndarray):
        return obj.ctypes.data
    if hasattr(obj, "data_ptr"):  # torch.Tensor
        return int(obj.data_ptr())
    if hasattr(obj, "value"):
        return int(obj.value or 0)
    raise TypeError(f"cannot take the address of {type(obj)!r}")


class DeviceScope:
    """``szs.DeviceScope(gpu_device=0)`` / ``DeviceScope::gpu_device(0)`` (bench.rs:379).

    ``cpu_cores=`` scopes are refused: this backend has no CPU path and says so loudly
    (the reference prints ``SKIPPED (<reason>)`` for a variant whose scope cannot be built).
    ``stream`` may be a raw ``hipStream_t`` address (e.g. ``torch.cuda.current_stream().cuda_stream``).
    """

    def __init__(self, gpu_device: Optional[int] = None, cpu_cores: Optional[int] = None, stream: Optional[int] = None,
                 gpu_devices: Optional[Sequence[int]] = None):
        handle = C.c_void_p()
        err = C.c_char_p()
        if gpu_devices is not None:
            # several GPUs of one node behind one scope (`swh_scope_init_gpus`): batches are split over them by the
            # `*_sharded` calls, distances gathered with RCCL inside the library
            devices = (C.c_int * len(gpu_devices))(*[int(d) for d in gpu_devices])
            status = N.lib.swh_scope_init_gpus(devices, len(gpu_devices), C.byref(handle), C.byref(err))
            gpu_device = gpu_devices[0] if len(gpu_devices) else 0
        elif cpu_cores is not None and gpu_device is None:
            status = N.lib.swh_scope_init_cpu(int(cpu_cores), C.byref(handle), C.byref(err))
        elif stream is not None:
            status = N.lib.swh_scope_init_gpu_stream(int(gpu_device or 0), C.c_void_p(int(stream)), C.byref(handle), C.byref(err))
        else:
            status = N.lib.swh_scope_init_gpu(int(gpu_device or 0), C.byref(handle), C.byref(err))
        N.check(status, err)
        self._handle = handle
        self.gpu_device = int(gpu_device or 0)

    @property
    def handle(self) -> C.c_void_p:
        return self._handle

    @property
    def compute_units(self) -> int:
        value = C.c_size_t()
        N.lib.swh_scope_compute_units(self._handle, C.byref(value))
        return int(value.value)

    @property
    def device_count(self) -> int:
        value = C.c_size_t()
        N.lib.swh_scope_device_count(self._handle, C.byref(value))
        return int(value.value)

    def shard_timing(self) -> dict:
        timing = N.ShardTiming()
        N.lib.swh_scope_shard_timing(self._handle, C.byref(timing))
        return {"compute_ms": timing.compute_ms, "gather_ms": timing.gather_ms, "cells": int(timing.cells), "pairs": int(timing.pairs)}

    def set_async(self, enabled: bool) -> None:
        N.lib.swh_scope_set_async(self._handle, int(bool(enabled)))

    def set_pipelined(self, enabled: bool) -> None:
        """Alternate calls between two internal lanes so the next call's planning overlaps this call's DP kernel;
        consumers ordered on the scope's stream call ``join()`` first, everyone else ``synchronize()``."""
        err = C.c_char_p()
        N.check(N.lib.swh_scope_set_pipelined(self._handle, int(bool(enabled)), C.byref(err)), err)

    def join(self) -> None:
        err = C.c_char_p()
        N.check(N.lib.swh_scope_join(self._handle, C.byref(err)), err)

    def forget(self) -> None:
        """Drops everything the scope believes about earlier calls (``swh_scope_forget``): the next call is routed as on a new scope."""
        N.lib.swh_scope_forget(self._handle)

    def describe(self) -> dict:
        """The scope's beliefs (``swh_scope_describe``) as a dict of strings."""
        text = C.create_string_buffer(512)
        N.lib.swh_scope_describe(self._handle, text, len(text))
        return dict(item.split("=", 1) for item in text.value.decode().split())

    def set_profiling(self, enabled: bool) -> None:
        N.lib.swh_scope_set_profiling(self._handle, int(bool(enabled)))

    def synchronize(self) -> None:
        err = C.c_char_p()
        N.check(N.lib.swh_scope_synchronize(self._handle, C.byref(err)), err)

    def last_timing(self) -> dict:
        timing = N.Timing()
        N.lib.swh_scope_last_timing(self._handle, C.byref(timing))
        return {
            "total_ms": timing.total_ms, "dominant_ms": timing.dominant_ms, "compute_ms": timing.compute_ms,
            "dominant_name": timing.dominant_name.decode(), "cells": int(timing.cells),
            "bytes": int(timing.bytes), "kernels": int(timing.kernels),
        }


    def timing_totals(self) -> dict:
        """Sums of ``last_timing``'s durations over every call since profiling was switched on, including
        asynchronous / pipelined calls (``swh_scope_timing_totals``)."""
        totals = N.TimingTotals()
        N.lib.swh_scope_timing_totals(self._handle, C.byref(totals))
        return {"total_ms": totals.total_ms, "dominant_ms": totals.dominant_ms, "compute_ms": totals.compute_ms,
                "calls": int(totals.calls)}

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle:
            N.lib.swh_scope_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Strs:
    """Arrow-style string tape on the host: ``sz.Strs(list)`` (bench.py:399), ``BytesTape<u64>``
    (bench.rs:292). ``offsets`` has ``count + 1`` entries of dtype uint64 or uint32."""

    def __init__(self, items: Union[Iterable[Union[bytes, str]], None] = None, *, data: Optional[np.ndarray] = None,
                 offsets: Optional[np.ndarray] = None):
        if items is not None:
            encoded = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in items]
            lengths = np.fromiter((len(s) for s in encoded), dtype=np.uint64, count=len(encoded))
            offsets = np.zeros(len(encoded) + 1, dtype=np.uint64)
            np.cumsum(lengths, out=offsets[1:])
            data = np.frombuffer(b"".join(encoded), dtype=np.uint8).copy() if encoded else np.zeros(0, np.uint8)
        if data is None or offsets is None:
            raise ValueError("Strs needs either items or data+offsets")
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets)
        self.count = len(self.offsets) - 1

    def __len__(self) -> int:
        return self.count

    def __getitem__(self, index):
        if isinstance(index, slice):
            start, stop, step = index.indices(self.count)
            if step != 1:
                raise ValueError("only contiguous sub-views")
            return self.subview(start, stop)
        lo, hi = int(self.offsets[index]), int(self.offsets[index + 1])
        return self.data[lo:hi].tobytes()

    def subview(self, start: int, stop: int) -> "Strs":
        """Zero-copy sub-range, ``BytesTapeView::subview(lo, hi)`` (bench.rs:134-139)."""
        return Strs(data=self.data, offsets=self.offsets[start:stop + 1])

    def with_offsets(self, dtype) -> "Strs":
        return Strs(data=self.data, offsets=self.offsets.astype(dtype))

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets.astype(np.int64))

    def to_device(self, scope: DeviceScope) -> "DeviceTape":
        return DeviceTape.upload(scope, self)


class DeviceTape:
    """A tape whose data and offsets are device pointers (hipMalloc or torch CUDA tensors)."""

    def __init__(self, data_ptr: int, offsets_ptr: int, count: int, offsets_dtype, keepalive=None, scope=None, owned=False):
        self.data_ptr, self.offsets_ptr, self.count = int(data_ptr), int(offsets_ptr), int(count)
        self.offsets_dtype = np.dtype(offsets_dtype)
        self._keepalive, self._scope, self._owned = keepalive, scope, owned

    @classmethod
    def upload(cls, scope: DeviceScope, strs: Strs) -> "DeviceTape":
        err = C.c_char_p()
        pointers = []
        for array in (strs.data, strs.offsets):
            pointer = C.c_void_p()
            N.check(N.lib.swh_device_alloc(scope.handle, array.nbytes + 16, C.byref(pointer), C.byref(err)), err)
            if array.nbytes:
                N.check(N.lib.swh_copy_to_device(scope.handle, pointer, array.ctypes.data, array.nbytes, C.byref(err)), err)
            pointers.append(pointer)
        # a sub-view's offsets index into the full data buffer, which was uploaded whole
        return cls(pointers[0].value, pointers[1].value, strs.count, strs.offsets.dtype, scope=scope, owned=True)

    @classmethod
    def from_torch(cls, data, offsets) -> "DeviceTape":
        import torch
        dtype = {torch.int32: np.uint32, torch.int64: np.uint64, torch.uint8: None}.get(offsets.dtype)
        if hasattr(torch, "uint32"):
            dtype = {torch.uint32: np.uint32, torch.uint64: np.uint64}.get(offsets.dtype, dtype)
        if dtype is None:
            raise TypeError("offsets tensor must be (u)int32 or (u)int64")
        return cls(data.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, dtype, keepalive=(data, offsets))

    def __len__(self) -> int:
        return self.count

    def free(self) -> None:
        if self._owned and self._scope is not None and self._scope.handle:
            N.lib.swh_device_free(self._scope.handle, C.c_void_p(self.data_ptr))
            N.lib.swh_device_free(self._scope.handle, C.c_void_p(self.offsets_ptr))
        self._owned = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PreparedTape:
    """A tape made ready once (``swh_tape_prepare_*``): resident on the scope's device, measured, and -- with
    ``utf8=True`` -- validated and decoded to code points. The counterpart of the ``BytesTapeView`` / ``CharsTapeView`` the
    reference builds once outside its timed closures (bench.rs:292-306; ``try_into`` is where invalid UTF-8 surfaces, and
    so it does here: ``StringWarsError('invalid_utf8')`` from the constructor). Slicing gives zero-copy sub-views
    (``subview(lo, hi)``, bench.rs:134-139). Engines take prepared tapes wherever they take tapes; both sides of a call
    must then be prepared, and in the same mode."""

    def __init__(self, scope: DeviceScope, tape, utf8: bool = False, _parent: Optional["PreparedTape"] = None,
                 first: int = 0, count: Optional[int] = None):
        if _parent is not None:
            self._handle, self._root, self.utf8 = _parent._handle, _parent._root, _parent.utf8
            self.first, self.count = first, count
            return
        tape = _as_tape(tape)
        struct, is64, keep = _c_tape(tape)
        handle, err = C.c_void_p(), C.c_char_p()
        fn = N.lib.swh_tape_prepare_u64 if is64 else N.lib.swh_tape_prepare_u32
        N.check(fn(scope.handle, C.byref(struct), int(bool(utf8)), C.byref(handle), C.byref(err)), err)
        self._handle, self._root, self.utf8 = handle, self, bool(utf8)
        self._keepalive = keep if isinstance(keep, DeviceTape) else None   # device tapes are used in place
        self._source, self._lengths = tape, None   # what symbol_lengths measures, once
        self.first, self.count = 0, len(tape)

    def __len__(self) -> int:
        return self.count

    @property
    def info(self) -> dict:
        info = N.PreparedInfo()
        N.lib.swh_prepared_info(self._handle, C.byref(info))
        return {"count": int(info.count), "bytes": int(info.bytes), "symbols": int(info.symbols), "longest": int(info.longest),
                "utf8": bool(info.utf8), "ascii": bool(info.ascii)}

    def subview(self, start: int, stop: int) -> "PreparedTape":
        if not 0 <= start <= stop <= self.count:
            raise IndexError("sub-view outside the tape")
        return PreparedTape(None, None, _parent=self, first=self.first + start, count=stop - start)

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("prepared tapes are sliced, not indexed")
        start, stop, step = index.indices(self.count)
        if step != 1:
            raise ValueError("only contiguous sub-views")
        return self.subview(start, max(start, stop))

    def view(self) -> "N.PreparedView":
        return N.PreparedView(self._handle, self.first, self.count)

    def symbol_lengths(self, scope: DeviceScope) -> np.ndarray:
        """Symbols (bytes, or code points of a ``utf8=True`` tape) of every string of this view, as int64, on the host."""
        root = self._root
        if root._lengths is None:
            root._lengths = _symbol_lengths(root._source, root.utf8, scope)
        return root._lengths[self.first:self.first + self.count]

    def free(self) -> None:
        if self._root is self and getattr(self, "_handle", None) and getattr(N, "lib", None) is not None:
            N.lib.swh_prepared_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def shard_cuts(a: Strs, b: Strs, shards: int) -> list:
    """Cells-balanced contiguous cuts of a pairwise batch (`swh_shard_cuts_*`): shard r = pairs [cuts[r], cuts[r+1])."""
    ta, a64, keep_a = _c_tape(a)
    tb, b64, keep_b = _c_tape(b, want64=a64 or None)
    if a64 != b64:
        ta, a64, keep_a = _c_tape(a, want64=True)
        tb, b64, keep_b = _c_tape(b, want64=True)
    cuts = (C.c_size_t * (shards + 1))()
    (N.lib.swh_shard_cuts_u64tape if a64 else N.lib.swh_shard_cuts_u32tape)(C.byref(ta), C.byref(tb), shards, cuts)
    return [int(c) for c in cuts]


class ShardedPairs:
    """A pairwise batch made resident on every device of a multi-GPU scope (`swh_sharded_prepare_*`): contiguous
    cells-balanced shards, shard r uploaded to and prepared on device r. The steady state of the `<Ngpu>` rows:
    ``engine.pairs_sharded(batch, scope)`` scores all shards and gathers the distances with RCCL."""

    def __init__(self, scope: DeviceScope, a: Strs, b: Strs, utf8: bool = False):
        if not isinstance(a, Strs) or not isinstance(b, Strs):
            raise TypeError("sharding reads host tapes (Strs)")
        ta, a64, keep_a = _c_tape(a)
        tb, b64, keep_b = _c_tape(b, want64=a64 or None)
        if a64 != b64:
            ta, a64, keep_a = _c_tape(a, want64=True)
            tb, b64, keep_b = _c_tape(b, want64=True)
        handle, err = C.c_void_p(), C.c_char_p()
        fn = N.lib.swh_sharded_prepare_u64tape if a64 else N.lib.swh_sharded_prepare_u32tape
        N.check(fn(scope.handle, C.byref(ta), C.byref(tb), int(bool(utf8)), C.byref(handle), C.byref(err)), err)
        self._handle, self.count, self.utf8, self._scope = handle, len(a), bool(utf8), scope

    @property
    def cuts(self) -> list:
        n = self._scope.device_count + 1
        cuts = (C.c_size_t * n)()
        N.lib.swh_sharded_cuts(self._handle, cuts, n)
        return [int(c) for c in cuts]

    def free(self) -> None:
        if getattr(self, "_handle", None) and getattr(N, "lib", None) is not None:
            N.lib.swh_sharded_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ShardedCross:
    """A dense queries x candidates product made resident on every device of a multi-GPU scope
    (`swh_sharded_cross_prepare_u64tape`): row blocks of equal query symbols, block r and all candidates prepared on device
    r. ``engine.cross_sharded(product, scope, out=matrix)`` is the `<Ngpu>` twin of the reference's `compute_into`."""

    def __init__(self, scope: DeviceScope, queries: Strs, candidates: Strs, utf8: bool = False):
        if not isinstance(queries, Strs) or not isinstance(candidates, Strs):
            raise TypeError("sharding reads host tapes (Strs)")
        tq, _, keep_q = _c_tape(queries, want64=True)
        tc, _, keep_c = _c_tape(candidates, want64=True)
        handle, err = C.c_void_p(), C.c_char_p()
        N.check(N.lib.swh_sharded_cross_prepare_u64tape(scope.handle, C.byref(tq), C.byref(tc), int(bool(utf8)), C.byref(handle), C.byref(err)), err)
        self._handle, self.shape, self.utf8, self._scope = handle, (len(queries), len(candidates)), bool(utf8), scope

    def free(self) -> None:
        if getattr(self, "_handle", None) and getattr(N, "lib", None) is not None:
            N.lib.swh_sharded_cross_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


TapeLike = Union[Strs, DeviceTape, PreparedTape, Sequence[Union[bytes, str]]]


class RangeMatches:
    """The result of ``LevenshteinDistances.within``: for every query the candidates within the bound, as CSR.

    Row ``i`` is ``indices[offsets[i]:offsets[i + 1]]`` with the true distances in ``distances`` at the same places, ascending by
    candidate index (callers who want them by distance sort a row, or use ``topk``). ``offsets`` is uint64 with one entry more than
    there are queries. Arrays that live on the device (``out=`` tensors) are brought to the host when a row or the pairs are asked for.
    The result of a counting call (``out=(offsets, None, None)``) has ``offsets`` and ``counts`` only: ``indices`` and ``distances`` are None."""

    def __init__(self, offsets, indices, distances):
        self.offsets, self.indices, self.distances = offsets, indices, distances
        if len(offsets) < 1 or (indices is None) != (distances is None) or (indices is not None and len(indices) != len(distances)):
            raise ValueError("offsets needs at least one entry, indices and distances the same length (or both None: counted, not filled)")

    @staticmethod
    def _host(array, dtype):
        if hasattr(array, "cpu"):   # torch.Tensor
            array = array.cpu().numpy()
        array = np.asarray(array)   # (a signed tensor of the same width holds the same bits: torch has no uint64 arithmetic)
        return array.view(dtype) if array.dtype.itemsize == np.dtype(dtype).itemsize else array.astype(dtype)

    def __len__(self) -> int:
        """The number of queries (rows)."""
        return len(self.offsets) - 1

    @property
    def counts(self) -> np.ndarray:
        """Hits per query."""
        return np.diff(self._host(self.offsets, np.uint64)).astype(np.uint64)

    def row(self, i: int):
        """``(indices, distances)`` of query ``i``."""
        if not -len(self) <= i < len(self):
            raise IndexError("query index out of range")
        i %= len(self)
        if self.indices is None:
            raise ValueError("a counting call holds no rows")
        offsets = self._host(self.offsets, np.uint64)
        first, last = int(offsets[i]), int(offsets[i + 1])
        return self._host(self.indices, np.uint32)[first:last], self._host(self.distances, np.uint32)[first:last]

    def pairs(self, upper: bool = False):
        """Flat ``(i, j, d)`` arrays of every hit, in row order. ``upper=True`` keeps ``i < j``: each unordered pair of a self-search
        once and no string with itself, which is what deduplication wants."""
        if self.indices is None:
            raise ValueError("a counting call holds no pairs")
        total = int(self._host(self.offsets, np.uint64)[-1])
        i = np.repeat(np.arange(len(self), dtype=np.uint64), self.counts.astype(np.int64))
        j, d = self._host(self.indices, np.uint32)[:total], self._host(self.distances, np.uint32)[:total]
        if upper:
            keep = i < j
            return i[keep], j[keep], d[keep]
        return i, j, d


class ScoreMatches:
    """The result of ``LevenshteinDistances.extract_within``: for every query the candidates whose score passes the cutoff, as CSR.

    Row ``i`` is ``indices[offsets[i]:offsets[i + 1]]`` with the float64 scores in ``scores`` at the same places, ascending by
    candidate index (callers who want them by score sort a row, or use ``extract``). ``offsets`` is uint64 with one entry more than
    there are queries. Arrays that live on the device (``out=`` tensors) are brought to the host when a row or the pairs are asked for.
    The result of a counting call (``out=(offsets, None, None)``) has ``offsets`` and ``counts`` only: ``indices`` and ``scores`` are None."""

    def __init__(self, offsets, indices, scores):
        self.offsets, self.indices, self.scores = offsets, indices, scores
        if len(offsets) < 1 or (indices is None) != (scores is None) or (indices is not None and len(indices) != len(scores)):
            raise ValueError("offsets needs at least one entry, indices and scores the same length (or both None: counted, not filled)")

    _host = staticmethod(RangeMatches._host)

    def __len__(self) -> int:
        """The number of queries (rows)."""
        return len(self.offsets) - 1

    @property
    def counts(self) -> np.ndarray:
        """Hits per query."""
        return np.diff(self._host(self.offsets, np.uint64)).astype(np.uint64)

    def row(self, i: int):
        """``(indices, scores)`` of query ``i``."""
        if not -len(self) <= i < len(self):
            raise IndexError("query index out of range")
        i %= len(self)
        if self.indices is None:
            raise ValueError("a counting call holds no rows")
        offsets = self._host(self.offsets, np.uint64)
        first, last = int(offsets[i]), int(offsets[i + 1])
        return self._host(self.indices, np.uint32)[first:last], self._host(self.scores, np.float64)[first:last]

    def pairs(self, upper: bool = False):
        """Flat ``(i, j, score)`` arrays of every hit, in row order. ``upper=True`` keeps ``i < j``: each unordered pair of a
        self-search once and no string with itself, which is what deduplication wants."""
        if self.indices is None:
            raise ValueError("a counting call holds no pairs")
        total = int(self._host(self.offsets, np.uint64)[-1])
        i = np.repeat(np.arange(len(self), dtype=np.uint64), self.counts.astype(np.int64))
        j, score = self._host(self.indices, np.uint32)[:total], self._host(self.scores, np.float64)[:total]
        if upper:
            keep = i < j
            return i[keep], j[keep], score[keep]
        return i, j, score


class Alignments:
    """The result of ``LevenshteinDistances.align``: a tape of edit operations, one string of op bytes per pair.

    ``distances[i]`` is ``min(d, bound + 1)``; pair ``i``'s ops are ``ops[offsets[i]:offsets[i + 1]]``, in forward order, each one of
    ``=`` (match), ``X`` (substitution), ``D`` (a symbol of ``a`` only) and ``I`` (a symbol of ``b`` only); a pair over the bound has none.
    The script is the library's CANONICAL one among the optimal ones (walking back from the end: ``=`` on equal symbols, else ``X`` if the
    diagonal is optimal, else ``D`` if the cell above is, else ``I``) -- not necessarily the one rapidfuzz or edlib picks when several are
    optimal, though it has the same length and cost. Positions count symbols: bytes, or code points for the UTF-8 engine."""

    _TAGS = {N.OP_SUBST: "replace", N.OP_DEL: "delete", N.OP_INS: "insert"}

    def __init__(self, distances, offsets, ops):
        self.distances = np.asarray(distances, dtype=np.uint32)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.ops = np.asarray(ops, dtype=np.uint8)
        if len(self.offsets) != len(self.distances) + 1:
            raise ValueError("offsets must have one entry more than distances")

    def __len__(self) -> int:
        return len(self.distances)

    def __getitem__(self, i: int) -> bytes:
        """The op bytes of pair ``i``, e.g. ``b"X===X=I"``."""
        if not -len(self) <= i < len(self):
            raise IndexError("pair index out of range")
        i %= len(self)
        return self.ops[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()

    def cigar(self, i: int) -> str:
        """SAM extended CIGAR of pair ``i`` (``=`` / ``X`` / ``D`` / ``I`` runs, ``a`` as the read, ``b`` as the reference): kitten -> sitting
        gives ``"1X3=1X1=1I"``. Empty for a pair over the bound and for two empty strings."""
        ops = self[i]
        out, run, last = [], 0, None
        for op in ops:
            if op == last:
                run += 1
                continue
            if last is not None:
                out.append("%d%c" % (run, last))
            last, run = op, 1
        if last is not None:
            out.append("%d%c" % (run, last))
        return "".join(out)

    def editops(self, i: int):
        """rapidfuzz-shaped ``Levenshtein.editops``: ``(tag, src_pos, dest_pos)`` tuples with the tags ``replace`` / ``delete`` /
        ``insert``, positions in symbols of ``a`` (source) and ``b`` (destination). The canonical script of this library, which is one of
        the optimal ones but need not be the one rapidfuzz returns."""
        result, src, dst = [], 0, 0
        for op in self[i]:
            if op == N.OP_MATCH:
                src += 1; dst += 1
                continue
            result.append((self._TAGS[op], src, dst))
            if op == N.OP_SUBST:
                src += 1; dst += 1
            elif op == N.OP_DEL:
                src += 1
            else:
                dst += 1
        return result


class InfixMatches:
    """The result of ``LevenshteinDistances.infix``: the best approximate occurrence of every pattern in its text.

    ``distances[i]`` is ``min(d, bound + 1)``, ``d`` the smallest distance of pattern ``i`` to any substring of text ``i``; the occurrence
    is ``text[starts[i]:ends[i]]`` -- the CANONICAL one: the smallest end that reaches ``d`` and, for that end, the shortest substring.
    A pair over the bound has ``starts[i] == ends[i] == INFIX_NONE``. Positions count symbols: bytes, or code points for the UTF-8 engine."""

    def __init__(self, distances, starts, ends):
        self.distances = np.asarray(distances, dtype=np.uint32)
        self.starts = np.asarray(starts, dtype=np.uint32)
        self.ends = np.asarray(ends, dtype=np.uint32)
        if not len(self.distances) == len(self.starts) == len(self.ends):
            raise ValueError("distances, starts and ends must have one entry per pair")

    def __len__(self) -> int:
        return len(self.distances)

    @property
    def found(self) -> np.ndarray:
        """Bool mask of the pairs whose best occurrence is within the bound."""
        return self.ends != np.uint32(N.INFIX_NONE)

    def __getitem__(self, i: int):
        """``(distance, start, end)`` of pair ``i``, or ``None`` when its best occurrence is over the bound."""
        if not -len(self) <= i < len(self):
            raise IndexError("pair index out of range")
        i %= len(self)
        if int(self.ends[i]) == N.INFIX_NONE:
            return None
        return int(self.distances[i]), int(self.starts[i]), int(self.ends[i])


class PartialAlignments:
    """The result of ``LevenshteinDistances.partial_ratio_alignment``, after rapidfuzz's ``ScoreAlignment``: ``score[i]`` is
    ``fuzz.partial_ratio(a[i], b[i])`` as float64, reached between ``a[i][src_start[i]:src_end[i]]`` and
    ``b[i][dest_start[i]:dest_end[i]]``. The shorter string (the needle) spans its whole length, the other side is the best window --
    among windows of equal score the one of the smallest offset. Positions count symbols: bytes, or code points for the UTF-8 engine."""

    def __init__(self, score, src_start, src_end, dest_start, dest_end):
        self.score = np.asarray(score, dtype=np.float64)
        self.src_start, self.src_end, self.dest_start, self.dest_end = (np.asarray(x, dtype=np.uint32) for x in (src_start, src_end, dest_start, dest_end))
        if not len(self.score) == len(self.src_start) == len(self.src_end) == len(self.dest_start) == len(self.dest_end):
            raise ValueError("one entry per pair in every array")

    def __len__(self) -> int:
        return len(self.score)

    def __getitem__(self, i: int):
        """``(score, src_start, src_end, dest_start, dest_end)`` of pair ``i``."""
        if not -len(self) <= i < len(self):
            raise IndexError("pair index out of range")
        i %= len(self)
        return (float(self.score[i]), int(self.src_start[i]), int(self.src_end[i]), int(self.dest_start[i]), int(self.dest_end[i]))


def _as_tape(obj: TapeLike):
    if isinstance(obj, (Strs, DeviceTape, PreparedTape)):
        return obj
    return Strs(obj)


def _symbol_lengths(tape, utf8: bool, scope: DeviceScope) -> np.ndarray:
    """Symbols of every string of a tape as int64: bytes, or with ``utf8`` code points (bytes that are no continuation bytes).
    Device tapes are read back; prepared tapes remember what they were prepared from."""
    if isinstance(tape, PreparedTape):
        return tape.symbol_lengths(scope)
    if isinstance(tape, DeviceTape):
        err = C.c_char_p()
        offsets = np.zeros(tape.count + 1, dtype=tape.offsets_dtype)
        N.check(N.lib.swh_copy_to_host(scope.handle, offsets.ctypes.data, C.c_void_p(tape.offsets_ptr), offsets.nbytes, C.byref(err)), err)
        data = np.zeros(int(offsets[-1]) if utf8 else 0, dtype=np.uint8)
        if data.nbytes:
            N.check(N.lib.swh_copy_to_host(scope.handle, data.ctypes.data, C.c_void_p(tape.data_ptr), data.nbytes, C.byref(err)), err)
        tape = Strs(data=data, offsets=offsets)
    if not utf8:
        return tape.lengths
    starts = np.zeros(len(tape.data) + 1, dtype=np.int64)
    np.cumsum((tape.data & 0xC0) != 0x80, out=starts[1:])
    at = starts[tape.offsets.astype(np.int64)]
    return at[1:] - at[:-1]


def _c_tape(tape, want64: Optional[bool] = None):
    """ctypes tape struct + its width; keeps arrays alive through the returned tuple."""
    if isinstance(tape, Strs):
        if want64 is True and tape.offsets.dtype != np.uint64:
            tape = tape.with_offsets(np.uint64)
        is64 = tape.offsets.dtype == np.uint64
        struct = (N.TapeU64 if is64 else N.TapeU32)(tape.data.ctypes.data, tape.offsets.ctypes.data, tape.count)
        return struct, is64, tape
    is64 = tape.offsets_dtype == np.dtype(np.uint64)
    if want64 is True and not is64:
        raise TypeError("this call needs u64 offsets on the device tape")
    struct = (N.TapeU64 if is64 else N.TapeU32)(tape.data_ptr, tape.offsets_ptr, tape.count)
    return struct, is64, tape


_EXPORTS = {}   # (engine type, stem, prepared) -> the export, as _Engine._two_tapes found it


class _Engine:
    _utf8 = False
    _abi_prefix = "swh_levenshtein"

    def __init__(self):
        self._handle = None

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

    def _two_tapes(self, a, b, scope, stem):
        """The two sides of one ``<prefix>_<stem>_prepared`` / ``<prefix>_[utf8_]<stem>_u64tape`` call: both prepared (the first in the
        engine's mode), or neither; ``b`` None is a null pointer. Returns ``call``: ``call(*tail, byref(err))`` passes the engine, the
        scope, the two sides and the C arguments ``tail``, keeps the tapes alive meanwhile and returns the status for ``N.check``.
        A search of 2048 x 2048 words takes ~100 us, so a prepared call is held to what the inline calls cost (0.3 us more, on a
        stub export): the export is looked up by name once per (engine type, stem, form), and ``call`` is a ``partial`` of the export
        itself -- no Python frame between the caller and the library."""
        prepared = isinstance(a, PreparedTape) or isinstance(b, PreparedTape)
        key = (type(self), stem, prepared)
        fn = _EXPORTS.get(key)
        if fn is None:
            form = "%s_prepared" % stem if prepared else "%s%s_u64tape" % ("utf8_" if self._utf8 else "", stem)
            fn = _EXPORTS[key] = getattr(N.lib, "%s_%s" % (self._abi_prefix, form))
        if prepared:
            if not isinstance(a, PreparedTape) or not (b is None or isinstance(b, PreparedTape)):
                raise TypeError("both tapes of a call must be prepared, or neither")
            self._need_mode(a)
            return functools.partial(fn, self._handle, scope.handle, C.byref(a.view()), None if b is None else C.byref(b.view()))
        kept = (_c_tape(a, want64=True), None if b is None else _c_tape(b, want64=True))
        call = functools.partial(fn, self._handle, scope.handle, C.byref(kept[0][0]), None if b is None else C.byref(kept[1][0]))
        call.kept = kept   # (the structs hold bare pointers into these arrays; prepared tapes are the caller's own arguments)
        return call

    def _prepared(self, stem, a, b, scope, out, out_dtype, extra=(), cross=False):
        """The ``*_prepared`` twin of a call: both sides are PreparedTape views."""
        call = self._two_tapes(a, b, scope, stem)
        if out is None:
            shape = (len(a), len(b if b is not None else a)) if cross else (len(a),)
            out = np.zeros(shape, dtype=out_dtype)
        stride = 0
        if isinstance(out, np.ndarray):
            stride = out.strides[0] if (cross or out.size > 1) else 0
        err = C.c_char_p()
        N.check(call(*extra, C.c_void_p(_pointer(out)), stride, C.byref(err)), err)
        return out

    def cross_sharded(self, product: "ShardedCross", scope: DeviceScope, out=None):
        """The dense matrix of a sharded product: every device of the scope fills its rows and copies them into `out` (host
        memory or memory of the first device; 64-bit entries)."""
        if self._utf8 != product.utf8:
            raise ValueError("engine and sharded product disagree on UTF-8")
        if out is None:
            out = np.zeros(product.shape, dtype=np.uint64 if self._abi_prefix == "swh_levenshtein" else np.int64)
        if isinstance(out, np.ndarray) and (out.dtype.itemsize != 8 or out.shape != product.shape):
            raise ValueError("out must be a (len(queries), len(candidates)) matrix of 64-bit integers")
        row_stride = out.strides[0] if isinstance(out, np.ndarray) else product.shape[1] * 8
        err = C.c_char_p()
        status = getattr(N.lib, self._abi_prefix + "_cross_sharded")(self._handle, scope.handle, product._handle, C.c_void_p(_pointer(out)), row_stride, C.byref(err))
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
        fn = getattr(N.lib, self._abi_prefix + "_pairs_prepared")
        extra = (C.c_uint32(N.UNBOUNDED if bound is None else int(bound)),) if self._abi_prefix == "swh_levenshtein" else ()
        args = (self._handle, scope.handle, C.byref(va), C.byref(vb), *extra, C.c_void_p(_pointer(out)),
                out.strides[0] if isinstance(out, np.ndarray) and out.size > 1 else 0, C.byref(err))
        keep = (va, vb, err, a, b, out)

        def call(_fn=fn, _args=args, _keep=keep):
            status = _fn(*_args)
            if status != N.SUCCESS:
                N.check(status, _keep[2])
        return call

    def _pairs(self, fn32, fn64, a, b, scope, out, out_dtype, extra=(), prepared_stem="pairs"):
        """``fn32`` is None for a call family that only takes u64 tapes."""
        a, b = _as_tape(a), _as_tape(b)
        if len(a) != len(b):
            raise ValueError("pairwise scoring needs two collections of equal length")
        if isinstance(a, PreparedTape) or isinstance(b, PreparedTape):
            return self._prepared(prepared_stem, a, b, scope, out, out_dtype, extra)
        ta, a64, keep_a = _c_tape(a, want64=True if fn32 is None else None)
        tb, b64, keep_b = _c_tape(b, want64=a64 or None)
        if a64 != b64:
            ta, a64, keep_a = _c_tape(a, want64=True)
            tb, b64, keep_b = _c_tape(b, want64=True)
        if out is None:
            out = np.empty(len(a), dtype=out_dtype)
        stride = out.strides[0] if isinstance(out, np.ndarray) and out.ndim == 1 and out.size > 1 else 0
        err = C.c_char_p()
        fn = fn64 if a64 else fn32
        status = fn(self._handle, scope.handle, C.byref(ta), C.byref(tb), *extra, C.c_void_p(_pointer(out)), stride, C.byref(err))
        N.check(status, err)
        del keep_a, keep_b
        return out

    def _cross(self, fn, queries, candidates, scope, out, out_dtype, prepared_stem="cross"):
        queries = _as_tape(queries)
        candidates = queries if candidates is None else _as_tape(candidates)
        if isinstance(queries, PreparedTape) or isinstance(candidates, PreparedTape):
            if isinstance(out, np.ndarray) and (out.dtype.itemsize != 8 or out.shape != (len(queries), len(candidates))):
                raise ValueError("out must be a (len(queries), len(candidates)) matrix of 64-bit integers")
            return self._prepared(prepared_stem, queries, candidates, scope, out, out_dtype, cross=True)
        tq, _, keep_q = _c_tape(queries, want64=True)
        tc, _, keep_c = _c_tape(candidates, want64=True)
        if out is None:
            out = np.zeros((len(queries), len(candidates)), dtype=out_dtype)
        row_stride = out.strides[0] if isinstance(out, np.ndarray) else len(candidates) * 8
        if isinstance(out, np.ndarray) and (out.dtype.itemsize != 8 or out.shape != (len(queries), len(candidates))):
            raise ValueError("out must be a (len(queries), len(candidates)) matrix of 64-bit integers")
        err = C.c_char_p()
        status = fn(self._handle, scope.handle, C.byref(tq), C.byref(tc), C.c_void_p(_pointer(out)), row_stride, C.byref(err))
        N.check(status, err)
        del keep_q, keep_c
        return out


class LevenshteinDistances(_Engine):
    """``szs.LevenshteinDistances`` / ``LevenshteinDistances::new(&scope, 0, 1, 1, 1)`` (bench.rs:382).

    ``engine(queries, candidates, scope, out=matrix)`` is the reference's dense cross-product
    (bench.py:421-422, bench.rs:478-486); ``engine.pairs(a, b, scope, bound=k)`` scores
    ``a[i]`` against ``b[i]`` and returns ``min(d, k+1)``.
    """

    def __init__(self, match: int = 0, mismatch: int = 1, open: int = 1, extend: int = 1, *,
                 capabilities: Optional[DeviceScope] = None, algorithm: str = "auto"):
        super().__init__()
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
        if scope is None:
            raise ValueError("a DeviceScope is required")
        fn = N.lib.swh_levenshtein_utf8_cross_u64tape if self._utf8 else N.lib.swh_levenshtein_cross_u64tape
        return self._cross(fn, queries, candidates, scope, out, np.uint64)

    def pairs(self, a: TapeLike, b: TapeLike, scope: DeviceScope, bound: Optional[int] = None, out=None):
        bound_value = N.UNBOUNDED if bound is None else int(bound)
        if self._utf8:
            fns = (N.lib.swh_levenshtein_utf8_pairs_u32tape, N.lib.swh_levenshtein_utf8_pairs_u64tape)
        else:
            fns = (N.lib.swh_levenshtein_pairs_u32tape, N.lib.swh_levenshtein_pairs_u64tape)
        return self._pairs(fns[0], fns[1], a, b, scope, out, np.uint32, extra=(C.c_uint32(bound_value),))

    def topk(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, *, k: int,
             bound: Optional[int] = None, out=None):
        """The ``k`` nearest candidates of every query: ``(indices, distances)``, each ``(len(queries), k)`` of uint32, rows ordered
        by distance and then by candidate index, only candidates with ``d <= bound``, short rows padded with ``0xFFFFFFFF``.
        ``candidates=None`` searches the queries themselves (diagonal included). ``out=(indices, distances)`` fills given arrays
        or device tensors (contiguous, ``len(queries) * k`` uint32 / int32 each) instead of returning new numpy arrays.
        Two prepared byte tapes must share one offset width: one prepared from uint32 and one from uint64 offsets raise
        ``StringWarsError('invalid_argument')`` and nothing is written.
        rapidfuzz: ``process.extract(q, candidates, scorer=Levenshtein.distance, limit=k, score_cutoff=bound)`` per query."""
        if scope is None:
            raise ValueError("a DeviceScope is required")
        queries = _as_tape(queries)
        if candidates is not None:
            candidates = _as_tape(candidates)
        count = len(queries)
        if out is None:
            indices, distances = np.empty((count, int(k)), dtype=np.uint32), np.empty((count, int(k)), dtype=np.uint32)
        else:
            indices, distances = out
            for array in (indices, distances):
                if isinstance(array, np.ndarray) and (array.dtype.itemsize != 4 or array.size != count * int(k) or not array.flags.c_contiguous):
                    raise ValueError("out arrays must be contiguous (len(queries), k) arrays of 32-bit integers")
        bound_value = C.c_uint32(N.UNBOUNDED if bound is None else int(bound))
        err = C.c_char_p()
        N.check(self._two_tapes(queries, candidates, scope, "topk")(int(k), bound_value, C.c_void_p(_pointer(indices)),
                                                                    C.c_void_p(_pointer(distances)), C.byref(err)), err)
        return indices, distances

    @staticmethod
    def _csr_search(call, count, others, out, capacity, value_dtype, result):
        """The capacity protocol of the two range searches (``within``, ``extract_within``). ``call(offsets, indices, values, room)``
        runs the search and returns the hit total; ``values`` are the distances (uint32) or the scores (float64). With ``out`` the
        given arrays or tensors are checked and filled (too small: the offsets are written, then ``ValueError``); without, the first
        call has room for ``capacity`` hits and a second is made with the exact size only if they did not fit."""
        value_width = np.dtype(value_dtype).itemsize
        if out is not None:
            offsets, indices, values = out
            room = 0 if indices is None else int(indices.numel() if hasattr(indices, "numel") else indices.size)
            for array, width, entries in ((offsets, 8, count + 1), (indices, 4, room), (values, value_width, room)):
                if array is None:
                    continue
                size = int(array.numel() if hasattr(array, "numel") else array.size)
                itemsize = array.element_size() if hasattr(array, "element_size") else array.dtype.itemsize
                contiguous = array.is_contiguous() if hasattr(array, "is_contiguous") else array.flags.c_contiguous
                if itemsize != width or size != entries or not contiguous:
                    raise ValueError("out needs len(queries) + 1 64-bit offsets, and contiguous 32-bit indices and %d-bit values of one size"
                                     % (8 * value_width))
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
        if scope is None:
            raise ValueError("a DeviceScope is required")
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
        if scope is None:
            raise ValueError("a DeviceScope is required")
        a, b = self._promoted(a, b, scope, at=DeviceTape)
        if len(a) != len(b):
            raise ValueError("a and b must hold the same number of strings")
        count = len(a)
        bound_value = C.c_uint32(N.UNBOUNDED if bound is None else int(bound))
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
        N.check(call(bound_value, C.c_void_p(distances.ctypes.data), C.c_void_p(offsets.ctypes.data), C.c_void_p(ops.ctypes.data), capacity,
                     C.byref(err)), err)
        used = int(offsets[-1])
        return Alignments(distances, offsets, ops[:used].copy() if 2 * used < len(ops) else ops[:used])

    def infix(self, patterns: TapeLike, texts: TapeLike, scope: Optional[DeviceScope] = None, bound: Optional[int] = None) -> "InfixMatches":
        """Where, and how well, ``patterns[i]`` approximately occurs in ``texts[i]`` on unit costs (``swh_levenshtein_infix_*``): an
        :class:`InfixMatches` with ``distances``, ``starts`` and ``ends``. Patterns hold at most ``INFIX_MAX_PATTERN`` symbols. The two
        sides are tapes, or both ``PreparedTape``s. edlib: ``align(p, t, mode="HW", k=bound)`` (``editDistance``, ``locations[0]`` with an
        inclusive end); rapidfuzz: ``partial_ratio_alignment`` (``dest_start`` / ``dest_end``)."""
        if scope is None:
            raise ValueError("a DeviceScope is required")
        patterns, texts = self._promoted(patterns, texts, scope, at=DeviceTape)
        if len(patterns) != len(texts):
            raise ValueError("patterns and texts must hold the same number of strings")
        count = len(patterns)
        bound_value = C.c_uint32(N.UNBOUNDED if bound is None else int(bound))
        distances, starts, ends = (np.empty(count, dtype=np.uint32) for _ in range(3))
        call = self._two_tapes(patterns, texts, scope, "infix")
        if isinstance(patterns, PreparedTape):
            self._need_mode(texts)
        err = C.c_char_p()
        N.check(call(bound_value, *(C.c_void_p(array.ctypes.data) for array in (distances, starts, ends)), C.byref(err)), err)
        return InfixMatches(distances, starts, ends)

    def osa(self, a: TapeLike, b: TapeLike, scope: Optional[DeviceScope] = None, bound: Optional[int] = None, out=None):
        """Damerau-Levenshtein distances in the optimal-string-alignment (OSA, restricted) form of every pair ``(a[i], b[i])``
        (``swh_levenshtein_osa_pairs_*``): ``min(d, bound + 1)`` as uint32, where a swap of two neighbouring symbols costs one edit
        and no substring is edited twice (``ab`` / ``ba``: 1; ``ca`` / ``abc``: 3, not the 2 of unrestricted Damerau-Levenshtein).
        The shorter string of a pair holds at most ``OSA_MAX_SHORTER`` symbols. The two sides are tapes, or both ``PreparedTape``s.
        rapidfuzz: ``OSA.distance(a[i], b[i], score_cutoff=bound)``."""
        if scope is None:
            raise ValueError("a DeviceScope is required")
        a, b = self._promoted(a, b, scope, at=DeviceTape)
        fn = N.lib.swh_levenshtein_utf8_osa_pairs_u64tape if self._utf8 else N.lib.swh_levenshtein_osa_pairs_u64tape
        bound_value = N.UNBOUNDED if bound is None else int(bound)
        return self._pairs(None, fn, a, b, scope, out, np.uint32, extra=(C.c_uint32(bound_value),), prepared_stem="osa_pairs")

    def osa_cross(self, queries: TapeLike, candidates: Optional[TapeLike] = None, scope: Optional[DeviceScope] = None, out=None):
        """The dense OSA matrix ``out[i][j] = osa(queries[i], candidates[j])`` as uint64 (``swh_levenshtein_osa_cross_*``), the shape of
        ``engine(queries, candidates, scope)``; ``candidates=None`` is the self-product (symmetric, zero diagonal).
        rapidfuzz: ``process.cdist(queries, candidates, scorer=OSA.distance)``."""
        if scope is None:
            raise ValueError("a DeviceScope is required")
        queries, candidates = self._promoted(queries, candidates, scope, at=DeviceTape)
        fn = N.lib.swh_levenshtein_utf8_osa_cross_u64tape if self._utf8 else N.lib.swh_levenshtein_osa_cross_u64tape
        return self._cross(fn, queries, candidates, scope, out, np.uint64, prepared_stem="osa_cross")

    def _scored_call(self, family, a, b, scope, cross, outs, extra=()):
        """One ``swh_levenshtein_{lcs,jaro}_*`` call. ``outs``: for each output of the family, in the order of its exports, the array
        to fill, True for a fresh one, None where that output is not wanted; ``extra``: the C arguments between the tapes and the
        outputs (the bound of the pairwise LCS calls). Returns the arrays (None where not wanted) and the two tapes as called."""
        if scope is None:
            raise ValueError("a DeviceScope is required")
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
        strides = set()
        for out in outs:
            if isinstance(out, np.ndarray):
                if out.dtype.itemsize != dtype().itemsize or out.shape != shape:
                    raise ValueError("an output must be a %s array of %d-bit integers" % (shape, 8 * dtype().itemsize))
                strides.add(out.strides[0] if (cross or out.size > 1) else 0)
        if len(strides) > 1:
            raise ValueError("the outputs share one stride")
        stride = strides.pop() if strides else 0
        call = self._two_tapes(a, b, scope, "%s_%s" % (family, "cross" if cross else "pairs"))
        err = C.c_char_p()
        N.check(call(*extra, *(C.c_void_p(None if out is None else _pointer(out)) for out in outs), stride, C.byref(err)), err)
        return outs, a, (a if b is None else b)

    def _lcs_call(self, a, b, scope, cross, bound, indel, lcs):
        """The Indel distances and the LCS lengths of one ``swh_levenshtein_lcs_*`` call, each as ``_scored_call`` takes and returns it."""
        extra = () if cross else (C.c_uint32(N.UNBOUNDED if bound is None else int(bound)),)
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
        if scope is None:
            raise ValueError("a DeviceScope is required")
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
            for array, width in ((indices, 4), (scores, 8)):
                if isinstance(array, np.ndarray) and (array.dtype.itemsize != width or array.size != count * int(k) or not array.flags.c_contiguous):
                    raise ValueError("out arrays must be contiguous (len(queries), k) arrays of uint32 and float64")
                if hasattr(array, "element_size") and (array.element_size() != width or array.numel() != count * int(k) or not array.is_contiguous()):
                    raise ValueError("out tensors must be contiguous, of len(queries) * k elements of 4 (indices) and 8 (scores) bytes")
        if cutoff is None:
            cutoff = 0.0 if N.SCORERS[scorer] >= N.SCORERS["lcs"] else float("inf")
        bits = [C.c_uint64(int(np.float64(value).view(np.uint64))) for value in (cutoff, prefix_weight)]   # what memcpy of the double gives
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
        if scope is None:
            raise ValueError("a DeviceScope is required")
        if scorer not in N.SCORERS:
            raise ValueError("scorer must be one of %s" % ", ".join(N.SCORERS))
        if cutoff is None:
            raise ValueError("a range search needs a cutoff; without one it is the dense cross-product")
        queries = _as_tape(queries)
        if candidates is not None:
            candidates = _as_tape(candidates)
        count = len(queries)
        search = self._two_tapes(queries, candidates, scope, "extract_within")
        bits = [C.c_uint64(int(np.float64(value).view(np.uint64))) for value in (cutoff, prefix_weight)]   # what memcpy of the double gives

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
                                                     N.UNBOUNDED if bound is None else int(bound), C.c_void_p(_pointer(out)), C.byref(err))
        N.check(status, err)
        return out

    def __del__(self):
        if getattr(self, "_handle", None) and getattr(N, "lib", None) is not None:   # module globals go first at exit
            N.lib.swh_levenshtein_free(self._handle)
            self._handle = None


class LevenshteinDistancesUTF8(LevenshteinDistances):
    """``szs.LevenshteinDistancesUTF8`` / ``LevenshteinDistancesUtf8`` (bench.rs:386-399): symbols are
    Unicode scalar values; invalid UTF-8 raises ``StringWarsError('invalid_utf8')``."""

    _utf8 = True


class NeedlemanWunschScores(_Engine):
    """``szs.NeedlemanWunschScores(byte_to_class, class_costs, open=, extend=, capabilities=)``
    (bench.py:466-472, bench.rs:658-662). ``substitution_matrix=`` takes a full 256x256 int8 table
    instead (config C4). gap(k) = open + (k-1)*extend."""

    _prefix = "swh_nw"
    _abi_prefix = "swh_nw"

    def __init__(self, byte_to_class: Optional[np.ndarray] = None, class_costs: Optional[np.ndarray] = None, *,
                 open: int = -2, extend: int = -2, capabilities: Optional[DeviceScope] = None,
                 substitution_matrix: Optional[np.ndarray] = None):
        super().__init__()
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
        if scope is None:
            raise ValueError("a DeviceScope is required")
        return self._cross(getattr(N.lib, self._prefix + "_cross_u64tape"), queries, candidates, scope, out, np.int64)

    def pairs(self, a: TapeLike, b: TapeLike, scope: DeviceScope, out=None):
        return self._pairs(getattr(N.lib, self._prefix + "_pairs_u32tape"), getattr(N.lib, self._prefix + "_pairs_u64tape"),
                           a, b, scope, out, np.int32)

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

    def __del__(self):
        if getattr(self, "_handle", None) and getattr(N, "lib", None) is not None:   # module globals go first at exit
            getattr(N.lib, self._prefix + "_free")(self._handle)
            self._handle = None


class SmithWatermanScores(NeedlemanWunschScores):
    """``szs.SmithWatermanScores`` (bench.py:789, bench.rs:882-963): local alignment score, same arguments."""

    _prefix = "swh_sw"
    _abi_prefix = "swh_sw"


def edit_distance(column_a: TapeLike, column_b: TapeLike, scope: DeviceScope, utf8: bool = True,
                  bound: Optional[int] = None) -> np.ndarray:
    """Element-wise edit distance of two equal-length string columns, the call shape of
    ``cudf.Series.str.edit_distance(other)`` (similarities/bench.py:602)."""
    engine = (LevenshteinDistancesUTF8 if utf8 else LevenshteinDistances)(capabilities=scope)
    return engine.pairs(column_a, column_b, scope, bound=bound)
