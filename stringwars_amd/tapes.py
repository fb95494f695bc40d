"""What a call is made on: the scope, the tapes in their three residences (``Strs`` on the host, ``DeviceTape`` in device memory,
``PreparedTape`` made ready once by the library) and the two sharded batches of a multi-GPU scope -- and the helpers that turn them
into the structs of the C ABI. Every class that owns a library handle is a ``_Owner``."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence, Union

import numpy as np

from . import _native as N


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


class _Owner:
    """One handle of the library and the export that releases it (``_free``, by name). ``free()`` may be called any number of times;
    ``__del__`` never raises, on a half-built object or at interpreter exit, when the module's globals (``N.lib``) are already gone."""

    _handle = None
    _free = None

    def free(self) -> None:
        handle, self._handle = self._handle, None
        if handle and getattr(N, "lib", None) is not None:
            getattr(N.lib, self._free)(handle)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceScope(_Owner):
    """``szs.DeviceScope(gpu_device=0)`` / ``DeviceScope::gpu_device(0)`` (bench.rs:379).

    ``cpu_cores=`` scopes are refused: this backend has no CPU path and says so loudly
    (the reference prints ``SKIPPED (<reason>)`` for a variant whose scope cannot be built).
    ``stream`` may be a raw ``hipStream_t`` address (e.g. ``torch.cuda.current_stream().cuda_stream``).
    """

    _free = "swh_scope_free"

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

    close = _Owner.free


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
        """Two allocations of the scope's, not a handle: released through the scope while it lives."""
        if self._owned and self._scope is not None and self._scope.handle:
            N.lib.swh_device_free(self._scope.handle, C.c_void_p(self.data_ptr))
            N.lib.swh_device_free(self._scope.handle, C.c_void_p(self.offsets_ptr))
        self._owned = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PreparedTape(_Owner):
    """A tape made ready once (``swh_tape_prepare_*``): resident on the scope's device, measured, and -- with
    ``utf8=True`` -- validated and decoded to code points. The counterpart of the ``BytesTapeView`` / ``CharsTapeView`` the
    reference builds once outside its timed closures (bench.rs:292-306; ``try_into`` is where invalid UTF-8 surfaces, and
    so it does here: ``StringWarsError('invalid_utf8')`` from the constructor). Slicing gives zero-copy sub-views
    (``subview(lo, hi)``, bench.rs:134-139). Engines take prepared tapes wherever they take tapes; both sides of a call
    must then be prepared, and in the same mode."""

    _free = "swh_prepared_free"
    _root = None

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
        self._scope = scope
        self.first, self.count = 0, len(tape)

    @classmethod
    def _adopt(cls, scope: DeviceScope, handle: C.c_void_p, utf8: bool, count: int) -> "PreparedTape":
        """A tape the library made on the device (``token_sorted``): the handle is this object's, there is no host source."""
        self = cls.__new__(cls)
        self._handle, self._root, self.utf8 = handle, self, bool(utf8)
        self._keepalive, self._source, self._lengths, self._scope = None, None, None, scope
        self.first, self.count = 0, int(count)
        return self

    def token_sorted(self, unique: bool = False) -> "PreparedTape":
        """The token-sorted normal form of every string of this view as a new ``PreparedTape`` (``swh_tape_token_sort``), derived on
        the device: ``" ".join(sorted(s.split()))``, or with ``unique`` ``" ".join(sorted(set(s.split())))`` -- whitespace as
        ``bytes.split()`` sees it, or ``str.split()`` on a ``utf8=True`` tape. The result owns its memory (the source may be freed),
        is in this tape's mode and is taken wherever a prepared tape is: ``ratio`` of two of them is rapidfuzz's
        ``fuzz.token_sort_ratio``, ``partial_ratio`` its ``partial_token_sort_ratio``. A string holds at most ``TOKEN_MAX_BYTES`` bytes."""
        scope = self._root._scope
        handle, err, view = C.c_void_p(), C.c_char_p(), self.view()
        form = N.TOKENS_UNIQUE if unique else N.TOKENS_SORTED
        N.check(N.lib.swh_tape_token_sort(scope.handle, C.byref(view), form, C.byref(handle), C.byref(err)), err)
        return PreparedTape._adopt(scope, handle, self.utf8, self.count)

    def to_strs(self) -> "Strs":
        """The strings of this view on the host, as a ``Strs`` with uint64 offsets from 0 (``swh_prepared_read``)."""
        root, err = self._root, C.c_char_p()
        offsets = np.zeros(root.count + 1, dtype=np.uint64)
        N.check(N.lib.swh_prepared_read(root._scope.handle, root._handle, None, C.c_void_p(offsets.ctypes.data), C.byref(err)), err)
        data = np.zeros(int(offsets[-1]), dtype=np.uint8)
        if data.nbytes:
            N.check(N.lib.swh_prepared_read(root._scope.handle, root._handle, C.c_void_p(data.ctypes.data), C.c_void_p(offsets.ctypes.data),
                                            C.byref(err)), err)
        window = offsets[self.first:self.first + self.count + 1]
        lo, hi = int(window[0]), int(window[-1])
        return Strs(data=data[lo:hi].copy(), offsets=window - window[0])

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
        if root._lengths is None:   # (a tape derived on the device has no host source: it is read back)
            root._lengths = _symbol_lengths(root.to_strs() if root._source is None else root._source, root.utf8, scope)
        return root._lengths[self.first:self.first + self.count]

    def free(self) -> None:
        if self._root is self:   # a sub-view borrows its root's handle
            super().free()


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


def _c_tapes(a, b, u32: bool = True):
    """The two raw tapes of one call as structs of ONE offset width: ``(struct_a, struct_b, is64, keep)``. Both u32 stay u32 where the
    call has a u32 form (``u32``); otherwise, and on disagreement, host tapes are widened to u64 and a u32 device tape is refused
    (``TypeError``: it cannot be widened in place). ``b`` None gives ``struct_b`` None. ``keep`` holds what the structs point into."""
    ta, is64, keep_a = _c_tape(a, want64=None if u32 else True)
    if b is None:
        return ta, None, is64, (keep_a,)
    tb, b64, keep_b = _c_tape(b, want64=is64 or None)
    if is64 != b64:
        (ta, is64, keep_a), (tb, b64, keep_b) = _c_tape(a, want64=True), _c_tape(b, want64=True)
    return ta, tb, is64, (keep_a, keep_b)


def shard_cuts(a: Strs, b: Strs, shards: int) -> list:
    """Cells-balanced contiguous cuts of a pairwise batch (`swh_shard_cuts_*`): shard r = pairs [cuts[r], cuts[r+1])."""
    ta, tb, is64, _keep = _c_tapes(a, b)
    cuts = (C.c_size_t * (shards + 1))()
    (N.lib.swh_shard_cuts_u64tape if is64 else N.lib.swh_shard_cuts_u32tape)(C.byref(ta), C.byref(tb), shards, cuts)
    return [int(c) for c in cuts]


class ShardedPairs(_Owner):
    """A pairwise batch made resident on every device of a multi-GPU scope (`swh_sharded_prepare_*`): contiguous
    cells-balanced shards, shard r uploaded to and prepared on device r. The steady state of the `<Ngpu>` rows:
    ``engine.pairs_sharded(batch, scope)`` scores all shards and gathers the distances with RCCL."""

    _free = "swh_sharded_free"

    def __init__(self, scope: DeviceScope, a: Strs, b: Strs, utf8: bool = False):
        if not isinstance(a, Strs) or not isinstance(b, Strs):
            raise TypeError("sharding reads host tapes (Strs)")
        ta, tb, is64, _keep = _c_tapes(a, b)
        handle, err = C.c_void_p(), C.c_char_p()
        fn = N.lib.swh_sharded_prepare_u64tape if is64 else N.lib.swh_sharded_prepare_u32tape
        N.check(fn(scope.handle, C.byref(ta), C.byref(tb), int(bool(utf8)), C.byref(handle), C.byref(err)), err)
        self._handle, self.count, self.utf8, self._scope = handle, len(a), bool(utf8), scope

    @property
    def cuts(self) -> list:
        n = self._scope.device_count + 1
        cuts = (C.c_size_t * n)()
        N.lib.swh_sharded_cuts(self._handle, cuts, n)
        return [int(c) for c in cuts]


class ShardedCross(_Owner):
    """A dense queries x candidates product made resident on every device of a multi-GPU scope
    (`swh_sharded_cross_prepare_u64tape`): row blocks of equal query symbols, block r and all candidates prepared on device
    r. ``engine.cross_sharded(product, scope, out=matrix)`` is the `<Ngpu>` twin of the reference's `compute_into`."""

    _free = "swh_sharded_cross_free"

    def __init__(self, scope: DeviceScope, queries: Strs, candidates: Strs, utf8: bool = False):
        if not isinstance(queries, Strs) or not isinstance(candidates, Strs):
            raise TypeError("sharding reads host tapes (Strs)")
        tq, tc, _, _keep = _c_tapes(queries, candidates, u32=False)
        handle, err = C.c_void_p(), C.c_char_p()
        N.check(N.lib.swh_sharded_cross_prepare_u64tape(scope.handle, C.byref(tq), C.byref(tc), int(bool(utf8)), C.byref(handle), C.byref(err)), err)
        self._handle, self.shape, self.utf8, self._scope = handle, (len(queries), len(candidates)), bool(utf8), scope


TapeLike = Union[Strs, DeviceTape, PreparedTape, Sequence[Union[bytes, str]]]


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
