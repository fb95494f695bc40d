"""What the calls that return more than one array give back: the CSR rows of the two range searches, the op tape of ``align``, the
occurrences of ``infix`` and the windows of ``partial_ratio_alignment``."""
from __future__ import annotations

import numpy as np

from . import _native as N


class _CsrMatches:
    """For every query the candidates a range search admitted, as CSR: row ``i`` is ``indices[offsets[i]:offsets[i + 1]]`` with the
    values at the same places, ascending by candidate index. ``offsets`` is uint64 with one entry more than there are queries. Arrays
    that live on the device (``out=`` tensors) are brought to the host when a row or the pairs are asked for. The result of a counting
    call (``out=(offsets, None, None)``) has ``offsets`` and ``counts`` only: ``indices`` and the values are None.
    A subclass names the attribute its values are kept under (``_values``) and their dtype (``_dtype``)."""

    _values, _dtype = None, None

    def __init__(self, offsets, indices, values):
        self.offsets, self.indices = offsets, indices
        setattr(self, self._values, values)
        if len(offsets) < 1 or (indices is None) != (values is None) or (indices is not None and len(indices) != len(values)):
            raise ValueError("offsets needs at least one entry, indices and %s the same length (or both None: counted, not filled)" % self._values)

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
        """``(indices, values)`` of query ``i``."""
        if not -len(self) <= i < len(self):
            raise IndexError("query index out of range")
        i %= len(self)
        if self.indices is None:
            raise ValueError("a counting call holds no rows")
        offsets = self._host(self.offsets, np.uint64)
        first, last = int(offsets[i]), int(offsets[i + 1])
        return self._host(self.indices, np.uint32)[first:last], self._host(getattr(self, self._values), self._dtype)[first:last]

    def pairs(self, upper: bool = False):
        """Flat ``(i, j, value)`` arrays of every hit, in row order. ``upper=True`` keeps ``i < j``: each unordered pair of a
        self-search once and no string with itself, which is what deduplication wants."""
        if self.indices is None:
            raise ValueError("a counting call holds no pairs")
        total = int(self._host(self.offsets, np.uint64)[-1])
        i = np.repeat(np.arange(len(self), dtype=np.uint64), self.counts.astype(np.int64))
        j, value = self._host(self.indices, np.uint32)[:total], self._host(getattr(self, self._values), self._dtype)[:total]
        if upper:
            keep = i < j
            return i[keep], j[keep], value[keep]
        return i, j, value


class RangeMatches(_CsrMatches):
    """The result of ``LevenshteinDistances.within``: for every query the candidates within the bound, with the true distances
    (uint32) in ``distances``. Callers who want a row by distance sort it, or use ``topk``."""

    _values, _dtype = "distances", np.uint32


class ScoreMatches(_CsrMatches):
    """The result of ``LevenshteinDistances.extract_within``: for every query the candidates whose score passes the cutoff, with the
    float64 scores in ``scores``. Callers who want a row by score sort it, or use ``extract``."""

    _values, _dtype = "scores", np.float64


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


class InfixOccurrences:
    """The result of ``LevenshteinDistances.infix_all``: for every pair the ends at which the pattern occurs within the bound, as CSR.
    Row ``i`` is ``[offsets[i], offsets[i + 1])`` of ``starts``, ``ends`` and ``distances``, ascending by end: the pattern occurs as
    ``text[starts[h]:ends[h]]`` with the true distance ``distances[h]``, the shortest occurrence that ends there. ``starts`` is None
    where the call skipped the start pass (``starts=False``); a counting call has ``offsets`` and ``counts`` only. Arrays that live
    on the device (``out=`` tensors) are brought to the host when a row is asked for. Positions count symbols."""

    def __init__(self, offsets, starts, ends, distances):
        self.offsets, self.starts, self.ends, self.distances = offsets, starts, ends, distances
        if len(offsets) < 1 or (ends is None) != (distances is None) or (ends is None and starts is not None):
            raise ValueError("offsets needs at least one entry; ends and distances come together, starts only with them")
        if ends is not None and (len(ends) != len(distances) or (starts is not None and len(starts) != len(ends))):
            raise ValueError("starts, ends and distances must have the same length")

    _host = staticmethod(_CsrMatches._host)

    def __len__(self) -> int:
        """The number of pairs (rows)."""
        return len(self.offsets) - 1

    @property
    def counts(self) -> np.ndarray:
        """Hits per pair."""
        return np.diff(self._host(self.offsets, np.uint64)).astype(np.uint64)

    def row(self, i: int):
        """``(starts, ends, distances)`` of pair ``i``; ``starts`` is None where the call skipped the start pass."""
        if not -len(self) <= i < len(self):
            raise IndexError("pair index out of range")
        i %= len(self)
        if self.ends is None:
            raise ValueError("a counting call holds no rows")
        offsets = self._host(self.offsets, np.uint64)
        first, last = int(offsets[i]), int(offsets[i + 1])
        starts = None if self.starts is None else self._host(self.starts, np.uint32)[first:last]
        return starts, self._host(self.ends, np.uint32)[first:last], self._host(self.distances, np.uint32)[first:last]

    def __getitem__(self, i: int):
        """The hits of pair ``i`` as a list of ``(distance, start, end)``, ascending by end (``start`` None without the start pass)."""
        starts, ends, distances = self.row(i)
        return [(int(distances[h]), None if starts is None else int(starts[h]), int(ends[h])) for h in range(len(ends))]


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
