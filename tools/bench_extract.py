"""The score search (`engine.extract`) against what the dense calls can do on the same inputs (MI355X).

Queries x candidate names of 5 .. 25 bytes, prepared tapes, device outputs, k = 10, scorers `jaro_winkler` and `ratio`:
  - the search: call time (host wall clock, median) and, from one profiled call, the kernel time with its split into the scoring kernel
    (`dominant_ms` of `extract_select/<kernel>`: that kernel over all slices) and the rest (the fold, the sizes kernels, the length pass),
    and `kernel_split_ms`: the launches and the summed event time of every stamped kernel of that call by name (the library prints them
    with STRINGWARS_AMD_STAMPS=1, which this tool sets for itself; the lines are read back from its own stderr);
  - the yardstick, where the dense form fits (`--yardstick-candidates`, 65 536 by default): `jaro_counts_cross` / `lcs_cross` into host
    matrices, the similarity in numpy (engines.py's expressions) and `argpartition` + a sort of the k kept, timed as one; its rows are
    compared with the search's (same scores; same indices wherever the k-th score is not tied).
`--within CUTOFF` measures the score range search (`engine.extract_within`) on the same batch instead: the counting call and the filled
call (device arrays of exactly the counted size), their hit total, and from one profiled filled call the kernel time with its split into
the scoring kernel (`dominant_ms` of `extract_within/<kernel>`: both walks) and the rest. Beside it stands the scoring time of one
`extract` call on the same shape and scorer: a filled call scores the pairs twice, so twice that figure is what it is compared with.
Prints one JSON object per (shape, scorer); `--out` appends them to a jsonl file."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SYLLABLES = ("an", "ber", "chi", "da", "el", "fi", "gar", "ho", "is", "jo", "ka", "li", "mar", "na", "ol", "pe", "qu", "ro", "son", "ti", "ul",
             "vi", "wa", "xe", "yo", "z", "sch", "th", "ng", "e", "a", "o")


def names(count, seed):
    """`count` name-like byte strings of 5 .. 25 bytes: syllables up to a drawn length, some with a second word."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(5, 26, count)
    picks = rng.integers(0, len(SYLLABLES), (count, 14))
    spaces = rng.integers(0, 4, count)
    out = []
    for size, row, space in zip(lengths.tolist(), picks.tolist(), spaces.tolist()):
        text = "".join(SYLLABLES[i] for i in row)
        if space == 0 and size > 9:
            text = text[:size // 2] + " " + text[size // 2:]
        out.append(text[:size].encode())
    return out


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def stamps_of(call):
    """Runs `call` with the process's stderr in a file and sums the library's stamp lines per kernel: {name: {launches, total_ms}}."""
    split = {}
    with tempfile.TemporaryFile() as held:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(held.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        held.seek(0)
        for name, ms in re.findall(r"stamp (\S+)\s+start\s+[\d.]+ ms\s+length\s+([\d.]+) ms", held.read().decode(errors="replace")):
            entry = split.setdefault(name, {"launches": 0, "total_ms": 0.0})
            entry["launches"] += 1
            entry["total_ms"] = round(entry["total_ms"] + float(ms), 4)
    return split


def yardstick(engine, scope, pq, pc, scorer, k, lengths):
    """The dense route: counts into host matrices, the similarity in numpy, the k best per row. Returns (seconds, indices, scores)."""
    t0 = time.perf_counter()
    if scorer == "ratio":
        indel = engine.indel_cross(pq, pc, scope)
        scores = engine._ratio(indel, engine.lcs_cross(pq, pc, scope))
    else:
        matches, transpositions, prefix = engine.jaro_counts_cross(pq, pc, scope)
        scores = engine._winkler(engine._jaro(matches, transpositions, lengths[0][:, None], lengths[1][None, :]), prefix, 0.1)
    part = np.argpartition(-scores, k - 1, axis=1)[:, :k]
    kept = np.take_along_axis(scores, part, axis=1)
    order = np.lexsort((part, -kept), axis=1)
    indices, best = np.take_along_axis(part, order, axis=1), np.take_along_axis(kept, order, axis=1)
    return time.perf_counter() - t0, indices, best


def emit(row, path):
    print(json.dumps(row), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def within_row(sw, torch, engine, scope, pq, pc, scorer, args, count):
    """One (shape, scorer) of `--within`: the counting call, the filled call, one profiled filled call, and extract's scoring time."""
    offsets = torch.empty(args.queries + 1, dtype=torch.int64, device="cuda")
    counting = lambda: engine.extract_within(pq, pc, scope, scorer=scorer, cutoff=args.within, out=(offsets, None, None))
    total = int(counting().offsets[-1])
    hits = (torch.empty(max(total, 1), dtype=torch.int32, device="cuda"), torch.empty(max(total, 1), dtype=torch.float64, device="cuda"))
    filled = lambda: engine.extract_within(pq, pc, scope, scorer=scorer, cutoff=args.within, out=(offsets, hits[0], hits[1]))
    filled()
    row = {"bench": "extract_within", "scorer": scorer, "cutoff": args.within, "queries": args.queries, "candidates": count,
           "pairs": args.queries * count, "hits": total, "count_ms": median_ms(counting, args.reps), "filled_ms": median_ms(filled, args.reps)}
    top = (torch.empty((args.queries, args.k), dtype=torch.int32, device="cuda"), torch.empty((args.queries, args.k), dtype=torch.float64, device="cuda"))
    ranked = lambda: engine.extract(pq, pc, scope, scorer=scorer, k=args.k, out=top)
    ranked()
    scope.set_profiling(True)
    try:
        split = stamps_of(filled)
        timing = scope.last_timing()
        stamps_of(ranked)   # (its stamp lines are not this mode's subject)
        extract_timing = scope.last_timing()
    finally:
        scope.set_profiling(False)
    row.update(kernel=timing["dominant_name"], kernels=timing["kernels"], cells=timing["cells"], kernels_ms=timing["compute_ms"],
               scoring_ms=timing["dominant_ms"], compaction_and_rest_ms=timing["compute_ms"] - timing["dominant_ms"],
               scoring_share=timing["dominant_ms"] / timing["compute_ms"] if timing["compute_ms"] else None, kernel_split_ms=split,
               extract_kernel=extract_timing["dominant_name"], extract_scoring_ms=extract_timing["dominant_ms"],
               twice_extract_scoring_ms=2 * extract_timing["dominant_ms"],
               mpairs_per_s=row["pairs"] / (row["filled_ms"] * 1e-3) / 1e6)
    return row


def main():
    os.environ.setdefault("STRINGWARS_AMD_STAMPS", "1")   # read by the library once, at its first profiled call
    import torch
    import stringwars_amd as sw
    parser = argparse.ArgumentParser()
    parser.add_argument("--queries", type=int, default=4096)
    parser.add_argument("--candidates", type=int, nargs="+", default=[65536, 1 << 20])
    parser.add_argument("--yardstick-candidates", type=int, default=65536, help="the dense route runs on shapes up to this many candidates")
    parser.add_argument("--scorers", nargs="+", default=["jaro_winkler", "ratio"])
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--reps", type=int, default=3)
    parser.add_argument("--within", type=float, default=None, metavar="CUTOFF", help="measure extract_within at this cutoff instead of extract")
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    queries = names(args.queries, 1)
    pq = sw.PreparedTape(scope, sw.Strs(queries))
    for count in args.candidates:
        candidates = names(count, 2)
        pc = sw.PreparedTape(scope, sw.Strs(candidates))
        lengths = (np.array([len(s) for s in queries], dtype=np.float64), np.array([len(s) for s in candidates], dtype=np.float64))
        for scorer in args.scorers:
            if args.within is not None:
                emit(within_row(sw, torch, engine, scope, pq, pc, scorer, args, count), args.out)
                continue
            out = (torch.empty((args.queries, args.k), dtype=torch.int32, device="cuda"), torch.empty((args.queries, args.k), dtype=torch.float64, device="cuda"))
            call = lambda: engine.extract(pq, pc, scope, scorer=scorer, k=args.k, out=out)
            call()
            row = {"bench": "extract", "scorer": scorer, "queries": args.queries, "candidates": count, "k": args.k, "pairs": args.queries * count,
                   "search_ms": median_ms(call, args.reps)}
            scope.set_profiling(True)
            try:
                split = stamps_of(call)
                timing = scope.last_timing()
            finally:
                scope.set_profiling(False)
            row.update(kernel=timing["dominant_name"], kernels=timing["kernels"], cells=timing["cells"], kernels_ms=timing["compute_ms"],
                       scoring_ms=timing["dominant_ms"], fold_and_rest_ms=timing["compute_ms"] - timing["dominant_ms"],
                       scoring_share=timing["dominant_ms"] / timing["compute_ms"] if timing["compute_ms"] else None,
                       kernel_split_ms=split, gcups=timing["cells"] / (row["search_ms"] * 1e-3) / 1e9, mpairs_per_s=row["pairs"] / (row["search_ms"] * 1e-3) / 1e6)
            if count <= args.yardstick_candidates:
                seconds, indices, best = yardstick(engine, scope, pq, pc, scorer, args.k, lengths)
                got_i, got_s = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy()
                row.update(yardstick_ms=seconds * 1e3, search_vs_yardstick=seconds * 1e3 / row["search_ms"],
                           scores_equal=bool((got_s.view(np.uint64) == best.view(np.uint64)).all()),
                           indices_equal_share=float((got_i == indices).mean()))
            emit(row, args.out)


if __name__ == "__main__":
    main()
