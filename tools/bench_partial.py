"""The partial ratio (`engine.partial_counts` / `partial_counts_cross`) against the plain LCS call on the same tapes (MI355X).

Three shapes, prepared tapes, device outputs, synchronous calls with profiling on:
  - words:  1 M pairs, a needle of 4 .. 16 bytes in a haystack of about 64;
  - lines:  100 K pairs, a needle of 64 bytes in a haystack of about 1 KB;
  - cross:  2048 x 2048 strings of about 16 bytes.
Per shape: the call time (host wall clock, median), from one profiled call the kernel time and its split by stamp, and
  - window-columns = the sum over all windows of a pair (both directions where the lengths are equal) of the window's length -- what
    the bit-vector kernel walks for the partial ratio, worked out from the lengths alone;
  - columns = the sum of the longer string's length -- what it walks for one LCS;
  - window-columns per second of `partial`, columns per second of `lcs` on the same tapes in the same process, and their ratio.
Nothing is asserted about the ratio: it is recorded. Prints one JSON object per shape; `--out` appends them to a jsonl file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window_columns(la, lb):
    """Sum over the n + m - 1 windows of their lengths: m (n - m + 1) for the full windows, m (m - 1) for the two overhanging runs of
    1 .. m - 1 symbols; twice where the lengths are equal (both directions run). la, lb: int64 arrays that broadcast."""
    m, n = np.minimum(la, lb), np.maximum(la, lb)
    one_way = m * (n - m + 1) + m * (m - 1)
    return np.where(la == lb, 2 * one_way, one_way)


def random_strings(rng, lengths, alphabet=26):
    data = (rng.integers(0, alphabet, int(lengths.sum())) + 97).astype(np.uint8).tobytes()
    ends = np.cumsum(lengths)
    return [data[e - k:e] for e, k in zip(ends.tolist(), lengths.tolist())]


def shapes(args):
    rng = np.random.default_rng(12)
    words = int(args.scale * (1 << 20))
    lines = int(args.scale * 100_000)
    side = max(1, int(2048 * min(1.0, args.scale) ** 0.5))
    yield "words", False, rng.integers(4, 17, words), rng.integers(48, 81, words)
    yield "lines", False, np.full(lines, 64), rng.integers(896, 1153, lines)
    yield "cross", True, rng.integers(8, 25, side), rng.integers(8, 25, side)


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def profiled(scope, call):
    scope.set_profiling(True)
    try:
        call()
        return scope.last_timing()
    finally:
        scope.set_profiling(False)


def main():
    import torch
    import stringwars_amd as sw
    parser = argparse.ArgumentParser()
    parser.add_argument("--scale", type=float, default=1.0, help="of the pair counts (and of the cross-product's area)")
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    rng = np.random.default_rng(13)
    for name, cross, la, lb in shapes(args):
        la, lb = la.astype(np.int64), lb.astype(np.int64)
        pa, pb = sw.PreparedTape(scope, sw.Strs(random_strings(rng, la))), sw.PreparedTape(scope, sw.Strs(random_strings(rng, lb)))
        shape = (len(la), len(lb)) if cross else (len(la),)
        dtype = torch.int64 if cross else torch.int32
        outs = tuple(torch.empty(shape, dtype=dtype, device="cuda") for _ in range(4))
        if cross:
            partial = lambda: engine.partial_counts_cross(pa, pb, scope, out=outs)
            lcs = lambda: engine.lcs_cross(pa, pb, scope, out=outs[0])
            wcols = int(window_columns(la[:, None], lb[None, :]).sum())
            cols = int(np.maximum(la[:, None], lb[None, :]).sum())
        else:
            partial = lambda: engine.partial_counts(pa, pb, scope, out=outs)
            lcs = lambda: engine.lcs(pa, pb, scope, out=outs[0])
            wcols = int(window_columns(la, lb).sum())
            cols = int(np.maximum(la, lb).sum())
        partial(); lcs()
        scope.set_profiling(True)
        try:
            partial_ms, lcs_ms = median_ms(partial, args.reps), median_ms(lcs, args.reps)
        finally:
            scope.set_profiling(False)
        timing, lcs_timing = profiled(scope, partial), profiled(scope, lcs)
        row = {"bench": "partial", "shape": name, "pairs": int(np.prod(shape)), "reps": args.reps,
               "partial_ms": partial_ms, "lcs_ms": lcs_ms, "window_columns": wcols, "lcs_columns": cols,
               "partial_kernel": timing["dominant_name"], "partial_kernels": timing["kernels"], "partial_kernels_ms": timing["compute_ms"],
               "partial_scoring_ms": timing["dominant_ms"], "lcs_kernel": lcs_timing["dominant_name"], "lcs_scoring_ms": lcs_timing["dominant_ms"],
               "cells": timing["cells"],
               "window_columns_per_s": wcols / (partial_ms * 1e-3), "lcs_columns_per_s": cols / (lcs_ms * 1e-3)}
        row["window_columns_vs_lcs_columns_per_s"] = row["window_columns_per_s"] / row["lcs_columns_per_s"]
        # the same ratio on the scoring kernels alone, where the LCS call's longest kernel is its scoring kernel (on short strings it is
        # the sizes kernel: there is no such figure then)
        if timing["dominant_name"].startswith("partial") and lcs_timing["dominant_name"].startswith("lcs") and lcs_timing["dominant_ms"]:
            row["kernel_window_columns_vs_lcs_columns_per_s"] = (wcols / timing["dominant_ms"]) / (cols / lcs_timing["dominant_ms"])
        print(json.dumps(row), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
