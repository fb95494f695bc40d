"""Infix search against global distances on the same tapes (MI355X).

Two workloads on prepared tapes and one warmed scope:
 (a) 64-symbol byte patterns in 4096-symbol byte texts, half of them planted with a few edits;
 (b) word-sized patterns (a word of the line, sometimes one edit off) in ~1 KB UTF-8 lines, as code points.
For each: the ms of a synchronous `infix` call (host outputs) and of a `pairs` call on the same tapes -- the nominal cells, sum m n,
are the same -- alternated rep by rep, medians of host wall clock; their ratio, the TCUPS of `infix` over sum m n, and the kernels
of one profiled `infix` call. Prints one JSON object per workload and one for the run; `--out` also writes it to a file. The kernel
split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def byte_workload(sw, count, rng):
    """(a): 64-symbol patterns over 20 letters in 4096-symbol texts; every second text holds its pattern with up to three substitutions."""
    patterns = rng.integers(97, 117, size=(count, 64)).astype(np.uint8)
    texts = rng.integers(97, 117, size=(count, 4096)).astype(np.uint8)
    at = rng.integers(0, 4096 - 64, size=count)
    for i in range(0, count, 2):
        planted = patterns[i].copy()
        planted[rng.integers(0, 64, size=3)] = rng.integers(97, 117, size=3)
        texts[i, at[i]:at[i] + 64] = planted
    tape = lambda rows: sw.Strs(data=rows.reshape(-1), offsets=(np.arange(len(rows) + 1, dtype=np.uint64) * rows.shape[1]))
    return tape(patterns), tape(texts)


def line_workload(sw, count, rng):
    """(b): the lines of the `utf8_lines` generator; pattern i is a word of line i, every third one with a symbol replaced."""
    lines, _ = sw.generate_pairs("utf8_lines", count, seed=42)
    texts, patterns = [], []
    for i in range(count):
        line = bytes(lines.data[int(lines.offsets[i]):int(lines.offsets[i + 1])]).decode("utf-8")
        words = [w for w in line.split() if len(w) >= 3] or [line[:8]]
        word = words[int(rng.integers(0, len(words)))]
        if i % 3 == 0 and word:
            k = int(rng.integers(0, len(word)))
            word = word[:k] + "#" + word[k + 1:]
        texts.append(line); patterns.append(word)
    return sw.Strs(patterns), sw.Strs(texts)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--scale", type=float, default=1.0, help="multiply every workload's pair count")
    parser.add_argument("--out")
    args = parser.parse_args()
    import stringwars_amd as sw

    scope = sw.DeviceScope(gpu_device=0)
    rng = np.random.default_rng(42)
    rows = []
    for name, make, count, utf8 in (("bytes_64_in_4096", byte_workload, 20_000, False), ("utf8_word_in_line", line_workload, 10_000, True)):
        count = max(1, int(count * args.scale))
        patterns, texts = make(sw, count, rng)
        engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
        pp, pt = sw.PreparedTape(scope, patterns, utf8=utf8), sw.PreparedTape(scope, texts, utf8=utf8)
        got = engine.infix(pp, pt, scope)   # warm-up of both calls
        whole = engine.pairs(pp, pt, scope)
        assert (got.distances <= whole).all(), name
        infix_ms, pairs_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            engine.infix(pp, pt, scope)
            infix_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            engine.pairs(pp, pt, scope)
            pairs_ms.append((time.perf_counter() - t0) * 1e3)
        scope.set_profiling(True)
        try:
            engine.infix(pp, pt, scope)
            timing = scope.last_timing()
        finally:
            scope.set_profiling(False)
        im, pm = float(np.median(infix_ms)), float(np.median(pairs_ms))
        rows.append({"workload": name, "pairs": count, "infix_ms": round(im, 3), "pairs_ms": round(pm, 3), "ratio_to_pairs": round(im / pm, 2),
                     "infix_tcups": round(timing["cells"] / (im * 1e-3) / 1e12, 3), "cells": int(timing["cells"]),
                     "infix_kernel_ms": round(timing["total_ms"], 3), "dominant": timing["dominant_name"],
                     "dominant_ms": round(timing["dominant_ms"], 3), "exact": int((got.distances == 0).sum()),
                     "mean_distance": round(float(got.distances.mean()), 2)})
        print(json.dumps(rows[-1]), flush=True)
    result = {"bench": "infix", "reps": args.reps, "rows": rows}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
