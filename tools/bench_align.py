"""Alignments against distances on the same inputs (MI355X).

For each shape, on prepared tapes and one warmed scope: the ms of a synchronous `align` call (host outputs: distances, offsets and
ops) and of a `pairs` call (host distances), the two alternated rep by rep, medians of host wall clock. Reports their ratio, the
cells (sum len(a_i) len(b_i)) per second of `align`, and the dominant kernel of one profiled `align` call. Prints one JSON object;
`--out` also writes it to a file. The kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (("tokens64", 1_000_000, False), ("short_words", 1_000_000, False), ("utf8_lines", 10_000, True), ("protein4k", 1_000, False))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--scale", type=float, default=1.0, help="multiply every shape's pair count")
    parser.add_argument("--out")
    args = parser.parse_args()
    import stringwars_amd as sw

    scope = sw.DeviceScope(gpu_device=0)
    rows = []
    for workload, count, utf8 in SHAPES:
        count = max(1, int(count * args.scale))
        a, b = sw.generate_pairs(workload, count, seed=42)
        engine = (sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances)(capabilities=scope)
        pa, pb = sw.PreparedTape(scope, a, utf8=utf8), sw.PreparedTape(scope, b, utf8=utf8)
        got = engine.align(pa, pb, scope)   # warm-up of both calls
        assert (got.distances == engine.pairs(pa, pb, scope)).all(), workload
        align_ms, pairs_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            engine.align(pa, pb, scope)
            align_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            engine.pairs(pa, pb, scope)
            pairs_ms.append((time.perf_counter() - t0) * 1e3)
        scope.set_profiling(True)
        try:
            engine.align(pa, pb, scope)
            timing = scope.last_timing()
        finally:
            scope.set_profiling(False)
        am, pm = float(np.median(align_ms)), float(np.median(pairs_ms))
        rows.append({"shape": workload, "pairs": count, "align_ms": round(am, 3), "pairs_ms": round(pm, 3), "ratio": round(am / pm, 2),
                     "align_gcups": round(timing["cells"] / (am * 1e-3) / 1e9, 2), "cells": int(timing["cells"]),
                     "align_kernel_ms": round(timing["total_ms"], 3), "dominant": timing["dominant_name"],
                     "dominant_ms": round(timing["dominant_ms"], 3), "ops": int(got.offsets[-1])})
        print(json.dumps(rows[-1]), flush=True)
    result = {"bench": "align", "reps": args.reps, "rows": rows}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
