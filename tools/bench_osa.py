"""OSA (restricted Damerau-Levenshtein) distances against plain Levenshtein distances on the same tapes (MI355X).

Three workloads on prepared tapes and one warmed scope:
 (a) `tokens64`: the 64-byte tokens of the headline configuration;
 (b) `short_words`: word-sized strings;
 (c) 64-symbol byte strings against 4096-symbol byte strings.
For each: the ms of a synchronous `osa` call (host outputs) and of a `pairs` call on the same tapes -- the cells, sum m n, are the
same -- alternated rep by rep, medians of host wall clock; their ratio, the TCUPS of `osa`, and the kernels of one profiled `osa`
call. On (c) the forward pass of an `infix` call on the same tapes is profiled too: `k_osa` and `k_infix` share layout and planner,
so their kernel times per cell compare the column loops alone. Prints one JSON object per workload and one for the run; `--out` also
writes it to a file. A kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shape_workload(sw, count, rng):
    """(c): 64 symbols over 20 letters against 4096 symbols."""
    short = rng.integers(97, 117, size=(count, 64)).astype(np.uint8)
    long = rng.integers(97, 117, size=(count, 4096)).astype(np.uint8)
    tape = lambda rows: sw.Strs(data=rows.reshape(-1), offsets=(np.arange(len(rows) + 1, dtype=np.uint64) * rows.shape[1]))
    return tape(short), tape(long)


def profiled(scope, call):
    scope.set_profiling(True)
    try:
        call()
        return scope.last_timing()
    finally:
        scope.set_profiling(False)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--scale", type=float, default=1.0, help="multiply every workload's pair count")
    parser.add_argument("--out")
    args = parser.parse_args()
    import stringwars_amd as sw

    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    rng = np.random.default_rng(42)
    rows = []
    for name, count in (("tokens64", 1_000_000), ("short_words", 1_000_000), ("bytes_64_vs_4096", 20_000)):
        count = max(1, int(count * args.scale))
        a, b = shape_workload(sw, count, rng) if name == "bytes_64_vs_4096" else sw.generate_pairs(name, count, seed=42)
        pa, pb = sw.PreparedTape(scope, a), sw.PreparedTape(scope, b)
        got = engine.osa(pa, pb, scope)   # warm-up of both calls
        whole = engine.pairs(pa, pb, scope)
        assert (got <= whole).all() and (whole <= 2 * got.astype(np.uint64)).all(), name
        osa_ms, pairs_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            engine.osa(pa, pb, scope)
            osa_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            engine.pairs(pa, pb, scope)
            pairs_ms.append((time.perf_counter() - t0) * 1e3)
        timing = profiled(scope, lambda: engine.osa(pa, pb, scope))
        om, pm = float(np.median(osa_ms)), float(np.median(pairs_ms))
        row = {"workload": name, "pairs": count, "osa_ms": round(om, 3), "pairs_ms": round(pm, 3), "ratio_to_pairs": round(om / pm, 2),
               "osa_tcups": round(timing["cells"] / (om * 1e-3) / 1e12, 3), "cells": int(timing["cells"]),
               "osa_kernel_ms": round(timing["total_ms"], 3), "dominant": timing["dominant_name"],
               "dominant_ms": round(timing["dominant_ms"], 3), "below_levenshtein": int((got < whole).sum())}
        if name == "bytes_64_vs_4096":
            engine.infix(pa, pb, scope)
            forward = profiled(scope, lambda: engine.infix(pa, pb, scope))
            assert forward["dominant_name"] == "infix" and forward["cells"] == timing["cells"]
            row.update({"infix_forward_ms": round(forward["dominant_ms"], 3),
                        "k_osa_over_k_infix_per_cell": round(timing["dominant_ms"] / forward["dominant_ms"], 2)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"bench": "osa", "reps": args.reps, "rows": rows}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
