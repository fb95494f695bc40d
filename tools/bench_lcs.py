"""Indel distances (LCS) against the unit-cost `pairs` call and against the general-cost route to the same numbers (MI355X).

Three workloads on prepared tapes and one warmed scope:
 (a) `tokens64`: 1 M pairs of the 64-byte tokens of the headline configuration;
 (b) `utf8_lines`: 100 K pairs of ~1 KB UTF-8 lines, scored over code points;
 (c) `acgt100_cross`: the 2048 x 2048 cross-product of 100-symbol strings over ACGT.
For each, alternated rep by rep on the same tapes: the new `indel` call, the unit-cost `pairs` (or cross) call, and
`LevenshteinDistances(0, 2, 1, 1).pairs` (or cross) -- the only route to an Indel distance without the LCS kernel, whose results
must equal the `indel` call's. Medians and quartiles of synchronous host wall clock, TCUPS, and the profiled kernel time of
`k_lcs` and, on the same tapes, of `k_osa` (the two share layout and planner, so their times per cell compare the column loops).
Prints one JSON object per workload and one for the run; `--out` also writes it to a file. A kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def acgt_tape(sw, count, rng):
    rows = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(count, 100))]
    return sw.Strs(data=rows.reshape(-1), offsets=np.arange(count + 1, dtype=np.uint64) * 100)


def profiled(scope, call, reps):
    """last_timing of `reps` profiled calls: the dominant kernel's name and its times."""
    scope.set_profiling(True)
    try:
        timings = []
        for _ in range(reps):
            call()
            timings.append(scope.last_timing())
        return timings
    finally:
        scope.set_profiling(False)


def quartiles(values):
    q1, q2, q3 = np.percentile(np.asarray(values, dtype=np.float64), (25, 50, 75))
    return {"median": round(float(q2), 4), "q1": round(float(q1), 4), "q3": round(float(q3), 4)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--scale", type=float, default=1.0, help="multiply every workload's pair count (the cross-product: its side by the root)")
    parser.add_argument("--out")
    args = parser.parse_args()
    import stringwars_amd as sw

    scope = sw.DeviceScope(gpu_device=0)
    rng = np.random.default_rng(42)
    rows = []
    for name, count, utf8, cross in (("tokens64", 1_000_000, False, False), ("utf8_lines", 100_000, True, False), ("acgt100_cross", 2048, False, True)):
        count = max(1, int(count * (args.scale ** 0.5 if cross else args.scale)))
        make = sw.LevenshteinDistancesUTF8 if utf8 else sw.LevenshteinDistances
        unit, costly = make(capabilities=scope), make(0, 2, 1, 1, capabilities=scope)
        if cross:
            a, b = acgt_tape(sw, count, rng), acgt_tape(sw, count, rng)
        else:
            a, b = sw.generate_pairs(name, count, seed=42)
        pa, pb = sw.PreparedTape(scope, a, utf8=utf8), sw.PreparedTape(scope, b, utf8=utf8)
        calls = {
            "indel": (lambda: unit.indel_cross(pa, pb, scope)) if cross else (lambda: unit.indel(pa, pb, scope)),
            "pairs": (lambda: unit(pa, pb, scope)) if cross else (lambda: unit.pairs(pa, pb, scope)),
            "general_cost": (lambda: costly(pa, pb, scope)) if cross else (lambda: costly.pairs(pa, pb, scope)),
            "osa": (lambda: unit.osa_cross(pa, pb, scope)) if cross else (lambda: unit.osa(pa, pb, scope)),
        }
        # warm-up of every call, and the check: two unrelated kernels, one answer
        first = {key: call() for key, call in calls.items()}
        assert (first["indel"] == first["general_cost"]).all(), name
        assert (first["pairs"] <= first["indel"]).all() and (first["indel"] <= 2 * first["pairs"].astype(np.uint64)).all(), name
        ms = {key: [] for key in ("indel", "pairs", "general_cost")}
        for _ in range(args.reps):
            for key in ms:
                t0 = time.perf_counter()
                calls[key]()
                ms[key].append((time.perf_counter() - t0) * 1e3)
        lcs_timing = profiled(scope, calls["indel"], args.reps)
        osa_timing = profiled(scope, calls["osa"], args.reps)
        cells = int(lcs_timing[0]["cells"])
        # (on a million 64-byte pairs k_osa_sizes, which cuts the items of both families, outlasts k_lcs: the row says whose time it holds)
        dominant = [lcs_timing[0]["dominant_name"], osa_timing[0]["dominant_name"]]
        assert dominant[0] in ("lcs_u32" if utf8 else "lcs", "osa_sizes") and dominant[1] in ("osa_u32" if utf8 else "osa", "osa_sizes"), dominant
        assert osa_timing[0]["cells"] == cells
        k_lcs, k_osa = quartiles([t["dominant_ms"] for t in lcs_timing]), quartiles([t["dominant_ms"] for t in osa_timing])
        row = {"workload": name, "pairs": count * count if cross else count, "cells": cells, "symbols": "code points" if utf8 else "bytes"}
        for key in ms:
            row[key + "_ms"] = quartiles(ms[key])
        row.update({
            "indel_tcups": round(cells / (row["indel_ms"]["median"] * 1e-3) / 1e12, 3),
            "indel_over_general_cost": round(row["indel_ms"]["median"] / row["general_cost_ms"]["median"], 3),
            "indel_over_pairs": round(row["indel_ms"]["median"] / row["pairs_ms"]["median"], 3),
            "k_lcs_ms": k_lcs, "k_osa_ms": k_osa, "dominant": dominant,
            "k_lcs_tcups": round(cells / (k_lcs["median"] * 1e-3) / 1e12, 3),
            "k_lcs_over_k_osa_per_cell": round(k_lcs["median"] / k_osa["median"], 3),
            "lcs_call_kernels_ms": round(float(np.median([t["total_ms"] for t in lcs_timing])), 4),
        })
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pa, pb, first
    result = {"bench": "lcs", "reps": args.reps, "rows": rows}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
