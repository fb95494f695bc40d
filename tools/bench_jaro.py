"""Jaro / Jaro-Winkler counts against the LCS call on the same tapes (MI355X). Reports; sets no threshold.

Three workloads on prepared tapes and one warmed scope:
 (a) `tokens64`: 1 M pairs of the 64-byte tokens of the headline configuration;
 (b) `words16`: 1 M pairs of word-sized strings -- names and words, one lane per pair;
 (c) `acgt100_cross`: the 2048 x 2048 cross-product of 100-symbol strings over ACGT.
For each, alternated rep by rep on the same tapes: the `jaro_counts` call (all three outputs) and the `lcs` call -- the two kernels
share layout and item shape, so their times per cell compare the column loops, and k_jaro has its second pass on top. Medians and
quartiles of synchronous host wall clock, and the profiled kernel times of `k_jaro` and `k_lcs` with their ratio (a call of two
kernels names only its longest, so the other is the rest of the call; a cross-product that ran in slices reports the sum of its
kernels instead). The warm-up checks only what the counts can be (M <= min(m, n), 2 t <= M, prefix <= 4): tests/test_jaro.py holds
the kernel against its references. Prints one JSON object per workload and one for the run; `--out` also
writes it to a file."""
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


def call_kernels(timings):
    """What the profile says of one call: its kernels, their summed time, and the longest of them."""
    return {"kernels": timings[0]["kernels"], "kernels_ms": quartiles([t["total_ms"] for t in timings]),
            "dominant_name": timings[0]["dominant_name"], "dominant_ms": quartiles([t["dominant_ms"] for t in timings])}


def kernel_ms(timings, name):
    """The time of the counting kernel `name` in calls of two kernels (the measuring one and it): the longest kernel where it is
    that, the rest of the call where the measuring kernel is the longest. None for calls that ran in slices."""
    if any(t["kernels"] != 2 for t in timings):
        return None
    return quartiles([t["dominant_ms"] if t["dominant_name"] == name else t["total_ms"] - t["dominant_ms"] for t in timings])


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--scale", type=float, default=1.0, help="multiply every workload's pair count (the cross-product: its side by the root)")
    parser.add_argument("--out")
    args = parser.parse_args()
    import stringwars_amd as sw

    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    rng = np.random.default_rng(42)
    rows = []
    for name, count, cross in (("tokens64", 1_000_000, False), ("words16", 1_000_000, False), ("acgt100_cross", 2048, True)):
        count = max(1, int(count * (args.scale ** 0.5 if cross else args.scale)))
        if cross:
            a, b = acgt_tape(sw, count, rng), acgt_tape(sw, count, rng)
        else:
            a, b = sw.generate_pairs(name, count, seed=42)
        pa, pb = sw.PreparedTape(scope, a), sw.PreparedTape(scope, b)
        calls = {
            "jaro_counts": (lambda: engine.jaro_counts_cross(pa, pb, scope)) if cross else (lambda: engine.jaro_counts(pa, pb, scope)),
            "lcs": (lambda: engine.lcs_cross(pa, pb, scope)) if cross else (lambda: engine.lcs(pa, pb, scope)),
        }
        # warm-up of both calls, and a check of what the counts can be
        matches, transpositions, prefix = calls["jaro_counts"]()
        calls["lcs"]()
        la, lb = a.lengths.astype(np.uint64), b.lengths.astype(np.uint64)
        shorter = np.minimum(la[:, None], lb[None, :]) if cross else np.minimum(la, lb)
        assert (matches <= shorter).all() and (2 * transpositions.astype(np.uint64) <= matches).all() and (prefix <= 4).all(), name
        ms = {key: [] for key in calls}
        for _ in range(args.reps):
            for key in ms:
                t0 = time.perf_counter()
                calls[key]()
                ms[key].append((time.perf_counter() - t0) * 1e3)
        jaro_timing = profiled(scope, calls["jaro_counts"], args.reps)
        lcs_timing = profiled(scope, calls["lcs"], args.reps)
        cells = int(jaro_timing[0]["cells"])
        assert lcs_timing[0]["cells"] == cells
        k_jaro, k_lcs = kernel_ms(jaro_timing, "jaro"), kernel_ms(lcs_timing, "lcs")
        row = {"workload": name, "pairs": count * count if cross else count, "cells": cells, "symbols": "bytes"}
        for key in ms:
            row[key + "_ms"] = quartiles(ms[key])
        row.update({
            "jaro_counts_mpairs_per_s": round(row["pairs"] / (row["jaro_counts_ms"]["median"] * 1e-3) / 1e6, 2),
            "jaro_counts_over_lcs": round(row["jaro_counts_ms"]["median"] / row["lcs_ms"]["median"], 3),
            "jaro_call": call_kernels(jaro_timing), "lcs_call": call_kernels(lcs_timing),
            "k_jaro_ms": k_jaro, "k_lcs_ms": k_lcs,
            "k_jaro_over_k_lcs": round(k_jaro["median"] / k_lcs["median"], 3) if k_jaro and k_lcs else None,
        })
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pa, pb
    result = {"bench": "jaro", "reps": args.reps, "rows": rows}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
