"""Top-k search against the dense cross-product on the same inputs (MI355X).

For 2048 x 2048 word-sized strings (`short_words`) and 2048 x 2048 tokens of ~64 bytes (`tokens64`), prepared tapes, device outputs:
  - the dense call (`swh_levenshtein_cross_prepared`, 64-bit matrix in device memory): call time and kernel time;
  - the top-k call at several k: call time, kernel time (`cross_topk` + `topk_merge`, or the general path) and the dominant kernel;
  - the same with the candidates in an adversarial order: sorted by decreasing mean distance to the queries, so the lists keep
    improving and every chunk admits entries.
Then one search no dense call can run: 65 536 queries x 1 M words, k = 10 (TCUPS = nominal cells / kernel time).
Kernel times come from the library's hipEvent profiling (`scope.last_timing()`); call times are host wall clock, medians.
STRINGWARS_AMD_TOPK_PRUNE=0 with the test library (STRINGWARS_AMD_LIBRARY=.../libstringwars_amd_test.so) measures without the
length-bound prune. Prints one JSON object; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def kernel_ms(scope, fn, reps):
    scope.set_profiling(True)
    totals, names, cells = [], [], 0
    try:
        for _ in range(reps):
            fn()
            t = scope.last_timing()
            totals.append(t["total_ms"])
            names.append(t["dominant_name"])
            cells = t["cells"]
    finally:
        scope.set_profiling(False)
    return float(np.median(totals)), names[-1], cells


def main():
    import torch
    import stringwars_amd as sw
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--big-queries", type=int, default=65536)
    parser.add_argument("--big-candidates", type=int, default=1 << 20)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    result = {"prune": os.environ.get("STRINGWARS_AMD_TOPK_PRUNE", "1"), "shapes": []}
    for workload in ("short_words", "tokens64"):
        queries, candidates = sw.generate_pairs(workload, 2048, seed=42)
        pq = sw.PreparedTape(scope, queries)
        matrix = torch.empty((2048, 2048), dtype=torch.int64, device="cuda")
        orders = {"random": candidates}
        engine(pq, sw.PreparedTape(scope, candidates), scope, out=matrix)
        mean = matrix.float().mean(dim=0).cpu().numpy()
        order = np.argsort(-mean, kind="stable")
        orders["adversarial"] = sw.Strs([candidates[int(i)] for i in order])
        for name, cands in orders.items():
            pc = sw.PreparedTape(scope, cands)
            dense = lambda: engine(pq, pc, scope, out=matrix)
            entry = {"workload": workload, "order": name, "queries": 2048, "candidates": 2048,
                     "dense_call_ms": median_ms(dense, args.reps)}
            entry["dense_kernel_ms"], entry["dense_kernel"], _ = kernel_ms(scope, dense, args.reps)
            entry["topk"] = []
            for k in (1, 4, 16, 64):
                out = (torch.empty((2048, k), dtype=torch.int32, device="cuda"), torch.empty((2048, k), dtype=torch.int32, device="cuda"))
                call = lambda k=k, out=out: engine.topk(pq, pc, scope, k=k, out=out)
                row = {"k": k, "call_ms": median_ms(call, args.reps)}
                row["kernel_ms"], row["kernel"], row["cells"] = kernel_ms(scope, call, args.reps)
                row["kernel_vs_dense"] = row["kernel_ms"] / entry["dense_kernel_ms"]
                row["call_vs_dense"] = row["call_ms"] / entry["dense_call_ms"]
                entry["topk"].append(row)
            result["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
    # beyond any dense call: 65 536 x 1 M words, k = 10
    queries, _ = sw.generate_pairs("short_words", args.big_queries, seed=1)
    _, candidates = sw.generate_pairs("short_words", args.big_candidates, seed=2)
    pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
    out = (torch.empty((args.big_queries, 10), dtype=torch.int32, device="cuda"), torch.empty((args.big_queries, 10), dtype=torch.int32, device="cuda"))
    call = lambda: engine.topk(pq, pc, scope, k=10, out=out)
    call()
    big = {"queries": args.big_queries, "candidates": args.big_candidates, "k": 10, "pairs": args.big_queries * args.big_candidates,
           "call_ms": median_ms(call, 3)}
    big["kernel_ms"], big["kernel"], big["cells"] = kernel_ms(scope, call, 3)
    big["tcups"] = big["cells"] / (big["kernel_ms"] * 1e-3) / 1e12
    result["search"] = big
    print(json.dumps(big), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
