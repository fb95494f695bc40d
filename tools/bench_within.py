"""Range search (`engine.within`) against the two older ways to the same answer, on the same inputs (MI355X).

For `short_words` at 2048 x 2048, 65 536 x 1 M and 1 M x 65 536, bounds 1, 2 and 4, prepared tapes, device outputs:
  - the counting call (NULL, NULL, 0: one walk, the row offsets);
  - the full call with arrays of exactly the counted size (two walks), when the hits fit `--max-hits`;
  - `topk(k=64, bound)` -- which loses the 65th neighbour -- and `topk(k=1, bound)`, the cheapest exit of the same walk;
  - the dense cross-product + `torch.nonzero(matrix <= bound)` on the device, where the dense call is allowed (under 2^32 pairs).
Kernel times come from the library's hipEvent profiling (`scope.last_timing()`), call times are host wall clock, medians.
Prints one JSON line per (shape, bound); `--out` appends them to a .jsonl file (profiles/r7/within_table.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((2048, 2048), (65536, 1 << 20), (1 << 20, 65536))
BOUNDS = (1, 2, 4)


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def kernel_ms(scope, fn, reps):
    scope.set_profiling(True)
    totals, name, cells = [], "", 0
    try:
        for _ in range(reps):
            fn()
            t = scope.last_timing()
            totals.append(t["total_ms"])
            name, cells = t["dominant_name"], t["cells"]
    finally:
        scope.set_profiling(False)
    return float(np.median(totals)), name, cells


def main():
    import torch
    import stringwars_amd as sw
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=10, help="repetitions at 2048 x 2048; the large shapes take a third of them, at least 3")
    parser.add_argument("--max-hits", type=int, default=1 << 30, help="the full call is measured only when the hits number at most this")
    parser.add_argument("--shapes", default=None, help="e.g. 2048x2048,65536x1048576")
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    shapes = SHAPES if args.shapes is None else tuple(tuple(int(n) for n in s.split("x")) for s in args.shapes.split(","))
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    for nq, nc in shapes:
        queries, _ = sw.generate_pairs("short_words", nq, seed=1)
        _, candidates = sw.generate_pairs("short_words", nc, seed=2)
        pq, pc = sw.PreparedTape(scope, queries), sw.PreparedTape(scope, candidates)
        reps = args.reps if nq * nc <= 1 << 24 else max(3, args.reps // 3)
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        topk_out = {k: (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.int32, device="cuda")) for k in (1, 64)}
        dense = torch.empty((nq, nc), dtype=torch.int64, device="cuda") if nq * nc < 1 << 32 and nq * nc * 8 <= 1 << 32 else None
        for bound in BOUNDS:
            count = lambda: engine.within(pq, pc, scope, bound=bound, out=(offsets, None, None))
            count()
            total = int(offsets[-1])
            row = {"workload": "short_words", "queries": nq, "candidates": nc, "bound": bound, "hits": total, "reps": reps,
                   "rows_over_64_hits": int((torch.diff(offsets) > 64).sum())}
            row["count_call_ms"] = median_ms(count, reps)
            row["count_kernel_ms"], row["kernel"], row["cells"] = kernel_ms(scope, count, reps)
            row["count_tcups"] = row["cells"] / (row["count_kernel_ms"] * 1e-3) / 1e12
            if 0 < total <= args.max_hits:
                out = (offsets, torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda"))
                full = lambda: engine.within(pq, pc, scope, bound=bound, out=out)
                row["full_call_ms"] = median_ms(full, reps)
                row["full_kernel_ms"], _, _ = kernel_ms(scope, full, reps)
                row["full_vs_count"] = row["full_kernel_ms"] / row["count_kernel_ms"]
                del out
            else:
                row["full_call_ms"] = row["full_kernel_ms"] = row["full_vs_count"] = None   # more hits than --max-hits: not filled
            for k in (1, 64):
                call = lambda k=k: engine.topk(pq, pc, scope, k=k, bound=bound, out=topk_out[k])
                row[f"topk{k}_call_ms"] = median_ms(call, reps)
                row[f"topk{k}_kernel_ms"], _, _ = kernel_ms(scope, call, reps)
            row["count_vs_topk1"] = row["count_kernel_ms"] / row["topk1_kernel_ms"]
            if dense is not None:
                def filtered():
                    engine(pq, pc, scope, out=dense)
                    hits = torch.nonzero(dense <= bound)
                    torch.cuda.synchronize()
                    return hits
                assert len(filtered()) == total
                row["dense_nonzero_call_ms"] = median_ms(filtered, reps)
            else:
                row["dense_nonzero_call_ms"] = None   # the dense call refuses 2^32 pairs or more (and 8 bytes a pair would not fit)
            print(json.dumps(row), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
