"""Infix search for every occurrence (`engine.infix_all`) against the single-occurrence `infix` call on the same tapes (MI355X).

bench_infix.py's two workloads on prepared tapes and one warmed scope:
 (a) 64-symbol byte patterns in 4096-symbol byte texts, half of them planted with a few edits;
 (b) word-sized patterns (a word of the line, sometimes one edit off) in ~1 KB UTF-8 lines, as code points.
bound = m / 8 of the median pattern, at least 1 (one bound per call). For each workload and each select (all, best, minima): the ms of the
counting call (offsets alone, one walk), of the filled call without starts and of the filled call with starts -- host arrays of exactly
the counted size -- each alternated rep by rep with the unchanged `infix` call, medians of host wall clock; the ratio of each to the
`infix` median of its own alternation; the spread of those `infix` medians across the alternations of the run (what the tool itself
cannot tell apart); hits per pair; and from one profiled call of each form the summed event time of every stamped kernel by name (the
library prints them with STRINGWARS_AMD_STAMPS=1, which this tool sets for itself). Prints one JSON object per (workload, select)
and one for the run; `--out` appends them to a JSON-lines file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_extract import stamps_of  # noqa: E402
from bench_infix import byte_workload, line_workload  # noqa: E402

SELECTS = ("all", "best", "minima")


def alternated(reps, call, yardstick):
    """Medians (ms) of `call` and of `yardstick`, run in turns."""
    ours, theirs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ours.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        yardstick()
        theirs.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ours)), float(np.median(theirs))


def main():
    os.environ.setdefault("STRINGWARS_AMD_STAMPS", "1")   # read by the library once, at its first profiled call
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
        lengths = patterns.lengths if not utf8 else [len(bytes(patterns.data[int(patterns.offsets[i]):int(patterns.offsets[i + 1])]).decode())
                                                     for i in range(count)]
        bound = max(1, int(np.median(lengths)) // 8)
        single = lambda: engine.infix(pp, pt, scope, bound=bound)
        found = single()   # warm-up
        infix_medians = []
        for select in SELECTS:
            offsets = np.zeros(count + 1, dtype=np.uint64)
            counting = lambda: engine.infix_all(pp, pt, scope, bound=bound, select=select, out=(offsets, None, None, None))
            total = int(counting().offsets[-1])   # warm-up
            arrays = [np.empty(total, dtype=np.uint32) for _ in range(3)]
            without = lambda: engine.infix_all(pp, pt, scope, bound=bound, select=select, starts=False, out=(offsets, None, arrays[1], arrays[2]))
            filled = lambda: engine.infix_all(pp, pt, scope, bound=bound, select=select, out=(offsets, *arrays))
            got = filled()
            if select == "best" and total:   # the first hit of a BEST row is the infix call's occurrence
                first = offsets[:-1][found.found].astype(np.int64)
                assert (got.ends[first] == found.ends[found.found]).all() and (got.starts[first] == found.starts[found.found]).all(), name
            row = {"workload": name, "pairs": count, "select": select, "bound": bound, "hits": total, "hits_per_pair": round(total / count, 3)}
            for form, call in (("count", counting), ("filled_no_starts", without), ("filled", filled)):
                call_ms, infix_ms = alternated(args.reps, call, single)
                infix_medians.append(infix_ms)
                scope.set_profiling(True)
                try:
                    split = stamps_of(call)
                    timing = scope.last_timing()
                finally:
                    scope.set_profiling(False)
                row[form] = {"ms": round(call_ms, 3), "infix_ms": round(infix_ms, 3), "ratio_to_infix": round(call_ms / infix_ms, 3),
                             "kernel_ms": round(timing["total_ms"], 3), "kernel_split_ms": split}
                row["cells"] = int(timing["cells"])
            rows.append(row)
            print(json.dumps(row), flush=True)
        spread = {"workload": name, "infix_ms_min": round(min(infix_medians), 3), "infix_ms_max": round(max(infix_medians), 3),
                  "infix_spread": round(max(infix_medians) / min(infix_medians) - 1, 4)}
        rows.append(spread)
        print(json.dumps(spread), flush=True)
    result = {"bench": "infix_all", "reps": args.reps, "rows": rows}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "a") as handle:
            handle.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
