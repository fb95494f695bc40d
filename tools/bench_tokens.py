"""The token scorers against the plain ratio call on the same tapes (MI355X).

One shape: 1 M pairs of names of 2 .. 6 words (10 .. 40 bytes), the second name the first with its words shuffled and, in half the
pairs, one word replaced. Prepared tapes, host outputs, synchronous calls. Timed, each as the median host wall clock of `--reps` calls:
  - derive:     `a.token_sorted()` of one tape (the kernel, the scan, the compaction and the measuring of the new tape);
  - token_sort: `engine.token_sort_ratio(a, b)` -- two derivations and the ratio call on the derived tapes;
  - sorted_ratio: `engine.ratio` on two tapes derived beforehand (what a caller pays who derives once and scores often);
  - token_set:  `engine.token_set_ratio(a, b)` -- two unique derivations, the split, two difference tapes and the LCS call on them;
  - ratio:      `engine.ratio(a, b)` on the source tapes: the yardstick, whose code the token scorers do not touch;
  - token_set_counts, lcs_counts: the last two without their float64 expressions on the host (the library calls alone).
From one profiled call each, the kernel time of the derivation and of the split. Nothing is asserted: the figures are recorded, with
derive_vs_ratio = derive / ratio. Prints one JSON object; `--out` appends it to a jsonl file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def names(rng, count):
    """`count` pairs of names as two lists of bytes."""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    vocabulary = [letters[rng.integers(0, 26, int(n))].tobytes() for n in rng.integers(3, 8, 4096)]
    words = rng.integers(2, 7, count)
    picks = rng.integers(0, len(vocabulary), int(words.sum()))
    swaps = rng.integers(0, 2 * len(vocabulary), count)   # half of them name a word
    a, b, at = [], [], 0
    for n, swap in zip(words.tolist(), swaps.tolist()):
        mine = [vocabulary[k] for k in picks[at:at + n]]
        at += n
        while len(b" ".join(mine)) > 40:   # 10 .. 40 bytes, 2 .. 6 words
            mine.pop()
        while len(b" ".join(mine)) < 10:
            mine.append(vocabulary[(swap + len(mine)) % len(vocabulary)])
        other = mine[::-1]
        if swap < len(vocabulary):
            other[0] = vocabulary[swap]
        a.append(b" ".join(mine))
        b.append(b" ".join(other))
    return a, b


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
    import stringwars_amd as sw
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=1 << 20)
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    scope = sw.DeviceScope(gpu_device=0)
    engine = sw.LevenshteinDistances(capabilities=scope)
    a, b = names(np.random.default_rng(14), args.pairs)
    lengths = np.array([len(x) for x in a])
    pa, pb = sw.PreparedTape(scope, sw.Strs(a)), sw.PreparedTape(scope, sw.Strs(b))
    sa, sb = pa.token_sorted(), pb.token_sorted()

    def derive():
        pa.token_sorted().free()

    calls = {"derive": derive, "token_sort": lambda: engine.token_sort_ratio(pa, pb, scope), "sorted_ratio": lambda: engine.ratio(sa, sb, scope),
             "token_set": lambda: engine.token_set_ratio(pa, pb, scope), "token_set_counts": lambda: engine.token_set_counts(pa, pb, scope),
             "ratio": lambda: engine.ratio(pa, pb, scope), "lcs_counts": lambda: engine._lcs_call(pa, pb, scope, False, None, True, True)}
    for call in calls.values():
        call()
    row = {"bench": "tokens", "pairs": args.pairs, "reps": args.reps, "bytes_min": int(lengths.min()), "bytes_mean": float(lengths.mean()),
           "bytes_max": int(lengths.max())}
    for name, call in calls.items():
        row[name + "_ms"] = median_ms(call, args.reps)
    row["derive_vs_ratio"] = row["derive_ms"] / row["ratio_ms"]
    row["token_sort_vs_ratio"] = row["token_sort_ms"] / row["ratio_ms"]
    row["token_set_vs_ratio"] = row["token_set_ms"] / row["ratio_ms"]
    timing = profiled(scope, derive)
    row["derive_kernels_ms"], row["derive_kernel"], row["derive_kernel_ms"] = timing["compute_ms"], timing["dominant_name"], timing["dominant_ms"]
    unique_a, unique_b = pa.token_sorted(unique=True), pb.token_sorted(unique=True)
    sect = np.empty(args.pairs, dtype=np.uint32)   # (without the LCS output: the split alone is the call's last timing)
    timing = profiled(scope, lambda: engine.token_set_counts(unique_a, unique_b, scope, out=(sect, None, None, None)))
    row["split_kernels_ms"], row["split_kernel"], row["split_kernel_ms"] = timing["compute_ms"], timing["dominant_name"], timing["dominant_ms"]
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
