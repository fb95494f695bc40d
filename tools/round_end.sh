# What a round ends with, in one GPU run: the whole -m gpu suite, the full bench line (C2, with every configuration's leg) and C5 at its
# full 100 M pairs. usage: tools/round_end.sh <outdir>; copy bench_c2.json / bench_c5_100m.json into profiles/<round>/ afterwards.
# (The PMC passes are tools/refresh_profiles.sh's; run that first when a kernel's sources changed.)
set -x
OUT=${1:?usage: tools/round_end.sh <outdir>}
mkdir -p "$OUT"
timeout 2700 python -m pytest tests/ -q -m gpu > "$OUT/tests.log" 2>&1; echo "pytest rc $?" >> "$OUT/tests.log"
tail -6 "$OUT/tests.log"
timeout 900 python bench.py --full > "$OUT/bench_c2.json" 2> "$OUT/bench_c2.err"
timeout 600 python bench.py --full --config c5 --steps 20 --warmup 2 --no-cpu-baseline --no-configs > "$OUT/bench_c5_100m.json" 2> "$OUT/bench_c5_100m.err"
