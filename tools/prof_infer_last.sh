# the last eager 1080p forward's launches (bf16 and fp32), one rocprofv3 kernel trace each
set -euo pipefail
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
mkdir -p $OUT/pinf
for d in bf16 f32; do
  rm -rf $OUT/pinf/raw_$d
  timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $OUT/pinf/raw_$d -o run -- python3 bench.py --full --workload infer1080 --dtype $d --steps 5 --warmup 2 --no-cpu-baseline > $OUT/pinf/$d.log 2>&1
  T=$(find $OUT/pinf/raw_$d -name run_kernel_trace.csv -print -quit)
  N=$(python3 -c "import csv; print(len(list(csv.DictReader(open('$T')))))")
  python3 tools/ktrace.py "$T" $((N - ${NK:-80})) ${NK:-80} > $OUT/pinf/last_$d.txt
  rm -rf $OUT/pinf/raw_$d
  grep -o '"value":[0-9.]*' $OUT/pinf/$d.log | head -1
done
