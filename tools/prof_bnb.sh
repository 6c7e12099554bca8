set -o pipefail
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for m in 0 2; do
NSM_BNB=$m timeout -k 10 180 rocprofv3 --kernel-trace -d $OUT/prof_bnb$m -o run -- python3 bench.py --full --dtype bf16 --batch 64 --steps 3 --warmup 2 --no-cpu-baseline --no-secondary > $OUT/prof_bnb$m.log 2>&1 || exit 1
NSM_BNB=$m timeout -k 10 180 rocprofv3 --kernel-trace -d $OUT/prof_bnbf$m -o run -- python3 bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-secondary > $OUT/prof_bnbf$m.log 2>&1 || exit 1
done
