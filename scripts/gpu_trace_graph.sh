# EGNN step timeline under HIP-graph replay vs eager (kernel trace per stream)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}  # where this script leaves its logs
export TMPDIR=/tmp
for mode in eager graph; do
  mkdir -p "$OUT"/trace_$mode
  extra=""; [ $mode = graph ] && extra="--graph"
  timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$OUT"/trace_$mode -o t -- python3 bench.py --full --workload egnn --steps 3 --warmup 1 --no-cpu-baseline $extra > "$OUT"/trace_$mode/bench.log 2>&1 || exit $?
  f=$(find "$OUT"/trace_$mode -name "*kernel_trace.csv" | head -n 1)
  idx=-2; [ $mode = graph ] && idx=-4
  python3 scripts/trace_timeline.py $f egnn_fwd_kernel 4 $idx > "$OUT"/trace_$mode/timeline.txt || exit $?
  echo "== $mode"; head -n 40 "$OUT"/trace_$mode/timeline.txt
done
