# The bench line with a fresh edge_index tensor per step (K0's CSR build inside every timed
# step, as the reference's loader-fed step) beside the cached-graph line, on one box.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}  # where this script leaves its logs
export TMPDIR=/tmp
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full --fresh-graph --no-cpu-baseline > "$OUT"/bench_fresh.log 2>&1 || { tail -5 "$OUT"/bench_fresh.log; exit 1; }
tail -1 "$OUT"/bench_fresh.log | cut -c1-300
timeout -k 10 600 python bench.py --full --no-cpu-baseline > "$OUT"/bench_cached.log 2>&1 || { tail -5 "$OUT"/bench_cached.log; exit 1; }
tail -1 "$OUT"/bench_cached.log | cut -c1-300
