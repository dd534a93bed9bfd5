# Round-end style check on the GPU box: build, GPU tests, smoke, default bench (+ optional
# rocprofv3 stats when PROFILE=1).  Every GPU step has its own time limit; stops at the
# first failure.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}  # where this script leaves its logs
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 1000 python -u -m pytest tests -v -m gpu --timeout 300 --timeout-method thread > "$OUT"/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc" >> "$OUT"/pytest_gpu.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1 || exit $?
timeout -k 10 600 python bench.py --full > "$OUT"/bench.log 2>&1 || exit $?
if [ "${PROFILE:-0}" = "1" ]; then
  mkdir -p "$OUT"/prof
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof -o egnn -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT"/prof_bench.log 2>&1
fi
