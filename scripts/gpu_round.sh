# One GPU-box pass: GPU tests (all, not stopping at the first failure), smoke, default bench.
# Every GPU step has its own time limit; a timeout / crash ends the script.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}  # where this script leaves its logs
mkdir -p "$OUT"
export TMPDIR=/tmp
T=${TESTS:-tests}
timeout -k 10 900 python -u -m pytest $T -v -m gpu --timeout 300 --timeout-method thread > "$OUT"/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc" >> "$OUT"/pytest_gpu.log
tail -3 "$OUT"/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1 || exit $?
cat "$OUT"/smoke.log | grep smoke
if [ "${BENCH:-1}" = "1" ]; then
  timeout -k 10 900 python bench.py --full > "$OUT"/bench.log 2>&1 || exit $?
  tail -1 "$OUT"/bench.log
fi
