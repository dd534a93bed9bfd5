# TP tests + rocprofv3 kernel stats of a short MACE bench (GPU box; via gpurun).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}  # where this script leaves its logs
export TMPDIR=/tmp
mkdir -p "$OUT"/prof_mace
timeout -k 10 400 python -u -m pytest ${TESTS:-tests/test_gpu_tpnode.py tests/test_gpu_equivariant.py} -m gpu --timeout 200 --timeout-method thread -q > "$OUT"/tp.log 2>&1
rc=$?; tail -3 "$OUT"/tp.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_mace -o stats -- python3 bench.py --full --workload mace --steps 2 --warmup 1 --no-cpu-baseline > "$OUT"/prof_mace/bench.log 2>&1 || exit $?
tail -1 "$OUT"/prof_mace/bench.log | cut -c1-400
