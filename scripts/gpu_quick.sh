# Quick GPU check: full GPU test suite (+ C++ facade tests and perf drivers through pytest) + short bench lines.
cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}  # (where the logs go)
mkdir -p "$OUT"
timeout 1700 python -m pytest tests -q -m gpu 2>&1 | grep -E "^E  |^FAILED|^ERROR|passed|failed" | cut -c1-500 | head -60 | tee "$OUT/pytest_gpu.log"
for c in ${BENCH_CONFIGS:-2}; do
  python bench.py --config $c --steps 5 --warmup 1 --full --no-cpu-baseline 2>&1 | tail -1 | tee "$OUT/bench_quick_config$c.log"
done
