#!/bin/bash
# GPU check: parity tests, a full bench line, a rocprofv3 kernel-trace summary.
# Stops at the first crash / timeout (exit status other than 0 or 1).
# Run from anywhere; results go to $OUT (default: out/ in the repository).
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT" || exit 1
export TMPDIR=${TMPDIR:-$(mktemp -d)}
OUT=${OUT:-$ROOT/out}
mkdir -p "$OUT"
ok() { local rc=$1; [ "$rc" -eq 0 ] || [ "$rc" -eq 1 ]; }
MODE=${1:-all}
[ "$MODE" = allpmc ] && RUNALL=1
python -c "import torch;print(torch.cuda.get_device_name(0))" > "$OUT/device.txt" 2>&1
if [ "$MODE" = all ] || [ -n "$RUNALL" ] || [ "$MODE" = tests ]; then
  timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 -rf \
      > "$OUT/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -30 "$OUT/pytest_gpu.log"
  ok $rc || exit $rc
fi
if [ "$MODE" = all ] || [ -n "$RUNALL" ] || [ "$MODE" = bench ]; then
  timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$OUT/bench.json" 2> "$OUT/bench.err"
  rc=$?; echo "bench rc=$rc"; cat "$OUT/bench.json"; tail -5 "$OUT/bench.err"
  [ $rc -eq 0 ] || exit $rc
fi
if [ "$MODE" = all ] || [ -n "$RUNALL" ] || [ "$MODE" = prof ]; then
  cd "$TMPDIR" && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv \
      -d "$OUT/prof" -o run -- \
      python "$ROOT/bench.py" --full --no-cpu-baseline --steps 10 --warmup 30 \
      > "$OUT/prof_bench.json" 2> "$OUT/prof.err"
  rc=$?; echo "rocprof rc=$rc"; cd "$ROOT"
  find "$OUT/prof" -name "*kernel_stats.csv" -exec cat {} \; | cut -c1-250 | head -20
  [ $rc -eq 0 ] || exit $rc
  python tools/trace_check.py "$OUT/prof/run_kernel_trace.csv" "$OUT/prof_bench.json" 30 10
  # headline kernel alone (a plain run): its stats average is the bench's kernel_ms
  cd "$TMPDIR" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv \
      -d "$OUT/prof_flash" -o run -- \
      python "$ROOT/bench.py" --steps 20 --warmup 5 \
      > "$OUT/prof_flash_bench.json" 2> "$OUT/prof_flash.err"
  rc=$?; echo "rocprof flash-only rc=$rc"; cd "$ROOT"
  [ $rc -eq 0 ] || exit $rc
fi
if [ "$MODE" = pmc ] || [ "$MODE" = allpmc ]; then
  # one counter group per pass (TCC FETCH_SIZE and WRITE_SIZE cannot share a pass)
  rocprofv3 -L > "$OUT/counters_available.txt" 2>&1 || true
  for ctr in FETCH_SIZE WRITE_SIZE "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_WAVES" "SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT"; do
    tag=$(echo $ctr | tr ' ' '_')
    cd "$TMPDIR" && timeout -k 10 300 rocprofv3 --pmc $ctr --kernel-trace --output-format csv \
        -d "$OUT/pmc_$tag" -o run -- \
        python "$ROOT/bench.py" --full --quick --with-decode --steps 3 --warmup 1 \
        > "$OUT/pmc_$tag.json" 2> "$OUT/pmc_$tag.err"
    rc=$?; echo "pmc $ctr rc=$rc"; cd "$ROOT"
    [ $rc -eq 0 ] || exit $rc
  done
  python tools/pmc_summary.py "$OUT" "$OUT/traffic.json" > /dev/null && cat "$OUT/traffic.json"
fi
