# round validation (round 4, 5): smoke, the whole GPU suite, bench.py, and its rocprofv3 kernel summary
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
export TMPDIR=/tmp
O=$GRAFT_REPO_ROOT/gpurun_out/${FINAL_TAG:-r05_final}
mkdir -p $O
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
rc=$?; tail -3 $O/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1
rc=$?; tail -4 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -u bench.py --full > $O/bench.json 2> $O/bench.err
rc=$?; cut -c1-600 $O/bench.json; [ $rc -eq 0 ] || exit $rc
(R=$PWD; cd "$TMPDIR" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o bench -- python3 $R/bench.py --full --steps 10 --warmup 3 > $O/bench_prof.json 2> $O/bench_prof.err)
rc=$?; echo "prof rc=$rc"; exit $rc
