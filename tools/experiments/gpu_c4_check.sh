#!/bin/bash
# GPU check of the C4 path: the GPU tests, then a C4 bench line (each step time-limited).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p bench_out
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread -p no:cacheprovider > bench_out/pytest_gpu.log 2>&1
rc=$?; tail -5 bench_out/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full --config 4 --steps 40 --warmup 10 --no-cpu-baseline > bench_out/c4.json 2> bench_out/c4.err
rc=$?; tail -c 1500 bench_out/c4.json; exit $rc
