#!/bin/bash
# Round-3 start: the full GPU suite, then the C4 bench line (pipelined + one-stream split).
set -u
cd "${GRAFT_REPO_ROOT}"
mkdir -p bench_out
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread -p no:cacheprovider > bench_out/r3_tests.log 2>&1
rc=$?; tail -3 bench_out/r3_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --config 4 --steps 20 --warmup 5 --no-cpu-baseline --no-host --no-other-mode > bench_out/r3_c4.json 2> bench_out/r3_c4.err || { tail bench_out/r3_c4.err; exit 1; }
tail -c 1500 bench_out/r3_c4.json
