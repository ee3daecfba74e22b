#!/bin/bash
# GPU tests (all), then the C4 bench line and a C4 kernel trace.
set -u
cd "${GRAFT_REPO_ROOT}"
R=$(pwd); mkdir -p bench_out; export TMPDIR=/tmp
timeout -k 10 420 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > bench_out/r2_pytest.log 2>&1; rc=$?; tail -5 bench_out/r2_pytest.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --config 4 --steps 20 --warmup 4 --no-cpu-baseline > bench_out/r2_c4.json 2>bench_out/r2_c4.err || { tail bench_out/r2_c4.err; exit 1; }
python -c "
import json
d=json.load(open('bench_out/r2_c4.json')); print(d['value'], d['ms_per_step'], json.dumps(d['extra']['c4_stages'])[:400], d['extra']['c4_zipf'])"
rm -rf bench_out/c4prof
cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $R/bench_out/c4prof -o run -- python3 $R/bench.py --full --config 4 --steps 10 --warmup 2 --no-cpu-baseline --no-other-mode > $R/bench_out/c4prof.log 2>&1 || exit 1
