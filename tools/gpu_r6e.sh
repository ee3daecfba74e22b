#!/bin/bash
# round 6: default bench line (incl. c4_zipf / c4_1m / c4_timed), then the one-box --gpus 2 rehearsal
# of the C5 line over gloo (two ranks on GPU 0: conservation + the routed table == the merged table)
set -u
cd "${GRAFT_REPO_ROOT}"
mkdir -p bench_out/r6e
timeout -k 10 400 python bench.py --full --steps 20 --warmup 20 > bench_out/r6e/bench.json 2> bench_out/r6e/bench.err || { tail -20 bench_out/r6e/bench.err; exit 1; }
tail -c 300 bench_out/r6e/bench.json
FB_C5_BACKEND=gloo timeout -k 10 400 python bench.py --full --gpus 2 --steps 20 --warmup 10 --no-cpu-baseline --no-other-mode --no-host --no-single-launch --no-imix --no-c4 --c5-frames 4194304 > bench_out/r6e/gpus2.json 2> bench_out/r6e/gpus2.err
rc=$?
tail -c 1500 bench_out/r6e/gpus2.json; echo "rc=$rc"; tail -5 bench_out/r6e/gpus2.err
