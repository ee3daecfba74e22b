set -u
cd "${GRAFT_REPO_ROOT}"
mkdir -p bench_out
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > bench_out/r2_pytest.log 2>&1; rc=$?; tail -3 bench_out/r2_pytest.log; [ $rc -le 1 ] || exit $rc
timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 > bench_out/r2_b20.json 2>bench_out/r2_b20.err || exit 1
timeout -k 10 200 python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-host > bench_out/r2_b200.json 2>bench_out/r2_b200.err || exit 1
python -c "
import json
for f in ('bench_out/r2_b20.json','bench_out/r2_b200.json'):
    d=json.load(open(f)); print(f, d['value'], d['roofline']['frac'], d['roofline']['kernel_ms_per_launch'], {k:v.get('value') for k,v in d.get('extra',{}).items() if isinstance(v,dict)})
"
