#!/bin/bash
# the full GPU suite + the benchmark line with every extra key (--full): tools/gpu_full.sh <tag> [<output dir>, default bench_out/<tag>]
cd "$(dirname "$0")/.."; export TMPDIR=${TMPDIR:-/tmp}
TAG=${1:-full}
O=${2:-bench_out/$TAG}
mkdir -p "$O"
timeout 1500 python -m pytest tests/ -q -m gpu -x > "$O/pytest_gpu.log" 2>&1; echo "pytest rc=$?"; tail -5 "$O/pytest_gpu.log"
timeout 900 python bench.py --full > "$O/bench.json" 2> "$O/bench.err"; echo "bench rc=$?"
python - "$O/bench.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print('headline', d['ms_per_step'], d['value'], d['roofline'])
for k in ('rmat','gat','gatmh','transform_first','cached_ah0','amazon_rank0of8'):
    v=d.get(k)
    if isinstance(v,dict): print(k, v.get('ms_per_step'), v.get('roofline'))
    else: print(k, v)
print('cpu', d.get('cpu_baseline'))
PY
