#!/bin/bash
# quick iteration: parity tests + bench (no rocprof)
set -u
RES=${FD_SESSION_OUT:-session_out}      # results, under the repository root
mkdir -p $RES
python -c "import __graft_entry__ as g; g.build()" > $RES/build.log 2>&1
timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider -x > $RES/pytest_gpu.log 2>&1 ; echo "pytest rc=$?" ; tail -5 $RES/pytest_gpu.log
timeout 900 python bench.py --steps 10 --warmup 2 --no-cpu-baseline --full > $RES/bench.log 2>&1 ; echo "bench rc=$?"
python - "$RES/bench.log" <<'PY'
import json, sys
for line in open(sys.argv[1]):
    if line.startswith('{'):
        d=json.loads(line)
        print('RTF', d['value'], 'ms/step', d['ms_per_step'], 'roofline', d.get('roofline'))
        for k,v in d.get('kernels',{}).items(): print(f"  {k:20s} {v}")
PY
