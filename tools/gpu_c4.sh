#!/bin/bash
# Run on the GPU box: configs[3] parity tests of the VM / CP paths, then tools/bench_c4.py
cd ${GRAFT_REPO_ROOT:-/root/repo}
python -m pytest tests/test_lotd_gpu.py tests/test_fullsize_gpu.py -m gpu -x -q -k "vm or c4 or mixed or half_tables or binned or atomic" 2>&1 | tail -4
python tools/bench_c4.py --iters 20 2>/dev/null | tail -1 | python -c "
import sys, json; d = json.loads(sys.stdin.read()); print('configs[3]:', d['ms'], d['ms_total'], {k: v['frac'] for k, v in d['roofline']['per_pass'].items()})"
