#!/bin/bash
# GPU box: A/B of library builds on ONE box, alternating:  tools/ab_lib.sh <variant.so> [rounds]
V=$1; R=${2:-3}
for i in $(seq $R); do for lib in "" $V; do LYRA_HIP_LIB=$lib python bench.py --full --no-cpu-baseline --steps 300 --latency-steps 0 2>/dev/null | python -c "
import json,sys
r=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('lib=${lib:-default}', r['value'], r['ms_per_step'], ' '.join(k.replace('_kernel','')+'='+str(v['avg_us']) for k,v in r['kernels'].items()))"; done; done
