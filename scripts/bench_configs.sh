#!/bin/bash
# The other BASELINE configurations on one GPU (builder-run numbers, not the headline)
set -o pipefail
O=gpurun_out/configs_${1:-a}
mkdir -p $O
run() {
  local tag=$1; shift
  timeout -k 10 400 python -u bench.py --full --no-cpu-baseline --sampler-batches 16 "$@" > $O/$tag.json 2> $O/$tag.err || { echo "bench $tag failed"; tail -5 $O/$tag.err; exit 1; }
  python3 -c "
import json
d=json.loads(open('$O/$tag.json').read().strip().splitlines()[-1]); c=d['config']
print('$tag', round(d['ms_per_step'],4), 'ms/step', '%.3g edges/s' % d['value'], 'issue', round(c['host_train_issue_s_per_step']*1e3,3), 'wait', round(c['host_sampler_wait_s_per_step']*1e3,3), 'epoch', round(c['epoch_time_s'],4), 'sampler-only %.3g' % c['gpu_sampler_only']['value'])"
}
run c3 --shape products --layers 100-256-256-47 --fanout 15-10-5 --batch 1024 --weight mean --steps 40 --warmup 10 --epochs 2
run c4 --shape products --layers 100-256-47 --fanout 25-10 --batch 1024 --steps 40 --warmup 10 --epochs 2
