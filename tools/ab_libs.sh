#!/usr/bin/env bash
# A/B several builds of the library on the same box: tools/ab_libs.sh <repeats> libA.so libB.so ...   (run through gpurun)
n="$1"; shift
for r in $(seq $n); do
  for v in "$@"; do
    echo -n "$v: "
    NNHIP_ALLOW_TOOLING_LIB=1 NNHIP_LIB_NAME=$v python bench.py --full --no-cpu-baseline --steps 30 --no-train-leg --no-strong-leg --no-box-leg 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.readlines()[-1]); c=d['kernel_classes']
print(d['value'], d['ms_per_step'], {k: round(v['ms_per_step'],3) for k,v in c.items() if k.startswith('edge_') or k in ('mlp128','lin128')})"
  done
done
