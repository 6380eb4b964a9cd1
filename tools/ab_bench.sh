#!/bin/bash
# same-box A/B on the headline step:  tools/ab_bench.sh <A> <B> [rounds] [steps] [warmup]
# A side is a build of libdge_hip.so (a path) or an environment switch of the same build (NAME=VALUE, e.g. DGE_NO_UP_DG_SMALL=1;
# `-` = no switch).  Interleaved rounds; prints ms_per_step of each run and the median step time.
A=$1; B=$2; R=${3:-2}; S=${4:-20}; W=${5:-3}
for r in $(seq 1 $R); do
  for L in "$A" "$B"; do
    case "$L" in
      -) set_env="DGE_AB_SIDE=default" ;;
      *=*) set_env="$L" ;;
      *) set_env="DGE_LIB_PATH=$L" ;;
    esac
    env "$set_env" python bench.py --gpus 1 --steps $S --warmup $W --no-cpu-baseline --no-extras --no-synthesis 2>/dev/null | tail -1 | \
      python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$L', round(d['ms_per_step'],3), 'median', round(d['step_ms']['median'],3), 'img/s', round(d['value'],1))"
  done
done
