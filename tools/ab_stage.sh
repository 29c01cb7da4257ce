#!/bin/bash
# like ab.sh, but prints the front-end stages (cfar / extract / filter) of tools/stage_times.py
#   e.g. tools/ab_stage.sh 3 "--unstaged" ""
n=${1:-3}; ca=$2; cb=$3; shift 3
for r in $(seq 1 "$n"); do
  for v in a b; do
    if [ "$v" = a ]; then c=$ca; else c=$cb; fi
    envs=(); args=()
    for w in $c; do
      if [ ${#args[@]} -eq 0 ] && [[ $w == [A-Z]*=* ]]; then envs+=("$w"); else args+=("$w"); fi
    done
    env "${envs[@]}" timeout -s KILL 90 python tools/stage_times.py --batch 512 --icp-variants 0 "${args[@]}" "$@" 2>&1 | grep "^cfar\|^extract\|^filter" | tr '\n' ' ' | sed "s/^/$v /"; echo
  done
done
