#!/bin/bash
# A/B two configurations inside ONE GPU session (box-to-box variance is larger than most kernel changes):
# alternates tools/stage_times.py between configuration A and configuration B.  A configuration is environment
# assignments (another build: SONARFE_LIB) followed by stage_times arguments (--tune NAME=VALUE, --unstaged).
# usage (on the GPU box): tools/ab.sh rounds "CONF_A" "CONF_B" [extra stage_times args]
#   e.g. tools/ab.sh 3 "SONARFE_LIB=$PWD/_ab/libsonarfe_a.so" ""      (another build vs the in-tree one)
#        tools/ab.sh 3 "--tune sw_rtrips=3" ""
n=${1:-3}; ca=$2; cb=$3; shift 3
for r in $(seq 1 "$n"); do
  for v in a b; do
    if [ "$v" = a ]; then c=$ca; else c=$cb; fi
    envs=(); args=()
    for w in $c; do
      if [ ${#args[@]} -eq 0 ] && [[ $w == [A-Z]*=* ]]; then envs+=("$w"); else args+=("$w"); fi
    done
    env "${envs[@]}" timeout -s KILL 90 python tools/stage_times.py --batch 512 --icp-variants 0 "${args[@]}" "$@" 2>&1 | grep "^icp" | sed "s/^/$v /"
  done
done
