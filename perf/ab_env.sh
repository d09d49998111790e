#!/bin/bash
# Same-box A/B of ENVIRONMENT switches with the default library:  bash perf/ab_env.sh [-w workload] [-a "bench args"] "A=0" "QPAL_PF=1" ...
# Every setting runs THREE times, interleaved (drift of the box shows up as disagreement between the passes).
WL=llama3.1-8b_tcomb_6_7; ARGS=""
while getopts "w:a:" o; do case $o in w) WL=$OPTARG;; a) ARGS=$OPTARG;; esac; done; shift $((OPTIND-1))
run() { env $1 timeout -k 10 300 python bench.py --full --workload $WL --steps 100 --warmup 10 --no-cpu-baseline --no-incoherent-extra --no-whole-model --no-calibration --no-other-configs $ARGS 2>/dev/null | python -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l); r=d['roofline']; bk=r.get('by_launch_kind') or {}
        print('%-24s %7.1f tok/s %7.4f ms frac %.4f | ' % ('[$1]', d['value'], d['ms_per_step'], r['frac']) + '  '.join('%s %.2f' % (k, v['us_per_launch']) for k, v in bk.items() if isinstance(v, dict)))"; }
for pass in 1 2 3; do for v in "$@"; do run "$v"; done; done
