#!/bin/bash
# A/B of the per-time-step launch budgets on the headline configuration (GPU box, repository root)
O=gpurun_out/r05; mkdir -p $O
for v in 1 0; do
  NSK_STEP_BUDGETS=$v python3 bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-fortran-host --no-kdim > $O/ab_sb$v.json 2> $O/ab_sb$v.err
  python3 -c "
import json; r=json.load(open('$O/ab_sb$v.json')); print('step_budgets=$v', 'value %.3f' % r['value'], 'ms/time step %.4f' % r['ms_per_time_step'], 'retries', r['map_retries'], 'recaptures', r['graph_recaptures'], r['graph_recapture_s'], r['launch_budgets']['per_time_step'], r['launch_budgets']['last_step_class'], 'iters', r['helm_iters_per_step'], r['pres_iters_per_step'])"
done
