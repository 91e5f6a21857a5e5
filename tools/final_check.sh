#!/bin/bash
# GPU box, end of round: smoke(), refreshed rocprofv3 evidence, default bench line (with cpu_baseline), ic bench line.
R=$GRAFT_REPO_ROOT
LOG=${BH_LOG_DIR:-$R/logs}
mkdir -p $LOG
cd $R
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2 || exit 1
bash tools/profile_round.sh ${1:-r02} > $LOG/profile_round.log 2>&1 || { tail -5 $LOG/profile_round.log; exit 1; }
cd $R
timeout -k 10 300 python bench.py --full > $LOG/bench_wc.log 2>&1 || { tail -5 $LOG/bench_wc.log; exit 1; }
timeout -k 10 200 python bench.py --variant ic --no-cpu-baseline --no-extras > $LOG/bench_ic.log 2>&1 || exit 1
tail -1 $LOG/bench_wc.log | cut -c1-300
tail -1 $LOG/bench_ic.log | cut -c1-200
