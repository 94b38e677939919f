#!/bin/bash
# A/B of the headline bench (C3 with its roofline stages, no sweep / cpu baseline) across library build flags; each variant rebuilds.
# usage: scripts/bench_variants.sh "<hipcc flags>" ...   (results appended to $VARIANTS_LOG, default variants/bench.txt)
cd $GRAFT_REPO_ROOT
LOG=${VARIANTS_LOG:-variants/bench.txt}
mkdir -p "$(dirname "$LOG")"
for v in "$@"; do
  for rep in 1 2; do
    echo -n "[$v] rep $rep: " | tee -a "$LOG"
    TACEX_EXTRA_HIPCC_FLAGS="$v" python bench.py --full --no-sweep --no-cpu-baseline --steps 60 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['value'], {k:round(v['avg_ms'],4) for k,v in d['roofline']['stages'].items()})" | tee -a "$LOG"
  done
done
