#!/bin/bash
# Runs on the GPU box: counter profiles (tools/profile.sh) of the non-headline BASELINE
# configs, summarised on the box so that the bench lines taken right after carry a
# sha-matched roofline.  The bench lines go to profiles/<tag>_bench_<cfg>.json; re-run
# tools/rocpd_summary.py on the merged prof_<tag>_<cfg> output of tools/profile.sh to install the summaries.
# Every GPU step has its own time limit; the first failing step ends the script.
#   tools/profile_configs.sh <tag> cfg4 cfg2 ...
set -euo pipefail
TAG=${1:-r02h}; shift
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$REPO"
for CFG in "$@"; do
  bash tools/profile.sh ${TAG}_$CFG --config $CFG > gpurun_out/profile_${TAG}_$CFG.log 2>&1
  python tools/rocpd_summary.py gpurun_out/prof_${TAG}_$CFG profiles/${TAG}_$CFG $CFG \
      >> gpurun_out/profile_${TAG}_$CFG.log 2>&1
  timeout -k 10 900 python bench.py --full --config $CFG 2>/dev/null | tail -1 > profiles/${TAG}_bench_$CFG.json
  if [ "$CFG" = cfg2 ]; then
    timeout -k 10 900 python bench.py --full --config cfg2 --graph 2>/dev/null | tail -1 > profiles/${TAG}_bench_cfg2_graph.json
  fi
  # keep the merged output small: the sqlite traces are what rocpd_summary.py needs
  find gpurun_out/prof_${TAG}_$CFG -type f ! -name '*.db' ! -name '*.txt' ! -name '*.log' -delete
  du -sh gpurun_out/prof_${TAG}_$CFG
done
tail -c 600 profiles/${TAG}_bench_*.json
