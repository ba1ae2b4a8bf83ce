#!/bin/bash
# Collects the judged profile artefacts of one version into $OUT_DIR/<tag>/ (default tools/scratch/<tag>/, git-ignored):
#   tools/collect_profiles.sh <tag> [extra bench.py arguments, e.g. --permute 42]
# 1. bench line (--full: with cpu_baseline)   2. rocprofv3 --kernel-trace --stats of the same bench command
# 3. PMC passes FETCH_SIZE / WRITE_SIZE (separate runs, kernel trace only) of the same bench command
# 4. the traffic summary of the dominant kernel (tools/pmc_traffic_json.py), with the fingerprint of the kernel sources
tag=$1; shift
extra="$@"
kern=k_spgemm_tile,k_spgemm_slab,k_spgemm_ghash,k_bs_numeric   # (the dominant one of the run is picked)
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
out=${OUT_DIR:-tools/scratch}/$tag
mkdir -p $out
timeout 900 python3 bench.py --gpus 1 --steps 10 --warmup 3 --full $extra > $out/bench.json 2> $out/bench.err
timeout 900 rocprofv3 --kernel-trace --stats -d $out/stats -o run -- python3 bench.py --gpus 1 --steps 10 --warmup 3 $extra > $out/stats.log 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 900 rocprofv3 --kernel-trace --pmc $c -d $out/pmc_$c -o run --output-format csv -- python3 bench.py --gpus 1 --steps 4 --warmup 3 $extra > $out/pmc_$c.log 2>&1
done
python3 tools/prof_summary.py $out/stats/run_results.db > $out/kernel_stats.csv
python3 tools/pmc_traffic_json.py $out $kern $out/pmc_traffic.json
# (only the summaries are kept: the raw traces are large)
rm -rf $out/stats $out/pmc_FETCH_SIZE $out/pmc_WRITE_SIZE
head -12 $out/kernel_stats.csv
