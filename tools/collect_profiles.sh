# copy the summaries of $PROFILE_DIR/final (tools/final_profile.sh; default profile_out) into profiles/ under the given tag:
#   bash tools/collect_profiles.sh r01_final
tag=${1:-r01_final}
cd "$(dirname "$0")/.."
d=${PROFILE_DIR:-profile_out}
python tools/pmc_summary.py $d/final profiles/${tag}_traffic.json > /dev/null
cp "$(ls -t $d/final/trace/*/*_kernel_stats.csv | head -1)" profiles/${tag}_kernel_stats.csv
cp $d/final/bench_full.json profiles/${tag}_bench.json
cp "$(ls -t $d/final/calib_FETCH_SIZE/*/*_counter_collection.csv | head -1)" profiles/${tag}_calibration_FETCH_SIZE.csv
cp "$(ls -t $d/final/calib_WRITE_SIZE/*/*_counter_collection.csv | head -1)" profiles/${tag}_calibration_WRITE_SIZE.csv
cp $d/final/shard_time.txt profiles/${tag}_shard_time.txt
[ -f $d/final/ablate_scatter.txt ] && cp $d/final/ablate_scatter.txt profiles/${tag}_ablations_scatter.txt
[ -f $d/final/ablate_combine.txt ] && cp $d/final/ablate_combine.txt profiles/${tag}_ablations_combine.txt
for k in 'k_wstream<10' 'k_wstream<11' 'k_wstream<12' 'k_wplan' 'k_wlevel_wave' 'k_wlevel_wg' 'k_scatter<13'; do echo "== $k (mean per dispatch)"; python tools/pmc_show.py $d/pmc_final "$k"; done > profiles/${tag}_instruction_mix.txt
ls -la profiles | grep ${tag}
