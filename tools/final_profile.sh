# final profile set of the round: kernel trace stats + PMC traffic passes + FETCH_SIZE calibration, under $PROFILE_DIR/final
# (default profile_out/final); the benchmark runs with --full, so that the traces and bench_full.json hold everything it measures
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROFILE_DIR:-profile_out}/final
cd /tmp && export TMPDIR=/tmp && cd "$root" && mkdir -p $out
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -w -o /tmp/fcal tools/fetch_calib.hip || exit 1
for C in FETCH_SIZE WRITE_SIZE; do timeout -k 10 120 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $out/calib_$C -- /tmp/fcal > $out/calib_$C.log 2>&1; done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $out/bench_trace.json 2> $out/trace.err
for C in FETCH_SIZE WRITE_SIZE "TCC_HIT_sum TCC_MISS_sum"; do t=$(echo $C | tr ' ' '_'); timeout -k 10 300 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $out/pmc_$t -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $out/bench_$t.json 2> $out/pmc_$t.err; done
timeout -k 10 400 python bench.py --full > $out/bench_full.json 2> $out/bench_full.err
ls $out
# diagnostic builds (if present): phase ablations and instruction mix of the scatter / combine kernels
if [ -f build/diag/libspasm_amd_ablate.so ]; then
  (export SPASM_AMD_LIB=$PWD/build/diag/libspasm_amd_ablate.so; bash tools/ablate_stream.sh > $out/ablate_scatter.txt 2>&1; bash tools/ablate_combine.sh > $out/ablate_combine.txt 2>&1)
fi
bash tools/pmc_insts.sh final > /dev/null 2>&1
python tools/shard_time.py 2>/dev/null | grep "G=" > $out/shard_time.txt
