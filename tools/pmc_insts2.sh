# more SQ counters per kernel: bash tools/pmc_insts2.sh <tag>   -> $PROFILE_DIR/pmc2_<tag> (default profile_out)
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROFILE_DIR:-profile_out}/pmc2_$tag
cd /tmp && export TMPDIR=/tmp && cd "$root" && mkdir -p $out
for kv in "$@"; do export "$kv"; done
C="SQ_INSTS_BRANCH SQ_IFETCH SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INST_LEVEL_VMEM SQ_INST_LEVEL_LDS SQ_BUSY_CU_CYCLES"
timeout -k 10 200 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $out/p1 -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/bench1.json 2> $out/err1.log || echo "pass failed"
