# instruction mix per kernel: bash tools/pmc_insts.sh <tag> [env...]   -> $PROFILE_DIR/pmc_<tag> (default profile_out)
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROFILE_DIR:-profile_out}/pmc_$tag
cd /tmp && export TMPDIR=/tmp && cd "$root" && mkdir -p $out
for kv in "$@"; do export "$kv"; done
for i in 1 2; do
  case $i in
    1) C="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_WAVE_CYCLES";;
    2) C="SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY";;
  esac
  timeout -k 10 200 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $out/p$i -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/bench$i.json 2> $out/err$i.log || echo "pass $i failed"
done
