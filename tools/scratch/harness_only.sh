#!/bin/bash
# the attention-harness block of tools/profile_round.sh alone (after rebuilding tools/scratch/attn_bench[_diag])
cd $GRAFT_REPO_ROOT
TAG=${1:-r06}; OUT=gpurun_out/$TAG; mkdir -p $OUT
{
  for args in "88 0 1 0" "22 0 1 0"; do
    echo -n "forward  B mode bias = $args: "; bash tools/scratch/trace_attn.sh attn_bench $args 2>&1 | grep -E "attn_fwd" | awk '{print $1, $(NF-1), $NF}'
  done
  for args in "88 0 1 1 1" "22 0 1 1 1"; do
    echo -n "backward $args: "; bash tools/scratch/trace_attn.sh attn_bench $args 2>&1 | grep -E "attn_bwd" | awk '{printf "%s %s us; ", $1, $(NF-1)} END {print ""}'
  done
  echo "stamps forward:"; tools/scratch/attn_bench_diag 88 0 1 0 2>&1 | grep -E "wave 0 clock"
  echo "stamps backward (dQ kernel):"; tools/scratch/attn_bench_diag 88 0 1 1 1 2>&1 | grep -E "wave 0 clock"
} > $OUT/${TAG}_attention_harness.txt 2>&1
cat $OUT/${TAG}_attention_harness.txt
