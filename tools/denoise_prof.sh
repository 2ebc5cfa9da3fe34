#!/bin/bash
# Collects the evidence of DESIGN.md section 4c for the `atrous` denoiser on a GPU box, from the repo root:  tools/denoise_prof.sh [OUT_DIR]
#   events   RENE_DEBUG=1 tools/denoise_workload.py W H REPS ab   per-kernel HIP events, the LDS staging A/B in one process
#   stats    rocprofv3 --kernel-trace --stats                      per-kernel time
#   sq1 / fetch / write   rocprofv3 --kernel-trace --pmc ...       one pass per counter group, never combined with --stats
# for 1920x1080 and 7680x4320 (cornell_box, 8 spp: the filter's cost does not depend on spp).  Each pass is reduced to
# OUT_DIR/prof_dn_<size>_<pass>.json by tools/extract_pass.py; tools/summarize_denoise_profiles.py OUT_DIR TAG writes profiles/.
R=$(pwd); OUT=${1:-$R/prof_out}; mkdir -p $OUT
export TMPDIR=/tmp
W="python3 $R/tools/denoise_workload.py"
( RENE_DEBUG=1 timeout -k 10 120 $W 1920 1080 4 ab && RENE_DEBUG=1 timeout -k 10 200 $W 7680 4320 3 ab ) > $OUT/dn_events.log 2>&1 || { echo "events run failed"; tail -20 $OUT/dn_events.log; exit 1; }
for size in "1920 1080" "7680 4320"; do
  tag=${size/ /x}
  for p in stats sq1 fetch write; do
    case $p in
      stats) ARGS="--stats" ;;
      sq1) ARGS="--pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_VALU_TRANS_F32 SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD" ;;
      fetch) ARGS="--pmc FETCH_SIZE" ;;
      write) ARGS="--pmc WRITE_SIZE" ;;
    esac
    D=$OUT/prof_dn_${tag}_$p
    rm -rf $D
    timeout -k 10 240 rocprofv3 --kernel-trace $ARGS -d $D -o p -- $W $size 2 > $D.log 2>&1 || { echo "pass $tag $p failed"; tail -5 $D.log; exit 1; }
    python3 $R/tools/extract_pass.py $D && rm -rf $D || exit 1
  done
done
