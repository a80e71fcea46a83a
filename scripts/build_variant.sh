#!/bin/bash
# Builds an A/B copy of libhvd_mi355x.so with extra defines for ONE translation unit, for same-box comparisons through
# HVD_LIB_PATH (the ablation / A-B figures under profiles/ were made this way).
#   bash scripts/build_variant.sh mstiming k_hamming.hip -DHVD_MATCH_SERVER_TIMING     -> build_tmp/libhvd_mstiming.so
set -eu
NAME=$1; UNIT=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd); SRC=$ROOT/hydrus-video-deduplicator_amd/csrc; OUT=$ROOT/build_tmp; mkdir -p $OUT
make -C $SRC -s
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize --offload-arch=gfx950"
# (.cpp units go through hipcc too: csrc/Makefile)
( cd $SRC && /opt/rocm/bin/hipcc $FLAGS "$@" -c $UNIT -o $OUT/${UNIT%.*}_$NAME.o )
OBJS=""
for o in hvd_api hvd_search hvd_comm hvd_stream k_hamming k_hamming_mfma k_hamming_index k_index_order k_index_scatter k_fp4_image k_vmatch k_synth k_pdq k_pdq_dihedral k_autocrop k_autocrop_fused k_barcolor k_detail k_crops k_valign k_valign_segments k_valign_rates k_valign_rate_segments k_valign_signed k_valign_loops k_group k_keeper k_spread k_runs; do
  if [ "$o" = "${UNIT%.*}" ]; then OBJS="$OBJS $OUT/${o}_$NAME.o"; else OBJS="$OBJS $SRC/$o.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 $OBJS -shared -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib -o $OUT/libhvd_$NAME.so
echo "$OUT/libhvd_$NAME.so"
