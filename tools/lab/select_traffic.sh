#!/bin/bash
# Prices the sources of select_lazy_kernel<true>'s memory traffic (LAB_NOTES "Selection kernel: where the bytes go").
#   select_traffic.sh build   lab libraries okvis2_amd/libokvfe_lab_off<N>.so, k_select.hip compiled with
#                             -DOKVFE_SELECT_OFF=<N> (bits: describe_setup_dev.h); needs `make lab` first
#   select_traffic.sh run [tag]   on the GPU: per library a kernel-trace run and the two byte passes (FETCH_SIZE,
#                             WRITE_SIZE, each a run of its own) of bench.py; one line per run in $SELECT_TRAFFIC_OUT/<tag>.txt
#                             (default: select_traffic_out/ in the repository root)
# The variant libraries compute wrong results by design: only their byte and time counts mean anything.
set -u
R=$(cd "$(dirname "$0")/../.." && pwd)
VARIANTS="1 2 4 8 16 32"
if [ "${1:-}" = build ]; then
  cd $R/okvis2_amd/csrc || exit 1
  FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function"
  OTHERS=$(ls build_lab/*.o | grep -v 'k_select\.hip' | grep -v '\.off')
  for N in $VARIANTS; do
    /opt/rocm/bin/hipcc $FLAGS -DOKVFE_LAB -DOKVFE_SELECT_OFF=$N -x hip -c k_select.hip -o build_lab/k_select.off$N.o &
  done
  wait
  for N in $VARIANTS; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libokvfe_lab_off$N.so build_lab/k_select.off$N.o $OTHERS -ldl || exit 1
  done
  exit 0
fi
TAG=${2:-select_traffic}
OUT=${SELECT_TRAFFIC_OUT:-$R/select_traffic_out}
mkdir -p $OUT
export TMPDIR=/tmp
cd /tmp
BENCH="python $R/bench.py --gpus 1 --steps 6 --warmup 3"
LIBS="${SELECT_TRAFFIC_LIBS:-product $VARIANTS}"
LIBDIR=${SELECT_TRAFFIC_DIR:-$R/okvis2_amd}  # (another tree's libraries: the same passes on a parent build)
for V in $LIBS; do
  if [ $V = product ]; then LIB=$LIBDIR/libokvfe.so; else LIB=$LIBDIR/libokvfe_lab_off$V.so; fi
  D=/tmp/st_${TAG}_$V
  OKVFE_LIB=$LIB timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $D/t -o p -- $BENCH > $D.t.log 2>&1 || { echo "$V trace: exit $?" >> $OUT/$TAG.txt; exit 1; }
  echo "$V time $(grep select_lazy_kernel $(find $D/t -name '*kernel_stats.csv' | head -1) | head -1)" >> $OUT/$TAG.txt
  for C in FETCH_SIZE WRITE_SIZE; do
    OKVFE_LIB=$LIB timeout -k 10 240 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $D/$C -o p -- $BENCH > $D.$C.log 2>&1 || { echo "$V $C: exit $?" >> $OUT/$TAG.txt; exit 1; }
    python $R/tools/pmc_summary.py $(find $D/$C -name '*counter_collection.csv' | head -1) $OUT/${TAG}_${V}_$C.json > /dev/null
    python - $OUT/${TAG}_${V}_$C.json $V $C >> $OUT/$TAG.txt <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d.items():
    if k.startswith("select_lazy_kernel"):
        print(sys.argv[2], sys.argv[3], k, v["mean_per_dispatch"], "grid", v["grid"], "vgpr", v["vgpr"], "scratch", v["scratch"], "lds", v["lds"])
PY
  done
done
