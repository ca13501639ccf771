#!/bin/bash
# Mutants of the link-prediction kernels: each is the library
# with one -DSKGE_MUTANT_* switch in csrc/skge_score.hip or csrc/skge_curve.hip,
# built beside the real one and run ONCE over tests/test_gpu_linkpred.py through
# SKGE_LIB_PATH.  Every mutant stays inside its buffers (see the #ifdef sites).
#   build:  tools/mutants_linkpred.sh build      (no GPU needed)
#   run:    tools/mutants_linkpred.sh run        (prints failed / passed per mutant)
set -o pipefail
cd "$(dirname "$0")/../scikit-kge_amd" || exit 1
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=${ARCH:-gfx950} -Wall -Wno-unused-result"
OUT=mutants/linkpred
# mutant:source
MUTANTS="NO_ZERO_CANON:skge_curve TIES_NOT_GROUPED:skge_curve DROP_LAST_CARRY:skge_curve RESCAL_IGNORE_REL:skge_score"

case "$1" in
build)
  make -j"${JOBS:-8}" || exit 1
  mkdir -p "$OUT"
  for m in $MUTANTS; do
    name=${m%%:*}; src=${m##*:}
    $HIPCC $FLAGS -DSKGE_MUTANT_$name -c csrc/$src.hip -o "$OUT/$src.$name.o" || exit 1
    objs=$(ls build/*.o | grep -v "/$src.o")
    $HIPCC --offload-arch=${ARCH:-gfx950} -shared -fPIC -o "$OUT/libskgehip.$name.so" $objs \
      "$OUT/$src.$name.o" || exit 1
  done
  ;;
run)
  for m in $MUTANTS; do
    name=${m%%:*}
    line=$(SKGE_LIB_PATH="$PWD/$OUT/libskgehip.$name.so" timeout -k 10 300 \
      python -m pytest ../tests/test_gpu_linkpred.py -q -p no:cacheprovider 2>&1 | tail -1)
    rc=$?
    echo "$name: $line"
    # a time limit, an abort or a fault ends the run: nothing more goes to the GPU
    if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
  done
  ;;
*)
  echo "usage: $0 build|run"; exit 2 ;;
esac
