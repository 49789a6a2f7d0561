#!/bin/bash
# variant build of libposepipe_hip.so for kernel ablations: bash tools/build_variant.sh <tag> "<extra hipcc flags>"
# -> posepipeline_amd/libposepipe_hip_<tag>.so (select with POSEPIPE_LIB=...); every split-conv translation unit
# (csrc/conv_split*.hip) is recompiled with the extra flags, the other objects come from the regular build
set -e
R=$(cd $(dirname $0)/.. && pwd)
TAG=$1; FLAGS=$2
make -C $R/posepipeline_amd/csrc > /dev/null
mkdir -p $R/build/variants
VOBJS=""; PIDS=""
for SRC in $R/posepipeline_amd/csrc/conv_split*.hip; do
    OBJ=$R/build/variants/$(basename $SRC .hip)_$TAG.o
    rm -f $OBJ
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$R/include -I$R/posepipeline_amd/csrc -ffp-contract=off -Wno-unused-function $FLAGS \
        -x hip -c $SRC -o $OBJ &
    PIDS="$PIDS $!"
    VOBJS="$VOBJS $OBJ"
done
for P in $PIDS; do wait $P || { echo "build_variant: a compile failed" >&2; exit 1; }; done
OBJS=$(ls $R/build/csrc/*.o | grep -v '/conv_split[^/]*\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS $VOBJS -o $R/posepipeline_amd/libposepipe_hip_$TAG.so
echo built $R/posepipeline_amd/libposepipe_hip_$TAG.so
