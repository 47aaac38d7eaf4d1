#!/bin/bash
# usage: [UNITS="hm_merge_nf_1_9 ..."] tools/build_alt.sh <name> <extra hipcc flags...>  -> camera_linearity_amd/lib/alt_<name>/libhdrmerge.so
# A second build of the library that differs only in the compile flags of some units (A/B runs on one box via HDRMERGE_LIB). UNITS names
# the units to rebuild (without .hip); the default is every unit of the fused merge, which is right for any knob - a knob of one
# kernel family needs only the unit(s) that hold it (the file map is in csrc/hm_merge.hip; HM_LUT_U and HM_VAL3_FLAT_U also size the
# dispatcher's launches: rebuild hm_merge with them). The other objects come from the last `make`.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); name=$1; shift
S=$R/camera_linearity_amd/csrc; L=$R/camera_linearity_amd/lib
UNITS=${UNITS:-$(cd $S && ls hm_merge*.hip | sed 's/\.hip$//' | grep -v '^hm_merge_chunk$')}
D=$L/alt_$name; mkdir -p $D; rm -f $D/*.o          # (a unit that fails to compile then fails the link)
skip=""
for u in $UNITS; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I$R/include -I$S -DHM_TUNE_NF=${TUNE_NF:-0} "$@" \
    -c $S/$u.hip -o $D/$u.o &
  skip="$skip -e /$u.o\$"
done
wait
objs=$(ls $L/*.o | grep -v $skip)
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $objs $D/*.o -o $D/libhdrmerge.so -Wl,-rpath,/opt/rocm/lib -Wl,-z,defs
echo built $D/libhdrmerge.so
