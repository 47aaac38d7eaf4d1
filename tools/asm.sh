#!/bin/bash
# tools/asm.sh [-o <dir>] <file.hip>... [-- extra flags]: device-only assembly of the given sources -> <dir>/<name>.s (default /tmp), compiled
# in parallel; prints the VGPR counts and scratch sizes of their kernels. Two such directories are what tools/kernel_asm_diff.py compares.
R=$(cd "$(dirname "$0")/.." && pwd)
out=/tmp
if [ "$1" = "-o" ]; then out=$2; shift 2; mkdir -p $out; fi
files=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do files+=("$1"); shift; done
[ "$1" = "--" ] && shift
for f in "${files[@]}"; do
  n=$(basename $f .hip)
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I$R/include -I$R/camera_linearity_amd/csrc -DHM_TUNE_NF=${TUNE_NF:-0} "$@" \
    -Wall -Wno-unused-function -S --cuda-device-only $R/camera_linearity_amd/csrc/$n.hip -o $out/$n.s 2>&1 | grep -v "warning: argument unused" &
done
wait
for f in "${files[@]}"; do
  grep -E "^\s*\.set .*\.(num_vgpr|private_seg_size)," $out/$(basename $f .hip).s | sed 's/^\s*\.set //'
done
