#!/bin/bash
# tools/microbench/mfma_f64_rate.hip: the fp64 matrix-core rate behind the Gram kernel's estimate (profiles/gram.json)
#   tools/mb_mfma.sh [output file, default mfma_f64_rate.txt]
R=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-mfma_f64_rate.txt}
mkdir -p $R/tools/microbench/build
B=$R/tools/microbench/build/mfma_f64_rate
[ -x $B ] || hipcc --offload-arch=gfx950 -O3 -w -o $B $R/tools/microbench/mfma_f64_rate.hip || exit 1
timeout -k 10 120 $B | tee "$out"
