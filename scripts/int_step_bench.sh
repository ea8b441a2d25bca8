#!/bin/bash
# The arms of BRT_INT_STEP (brt_device.h) through tests/tools/int_step_bench.hip, a binary per arm under ab/:
#   scripts/int_step_bench.sh build [ARMS]     cross-compiles (no GPU needed)
#   scripts/int_step_bench.sh run [ARMS]       runs what was built, one arm after the other
set -e
mode="$1"; arms="${2:-0 1 2 3 4 5 6 7 8 16 15 23}"
root="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$root/ab"
for n in $arms; do
    bin="$root/ab/int_step_bench_$n"
    if [ "$mode" = build ]; then
        ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -I"$root/bevyray_amd/csrc" -DBRT_INT_STEP="$n" -o "$bin" "$root/tests/tools/int_step_bench.hip"
    else
        timeout -k 10 120 "$bin"
    fi
done
