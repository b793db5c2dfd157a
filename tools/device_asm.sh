#!/bin/bash
# gfx950 device assembly of the library with the per-build __hip_cuid_* symbol masked, for `diff` before / after a change that must not move the device code (needs no GPU)
# usage (repo root): bash tools/device_asm.sh OUT [extra hipcc flags]
OUT=$1; shift
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include --cuda-device-only -S extendedrtirtmodeling.jl_amd/csrc/ertirt.hip "$@" -o "$OUT" && sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$OUT"
