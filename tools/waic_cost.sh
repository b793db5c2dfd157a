#!/bin/bash
# A/B of the WAIC cost on ONE box: alternating processes of tools/waic_cost.py on the given libraries ("-" = the in-tree one), three rounds.
# usage (on the GPU box, from the repo root): bash tools/waic_cost.sh parent/libertirt.so -
set -o pipefail
for k in 1 2 3; do for lib in "$@"; do timeout -k 10 240 python tools/waic_cost.py "$lib" 5 || exit $?; done; done
