#!/bin/bash
# Build an A/B library from another copy of rt_kernels.hip (the rest of csrc/ and include/ as in
# the tree) into build/ab/lib$NAME.so:   bash scripts/build_ab.sh NAME path/to/rt_kernels.hip [-DFOO ...]
# Sources and flags are raytracing_gpu_amd/_build.py's (HIP_SOURCES, HIPCC_FLAGS), the only list of them.
set -e
name=$1; src=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
list() { python3 -c "import sys; sys.path.insert(0, '$root'); from raytracing_gpu_amd import _build; print(' '.join(_build.$1))"; }
tmp=$(mktemp -d)
mkdir -p "$tmp/raytracing_gpu_amd/csrc" "$tmp/include" "$root/build/ab"
cp "$root"/raytracing_gpu_amd/csrc/*.cpp "$root"/raytracing_gpu_amd/csrc/*.h "$root"/raytracing_gpu_amd/csrc/*.hip \
  "$tmp/raytracing_gpu_amd/csrc/"
cp "$root"/include/*.h "$tmp/include/"
cp "$src" "$tmp/raytracing_gpu_amd/csrc/rt_kernels.hip"
cd "$tmp/raytracing_gpu_amd/csrc"
/opt/rocm/bin/hipcc $(list HIPCC_FLAGS) "$@" -o "$root/build/ab/lib$name.so" $(list HIP_SOURCES)
rm -rf "$tmp"
