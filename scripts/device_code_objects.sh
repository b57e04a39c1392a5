#!/bin/bash
# Device-only code objects of a source tree, for comparing two commits' device code (compile-only, no GPU needed):
# the six inst_*.hip and the shape_chain 5x3 plug-in, with the Makefile's flags, plus their kernel_digest.py digests.
#   scripts/device_code_objects.sh <tree> <outdir>          (tree: a checkout of this repository)
#   python3 scripts/kernel_resource_diff.py <outdir of the parent> <outdir of the new commit>
set -euo pipefail
TREE=$(cd "$1" && pwd)
mkdir -p "$2"
OUT=$(cd "$2" && pwd)
HERE=$(cd "$(dirname "$0")" && pwd)
cd "$TREE/altro-cpp_amd/csrc"
FLAGS=$(grep '^CXXFLAGS' Makefile | sed 's/^CXXFLAGS := //; s/\$(ARCH)/gfx950/')
# the translation unit altro_register_model_source generates for a user model (altro_capi.cpp), without the source hash
{
  echo '#include <hip/hip_runtime.h>'
  echo '#define ALTRO_MODEL_FN __device__ __forceinline__'
  echo '#pragma clang fp contract(on)'
  echo 'namespace altro_user {'
  echo '#define SHAPE_N 5'
  echo '#define SHAPE_M 3'
  cat "$TREE/tests/models/shape_chain.hpp"
  echo '}  // namespace altro_user'
  echo '#pragma clang fp contract(fast)'
  echo '#include "altro_user_model.hpp"'
} > "$OUT/shape_chain_5_3.hip"
build() {  # <source> <stem>
  /opt/rocm/bin/hipcc $FLAGS -I. --cuda-device-only --no-gpu-bundle-output -c "$1" -o "$OUT/$2.co"
  python3 "$HERE/kernel_digest.py" "$OUT/$2.co" > "$OUT/$2.digest"
}
pids=()
for f in inst_*.hip; do build "$f" "${f%.hip}" & pids+=($!); done
build "$OUT/shape_chain_5_3.hip" shape_chain_5_3 & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
