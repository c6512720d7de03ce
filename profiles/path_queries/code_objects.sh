#!/bin/bash
# Compare the gfx950 code objects of two builds of libdrpo_hip.so, object file by object file:
#   code_objects.sh <parent build dir> <this tree's build dir>
# Each *.o carries its device code as a clang offload bundle in .hip_fatbin; the gfx950 entry is
# unbundled and its .text and .rodata are compared byte for byte.
set -euo pipefail
A=$1; B=$2
ROCM=${ROCM_PATH:-/opt/rocm}
BUNDLER=$ROCM/lib/llvm/bin/clang-offload-bundler
OBJCOPY=$ROCM/lib/llvm/bin/llvm-objcopy
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
same=0; total=0
for o in "$B"/*.o; do
  n=$(basename "$o" .o)
  [ "$n" = build_digest ] && continue
  for side in a b; do
    src=$A/$n.o; [ $side = b ] && src=$B/$n.o
    if [ ! -f "$src" ]; then echo "$n: only in this tree (no device code expected)"; continue 2; fi
    $OBJCOPY -O binary --only-section=.hip_fatbin "$src" "$T/$n.$side.fatbin"
    if [ ! -s "$T/$n.$side.fatbin" ]; then continue; fi
    $BUNDLER --unbundle --type=o --input="$T/$n.$side.fatbin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
      --output="$T/$n.$side.co"
    for sec in .text .rodata; do
      $OBJCOPY -O binary --only-section=$sec "$T/$n.$side.co" "$T/$n.$side$sec" 2>/dev/null || : > "$T/$n.$side$sec"
    done
  done
  if [ ! -s "$T/$n.a.fatbin" ] && [ ! -s "$T/$n.b.fatbin" ]; then echo "$n: no device code in either"; continue; fi
  total=$((total + 1))
  if cmp -s "$T/$n.a.text" "$T/$n.b.text" && cmp -s "$T/$n.a.rodata" "$T/$n.b.rodata"; then
    same=$((same + 1))
    echo "$n: .text $(stat -c %s "$T/$n.b.text") bytes, .rodata $(stat -c %s "$T/$n.b.rodata") bytes: identical"
  else
    echo "$n: DIFFERENT (.text $(stat -c %s "$T/$n.a.text") vs $(stat -c %s "$T/$n.b.text"))"
  fi
done
echo "identical .text and .rodata in $same of $total gfx950 code objects"
