#!/bin/bash
# Build libadaptive_amd.so variants for A/B runs (tools/ab.sh) into abvar/ (travels to the GPU box).
# usage: bash tools/build_variant.sh <name> <git-rev | WORK> [extra hipcc flags...]
#   WORK = the working tree's sources; a rev = those files as committed at that revision.
# Every translation unit of the chosen sources is built (that revision's own Makefile, objects side by
# side); a revision from before the library was split into units has the two files that existed then.
set -eu
name=$1; rev=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/tools/_build" "$ROOT/abvar"
if [ "$rev" = WORK ]; then  # a snapshot: hipcc reads the sources again for its host pass
  src=$(mktemp -d /tmp/aa_variant.XXXXXX)
  mkdir -p "$src/adaptive_amd" && cp -r "$ROOT/adaptive_amd/csrc" "$src/adaptive_amd/" && cp -r "$ROOT/include" "$src/"
else
  src=$(mktemp -d /tmp/aa_variant.XXXXXX)
  git -C "$ROOT" archive "$rev" adaptive_amd/csrc include | tar -x -C "$src"
fi
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -fvisibility=hidden -ffp-contract=off -Wall -Wno-unused-function -Wno-pass-failed $*"
if [ -f "$src/adaptive_amd/csrc/aa_lstm.hip" ]; then
  make -C "$src/adaptive_amd/csrc" OUT="$ROOT/abvar/$name.so" OBJDIR="$src/obj" CXXFLAGS="$FLAGS"
else
  /opt/rocm/bin/hipcc $FLAGS -I"$src/include" -shared -o "$ROOT/abvar/$name.so" \
    "$src/adaptive_amd/csrc/aa_kernels.hip" "$src/adaptive_amd/csrc/aa_optim.hip"
fi
echo "built abvar/$name.so from $rev $*"
