#!/bin/bash
# Build the HIP library of a git revision (or a source dir) as tools/var_<name>.so
# for same-box A/B runs (tools/ab_chain.py, tools/with_lib.py).
#   bash tools/build_variant.sh NAME REV [-DMACRO=VALUE ...]
# Kernel forms since removed from the tree are built this way: REV = a revision
# that still has them, with the macro that selected them there.
set -e
NAME=$1; REV=$2; shift 2
D=$(mktemp -d)
git archive "$REV" diplomjourney_amd/csrc include | tar -x -C "$D"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ldl -ffp-contract=off \
  -I "$D/include" "$@" -o tools/var_$NAME.so "$D"/diplomjourney_amd/csrc/*.hip
rm -rf "$D"
echo tools/var_$NAME.so
