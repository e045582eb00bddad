#!/bin/bash
# builds a library variant that recompiles ONE translation unit with extra flags and links it with the main build's other objects.
# usage: tools/build_variant.sh <name> <unit> "<extra flags>"   ->  build_variants/libmphip_<name>.so
set -euo pipefail
name=$1; unit=$2; flags=$3
here="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
src=$here/megaportrait-hack_amd/csrc
mkdir -p $here/build_variants
obj=$(mktemp -d "${TMPDIR:-/tmp}/bv_$name.XXXXXX")   # the recompiled unit's object: private to this run, removed on exit
trap 'rm -rf "$obj"' EXIT
extra=""
if [ "$unit" == "conv3d_f16x3_wino_pp" ] || [ "$unit" == "conv3d_f16x3_wino_bt" ]; then extra="-fno-slp-vectorize"; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fvisibility=default -Wall -Wno-unused-function $extra $flags -c $src/$unit.hip -o $obj/$unit.o
objs=()
for f in api warp warp_bwd norm conv3d conv3d_f16x3_plan conv3d_f16x3 conv3d_f16x3_wino conv3d_f16x3_wino_pp conv3d_f16x3_wino_bt mfma_sol backward conv3d_bwd_f16x3 flowfield plan g2d_final conv2d_f16x3 conv2d_gn_f16x3 conv2d_lp conv2d_run conv2d_s2_f16x3 conv2d_up2_f16x3 conv2d_stem conv2d_grp_f16x3 conv2d_splitk_f16x3 conv2d_pw_f16x3 conv2d_stem7_f16x3 conv2d_bwd_f16x3 feature_loss; do
  if [ "$f" == "$unit" ]; then objs+=($obj/$unit.o); else objs+=($src/build/$f.o); fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $here/build_variants/libmphip_$name.so "${objs[@]}"
echo built build_variants/libmphip_$name.so
