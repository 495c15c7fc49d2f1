#!/bin/bash
# Timing-only variants of the C-ABI library (tools/_build/, never shipped): the other objects come from the diagnostic build
# (tools/build_diag.sh), the convolution API object is recompiled per variant (csrc/Makefile: variant).
# usage: tools/build_variants.sh name1="-DX -DY" name2="-DZ" ...
set -e
cd "$(dirname "$0")/.."
MK=(make -s -C unet_bssfp_amd/csrc OBJDIR="$PWD/tools/_build" EXTRA_CXXFLAGS="-DMI355_DIAG $MI355_DIAG_FLAGS")
mkdir -p tools/_build
# Objects that are missing or older than a source are compiled once, here, with the diagnostic build's flags; no diagnostic
# library is linked.  make does not track flags: an up-to-date object keeps those of the call that compiled it
# (tools/build_diag.sh recompiles everything).
"${MK[@]}" -j8 objs
for spec in "$@"; do
  name=${spec%%=*}; flags=${spec#*=}
  ( "${MK[@]}" variant NAME="$name" VARIANT_FLAGS="$flags" && echo built $name ) &
done
wait
