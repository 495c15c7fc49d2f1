#!/bin/bash
# Diagnostic build of the C-ABI library (plan overrides via MI355_CONV_SHAPE / _CT / _KSPLIT): tools/_build/, never shipped.
# The sources are those of the shipped build (csrc/Makefile holds the list); every object is recompiled, since the flags
# may differ from the last call's.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/_build
make -B -j8 -C unet_bssfp_amd/csrc lib OBJDIR="$PWD/tools/_build" EXTRA_CXXFLAGS="-DMI355_DIAG $MI355_DIAG_FLAGS" \
  LIB="$PWD/tools/_build/libmi355_unet_diag${MI355_DIAG_SUFFIX}.so"
echo built tools/_build/libmi355_unet_diag${MI355_DIAG_SUFFIX}.so
