#!/bin/bash
# A/B builds of the count kernels with other compile-time switches, next to the product library (never loaded unless the Python
# harness is told to: QS_PY_LIB=<path>; the library itself reads no environment):
#   tools/build_probe_lib.sh <name> "<extra hipcc flags>"   ->  quartetscores_amd/lib/libqs_probe_<name>.so
# What makes up the library is csrc/Makefile's list; only the two count-kernel files are compiled with the flags.
set -e
name=${1:?name}; flags=${2:-}
cd "$(dirname "$0")/../quartetscores_amd/csrc"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
make -j4 OBJDIR="$tmp" OUT=../lib/libqs_probe_$name.so EXTRA_SRCS="qs_count.hip qs_count_fused.hip" EXTRA_HIPFLAGS="$flags"
ls -la ../lib/libqs_probe_$name.so
