#!/bin/bash
# A/B builds of the score kernels (timing probes): tools/build_score_probe_lib.sh <name> "<flags>" -> quartetscores_amd/lib/libqs_probe_<name>.so (QS_PY_LIB=...)
set -e
name=${1:?name}; flags=${2:-}
cd "$(dirname "$0")/../quartetscores_amd/csrc"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
make OBJDIR="$tmp" OUT=../lib/libqs_probe_$name.so EXTRA_SRCS=qs_score.hip EXTRA_HIPFLAGS="$flags"
ls -la ../lib/libqs_probe_$name.so
