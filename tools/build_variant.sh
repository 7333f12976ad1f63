#!/bin/bash
# Build a library variant for in-run A/B (tools/ab_lib.sh, tools/ab_chain.sh, tools/pmc_ab.sh): tools/_bin/libvsg_<name>.so
# from the sources as they are, with the SOURCES and FLAGS of visual_sgraphs_amd/build.py plus any extra flags; the in-tree
# library is not touched.  The library has no build-time switches: a variant is an edit of the sources (a constant, a code
# path) on a branch of its own.   Usage: tools/build_variant.sh <name> [extra hipcc flags] ...
set -e
name=$1; shift
cd "$(dirname "$0")/.."
mkdir -p tools/_bin
eval "$(python3 -c '
import shlex
from visual_sgraphs_amd.build import CSRC, FLAGS, SOURCES
print("flags=(%s)" % " ".join(map(shlex.quote, FLAGS)))
print("srcs=(%s)" % " ".join(shlex.quote(str(CSRC / s)) for s in SOURCES))
')"
/opt/rocm/bin/hipcc "${flags[@]}" "$@" -o tools/_bin/libvsg_$name.so "${srcs[@]}" -ldl -lpthread
echo "built tools/_bin/libvsg_$name.so"
