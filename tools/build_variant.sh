#!/bin/bash
# Build an A/B variant of libdse.so with extra defines: build_variant.sh NAME -DFOO=1 ...
# tools/build_rev.sh builds one from a git revision.
# The sources are copied to a scratch tree and built by their own Makefile, so
# the units (OBJS) and each unit's flags are the Makefile's, never a list kept here.
set -e
NAME=$1; shift
D=${SRC_DIR:-$(cd "$(dirname "$0")/../distributed-sieve-e_amd/csrc" && pwd)}  # SRC_DIR: another source tree (e.g. a git revision)
OUT=$(cd "$(dirname "$0")/.." && pwd)/variants
T=/tmp/dse_var_$NAME
rm -rf $T; mkdir -p $OUT $T/distributed-sieve-e_amd/csrc $T/include
cp $D/*.hip $D/*.cpp $D/*.h $D/Makefile $T/distributed-sieve-e_amd/csrc/
cp $D/../../include/dse.h $T/include/
HF="$(sed -n 's/^HIPFLAGS ?= //p' $D/Makefile) $*"  # the Makefile's flags, then the variant's defines
# WHEEL_FLAGS / PLAIN_FLAGS from the environment override the Makefile's (?=)
make -s -j8 -C $T/distributed-sieve-e_amd/csrc OUT=$OUT/libdse_$NAME.so HIPFLAGS="$HF"
echo $OUT/libdse_$NAME.so
