#!/bin/bash
# Build variants/libdse_NAME.so from git revision REV: build_rev.sh NAME REV [-DFOO=1 ...]
set -e
NAME=$1; REV=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=/tmp/dse_rev_$NAME
rm -rf $T && mkdir -p $T/distributed-sieve-e_amd/csrc $T/include
# whichever sources REV has (the set of units and headers differs between revisions)
for f in $(git -C $ROOT ls-tree --name-only $REV:distributed-sieve-e_amd/csrc); do
  case $f in *.hip|*.cpp|*.h|Makefile) git -C $ROOT show $REV:distributed-sieve-e_amd/csrc/$f > $T/distributed-sieve-e_amd/csrc/$f ;; esac
done
git -C $ROOT show $REV:include/dse.h > $T/include/dse.h
SRC_DIR=$T/distributed-sieve-e_amd/csrc WHEEL_FLAGS="$(sed -n 's/^WHEEL_FLAGS ?= //p' $T/distributed-sieve-e_amd/csrc/Makefile)" \
  bash $ROOT/tools/build_variant.sh $NAME "$@"
