#!/bin/bash
# usage: build_variant_lib.sh <src.hip> <tag> [extra -D flags]   -> scratch/abl/liboasr_<tag>.so
# <src.hip> (absolute, or relative to olmoasr_amd/csrc): a variant of one source of olmoasr_amd/csrc under that source's file name, e.g. a
# patched attention_fwd.hip; its object replaces the product object of the same name, every other object is the product's.
# Flags the Makefile gives that one object go with the extra flags: build_variant_lib.sh logmel_quad.hip waves4 -fno-slp-vectorize -DQUAD_WAVES=4
set -e
SRC=$1; TAG=$2; shift 2
OBJ=$(basename ${SRC%.*}).o
cd /root/repo/olmoasr_amd/csrc
make -s -j8 >/dev/null
[ -f build/$OBJ ] || { echo "no product object build/$OBJ to replace"; exit 1; }
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -munsafe-fp-atomics -I. "$@" -c $SRC -o /tmp/variant_$TAG.o
OBJS=$(ls build/*.o | grep -v "^build/$OBJ\$" | grep -v decode_fused.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $(dirname $0)/../../scratch/abl/liboasr_$TAG.so $OBJS /tmp/variant_$TAG.o
echo built $TAG
