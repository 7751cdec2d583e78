#!/bin/bash
# Diagnostic build of decode attention with launch -> first K/V request stamps (-DMILA_ATTN_STAMPS): a SEPARATE library, never the product one.
#   bash tools/experiments/attn_stamps.sh                    tools/experiments/_build/libmila_cdna4_attn_stamps.so from the tree (kernarg preload on, as build.py builds it)
#   TAG=before SRC=<an older attention.hip with the same stamp lines> PRELOAD= bash tools/experiments/attn_stamps.sh      the build to compare against
# (cross-compiles without a GPU; mila_amd/lib/obj must hold the product objects: python -m mila_amd.build)   then on the GPU box:
#   python tools/experiments/attn_stamps.py after=tools/experiments/_build/libmila_cdna4_attn_stamps.so before=tools/experiments/_build/libmila_cdna4_attn_stamps_before.so
set -e
cd "$(dirname "$0")/../.."
mkdir -p tools/experiments/_build
tag=${TAG:+_$TAG}
src=${SRC:-mila_amd/csrc/attention.hip}
preload=${PRELOAD--mllvm -amdgpu-kernarg-preload-count=16}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function $preload -DMILA_ATTN_STAMPS -Imila_amd/csrc -Iinclude \
    -c "$src" -o tools/experiments/_build/attention_stamps$tag.o
objs=$(for f in mila_amd/csrc/*.hip; do b=$(basename $f .hip); [ $b != attention ] && echo mila_amd/lib/obj/$b.o; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/experiments/_build/libmila_cdna4_attn_stamps$tag.so $objs tools/experiments/_build/attention_stamps$tag.o
echo built tools/experiments/_build/libmila_cdna4_attn_stamps$tag.so
