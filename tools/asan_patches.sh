#!/bin/bash
# Host sanitizer run of patches since a mark (CPU only): tools/patches_asan.cpp, a stand-alone
# program with its own main, built with oplog.cpp under AddressSanitizer + UBSan and run directly
# (no device code, no Python).  Forks keep a plain model of their document, sync by join or delta,
# and apply their own patches_since to the model: the models must converge.
set -e
cd "$(dirname "$0")/.."
ROCM=${ROCM:-/opt/rocm}
OUT=crdt-benches_amd/build/asan
mkdir -p "$OUT"
"$ROCM/lib/llvm/bin/clang++" -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -Iinclude -Icrdt-benches_amd/csrc \
    tools/patches_asan.cpp crdt-benches_amd/csrc/oplog.cpp -o "$OUT/patches_asan"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1:halt_on_error=1 \
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/patches_asan"
