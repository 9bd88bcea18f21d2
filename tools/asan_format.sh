#!/bin/bash
# Host sanitizer run of formats (CPU only): tools/format_asan.cpp, a stand-alone program with its
# own main, built with oplog.cpp under AddressSanitizer + UBSan and run directly (no device code, no
# Python).  Two forks keep a per-character attribute model beside their text; spans must match it
# after edits, after a join one way and a delta the other, both forks must paint the union of their
# formats alike, and every malformed call must be refused with its outputs untouched.
set -e
cd "$(dirname "$0")/.."
ROCM=${ROCM:-/opt/rocm}
OUT=crdt-benches_amd/build/asan
mkdir -p "$OUT"
"$ROCM/lib/llvm/bin/clang++" -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -Iinclude -Icrdt-benches_amd/csrc \
    tools/format_asan.cpp crdt-benches_amd/csrc/oplog.cpp -o "$OUT/format_asan"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1:halt_on_error=1 \
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/format_asan"
