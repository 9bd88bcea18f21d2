#!/bin/bash
# Host sanitizer run of text windows (CPU only): tools/text_asan.cpp, a stand-alone program with its
# own main, built with oplog.cpp under AddressSanitizer + UBSan and run directly (no device code, no
# Python).  A log goes through edits, wire updates, a join and a delta with a text model beside it
# and a mark after every step; every text_at(mark) must equal its recording, every window the slice
# of it with its info, patches_since(mark) applied to text_at(mark) the text now, and every
# malformed call must be refused with its outputs untouched.  Output buffers are heap blocks of
# exactly the size passed.
set -e
cd "$(dirname "$0")/.."
ROCM=${ROCM:-/opt/rocm}
OUT=crdt-benches_amd/build/asan
mkdir -p "$OUT"
"$ROCM/lib/llvm/bin/clang++" -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -Iinclude -Icrdt-benches_amd/csrc \
    tools/text_asan.cpp crdt-benches_amd/csrc/oplog.cpp -o "$OUT/text_asan"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1:halt_on_error=1 \
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/text_asan"
