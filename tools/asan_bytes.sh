#!/bin/bash
# Host sanitizer run of the byte-offset reading of positional patches (CPU only):
# tools/bytes_asan.cpp, a stand-alone program with its own main, built with oplog.cpp under
# AddressSanitizer + UBSan and run directly (no device code, no Python).  A log takes seeded
# non-touching patch sets in UTF-8 byte offsets through apply_patches_bytes, a clone takes them in
# codepoints one remove + insert at a time: the logs must stay equal, patches_since_bytes must
# splice a UTF-8 buffer into the current text, and every malformed set and every boundary inside a
# codepoint must be refused without a change.
set -e
cd "$(dirname "$0")/.."
ROCM=${ROCM:-/opt/rocm}
OUT=crdt-benches_amd/build/asan
mkdir -p "$OUT"
"$ROCM/lib/llvm/bin/clang++" -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -Iinclude -Icrdt-benches_amd/csrc \
    tools/bytes_asan.cpp crdt-benches_amd/csrc/oplog.cpp -o "$OUT/bytes_asan"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1:halt_on_error=1 \
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/bytes_asan"
