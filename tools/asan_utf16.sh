#!/bin/bash
# Host sanitizer run of the UTF-16 positions (CPU only): tools/utf16_asan.cpp, a stand-alone program
# with its own main, built with oplog.cpp under AddressSanitizer + UBSan and run directly (no device
# code, no Python).  A log goes through edits, wire updates, a join and a delta with a text model
# beside it and a mark after every step; after every step every gap of the version now and of each
# mark, asked in codepoints, bytes and UTF-16 code units, must give the three sums over the
# recording; the patches since each mark in UTF-16 must splice the recording's UTF-16 into the text
# now; a patch set in UTF-16 must leave the log its codepoint translation leaves; and every malformed
# call must be refused with its outputs or the log untouched.  Blocks are heap blocks of exactly n
# entries.
set -e
cd "$(dirname "$0")/.."
ROCM=${ROCM:-/opt/rocm}
OUT=crdt-benches_amd/build/asan
mkdir -p "$OUT"
"$ROCM/lib/llvm/bin/clang++" -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -Iinclude -Icrdt-benches_amd/csrc \
    tools/utf16_asan.cpp crdt-benches_amd/csrc/oplog.cpp -o "$OUT/utf16_asan"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1:halt_on_error=1 \
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/utf16_asan"
