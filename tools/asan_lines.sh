#!/bin/bash
# Host sanitizer run of the line index (CPU only): tools/lines_asan.cpp, a stand-alone program with
# its own main, built with oplog.cpp under AddressSanitizer + UBSan and run directly (no device code,
# no Python).  A log goes through edits, wire updates, a join and a delta with a text model beside it
# and a mark after every step; after every step every line number and every position of the version
# now and of each mark, in codepoints and in bytes, must give what a scan of the recording gives, and
# every malformed call must be refused with its outputs untouched.  Output blocks are heap blocks of
# exactly n records.
set -e
cd "$(dirname "$0")/.."
ROCM=${ROCM:-/opt/rocm}
OUT=crdt-benches_amd/build/asan
mkdir -p "$OUT"
"$ROCM/lib/llvm/bin/clang++" -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra \
    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -Iinclude -Icrdt-benches_amd/csrc \
    tools/lines_asan.cpp crdt-benches_amd/csrc/oplog.cpp -o "$OUT/lines_asan"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1:halt_on_error=1 \
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/lines_asan"
