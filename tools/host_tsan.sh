#!/bin/bash
# The host's parallel framer under ThreadSanitizer (CPU only: goss dump-bases needs no device), driven by the parser
# fuzz and tests/test_host_cpu.py.  -DGOSS_TSAN_BUILD: the one wait_for of the framer as a sleeping wait (gcc 11's
# ThreadSanitizer does not intercept pthread_cond_clockwait and reports nonsense behind it).  goss is built by the
# Makefile's own rule (its HOST_SRCS), as a stand-alone program linked with the sanitizer; libgossgpu.so is used as built.
# usage: bash tools/host_tsan.sh [cases] [seed]
set -e
cd "$(dirname "$0")/.."
mkdir -p scratch/tsan
make -C gossamer_amd/csrc ../libgossgpu.so
cp -p gossamer_amd/libgossgpu.so scratch/tsan/
make -C gossamer_amd/csrc OUT=../../scratch/tsan CXXFLAGS="-DGOSS_TSAN_BUILD -O1 -g -std=c++17 -fsanitize=thread -fno-omit-frame-pointer" \
    ../../scratch/tsan/goss
export GOSS_BIN="$PWD/scratch/tsan/goss" TSAN_OPTIONS=halt_on_error=1
python tools/dbg/parser_fuzz.py "${1:-200}" "${2:-1}"
exec python -m pytest tests/test_host_cpu.py -x -q
