#!/bin/bash
# The host's framers and command line under AddressSanitizer + UBSan (CPU only: goss dump-bases and the checks of the
# command line need no device), driven by the parser fuzz, tests/test_cli_surface.py and the surface checks of
# tests/test_relative_cpu.py.  goss and translucent are built by the Makefile's own rules (its HOST_SRCS), as stand-alone
# programs linked with the sanitizer; libgossgpu.so is used as built.
# usage: bash tools/host_asan.sh [cases] [seed]
set -e
cd "$(dirname "$0")/.."
mkdir -p scratch/asan
make -C gossamer_amd/csrc ../libgossgpu.so
cp -p gossamer_amd/libgossgpu.so scratch/asan/
make -C gossamer_amd/csrc OUT=../../scratch/asan CXXFLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer" \
    ../../scratch/asan/goss ../../scratch/asan/translucent
export GOSS_BIN="$PWD/scratch/asan/goss" ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
python tools/dbg/parser_fuzz.py "${1:-200}" "${2:-1}"
python -m pytest tests/test_cli_surface.py -x -q
# the same driver under its other name: the surface checks of translucent (decided before a command object runs)
export TRANSLUCENT_BIN="$PWD/scratch/asan/translucent"
exec python -m pytest tests/test_relative_cpu.py -x -q -k "surface or help or unknown or shared"
