#!/bin/bash
# another build of the library for same-box A/B rounds: tools/build_variant.sh <name> [-DFLAG=..] ...  -> build/ab/lib_<name>.so
# (select it with PF_LIB=build/ab/lib_<name>.so; tools/abn.sh takes that as part of a setting).  The product library's sources and
# flags, from its Makefile (EXTRA)
set -e
name=$1; shift
make -s -B -C "$(dirname "$0")/../pi-slam-fusion_amd/csrc" OUT=../../build/ab/lib_$name.so EXTRA="$*" ../../build/ab/lib_$name.so
echo built build/ab/lib_$name.so
