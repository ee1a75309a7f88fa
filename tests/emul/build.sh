#!/bin/sh
# TEST INFRASTRUCTURE ONLY: builds one of the host harnesses of this folder (see NAME_emul.cpp).
#   build.sh NAME [OUT]       OUT: where the program goes (default: NAME_emul in this folder)
#   EMUL_FLAGS: more compiler flags, e.g. -DWALK_NODE_MAP=1 or -fsanitize=address,undefined
#   EMUL_ROOT:  the tree whose include/ and re2-modification_amd/csrc/ are compiled (default: this repository); the harness itself,
#               the shim, emul_common.h and emul_wave.h are always this folder's
set -e
name=${1:?usage: build.sh NAME [OUT]}
here=$(cd "$(dirname "$0")" && pwd)
case ${2:-} in "") out=$here/${name}_emul ;; /*) out=$2 ;; *) out=$PWD/$2 ;; esac
cd "$here"
root=${EMUL_ROOT:-../..}
csrc=$root/re2-modification_amd/csrc
# the harnesses that compile the kernels' own headers do so through the HIP shim, and hear the warnings those headers raise under g++
shim="-Ishim -Wno-unknown-pragmas -Wno-unused-function -Wno-unused-variable"
# NAME          optimisation   more flags                              sources beside NAME_emul.cpp
case $name in
walk)           opt=-O1        more="$shim -Wno-maybe-uninitialized"   src="$csrc/walk_tables.cpp $csrc/image_host.cpp" ;;
plan|dfa_plan|memless_plan)
                opt=-O1        more=                                   src= ;;
dfa_split|dfa_resume|dfa_mixed|nfa_set|nfa_set_resume)
                opt=-O1        more=$shim                              src=$csrc/image_host.cpp ;;
# (-O2: these walk every string several times, or do 64 lanes' work per step)
dfa_spec|nfa_set_split|nfa_set_wave|nfa_set_wave_resume|nfa_set_wave_split)
                opt=-O2        more=$shim                              src=$csrc/image_host.cpp ;;
text_split|select)
                opt=-O2        more=$shim                              src= ;;
*)              echo "build.sh: no harness named '$name'" >&2; exit 2 ;;
esac
g++ $opt -g -std=c++17 $EMUL_FLAGS -Wall $more -I$csrc -I$root/include -o "$out" ${name}_emul.cpp $src
