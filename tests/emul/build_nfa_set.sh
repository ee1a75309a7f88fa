#!/bin/sh
# TEST INFRASTRUCTURE ONLY: builds the host harness of the set walk's core (see nfa_set_emul.cpp)
set -e
here=$(cd "$(dirname "$0")" && pwd)
out=${1:-$here/nfa_set_emul}
g++ -O1 -g -std=c++17 $EMUL_FLAGS -Wall -Wno-unknown-pragmas -Wno-unused-function -Wno-unused-variable -I"$here/shim" -I"$here/../../re2-modification_amd/csrc" -I"$here/../../include" \
    -o "$out" "$here/nfa_set_emul.cpp" "$here/../../re2-modification_amd/csrc/image_host.cpp"
