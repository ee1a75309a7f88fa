#!/bin/sh
# TEST INFRASTRUCTURE ONLY: builds the host harness of the large-table split path's core (see dfa_spec_emul.cpp)
set -e
here=$(cd "$(dirname "$0")" && pwd)
out=${1:-$here/dfa_spec_emul}
g++ -O2 -g -std=c++17 $EMUL_FLAGS -Wall -Wno-unknown-pragmas -Wno-unused-function -Wno-unused-variable -I"$here/shim" -I"$here/../../re2-modification_amd/csrc" -I"$here/../../include" \
    -o "$out" "$here/dfa_spec_emul.cpp" "$here/../../re2-modification_amd/csrc/image_host.cpp"
