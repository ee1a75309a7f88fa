#!/bin/sh
# TEST INFRASTRUCTURE ONLY: builds the host harness of the planner of memory-less segments (see dfa_plan_emul.cpp)
set -e
here=$(cd "$(dirname "$0")" && pwd)
out=${1:-$here/dfa_plan_emul}
g++ -O1 -g -std=c++17 $EMUL_FLAGS -Wall -I"$here/../../re2-modification_amd/csrc" -I"$here/../../include" -o "$out" "$here/dfa_plan_emul.cpp"
