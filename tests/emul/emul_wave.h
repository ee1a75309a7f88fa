// TEST INFRASTRUCTURE ONLY: how the wave harnesses of this folder (nfa_set_wave*_emul.cpp) load their image -- beside emul_common.h, so
// that the harnesses of the lane kernels do not compile the wave core.
#pragma once
#include "emul_common.h"
#include "nfa_set_wave_core.h"

namespace emul {

// the image of a blob file with wave tables (nfa_set_wave_build); tab: a copy from before the tables were built, for tabulate_nfa.
// Exit code 2: not a memory-less image; 3: the image gets no wave tables; 5: the tables built are not wave tables
inline void load_wave(const char* path, mfa::HostImage& set, mfa::HostImage* tab = nullptr) {
    const std::vector<uint8_t> blob = slurp(path);
    if (mfa::parse_blob(blob.data(), blob.size(), set) != MFA_OK || set.h.kind != MFA_KIND_NFA) { fprintf(stderr, "not a memory-less image\n"); exit(2); }
    if (tab) *tab = set;
    const int rc = mfa::nfa_set_wave_build(set);
    if (rc != MFA_OK) { fprintf(stderr, "no wave tables: %d\n", rc); exit(3); }
    if (!set.set_wave || set.set_tables[mfa::SET_H_WORDS] != mfa::wave_words_of(set.h.n_nodes)) fail("not wave tables");
}

// "tables WORDS W DEPTH": what the kernels place the tables by
inline void print_tables(const mfa::HostImage& set) {
    printf("tables %zu %u %u\n", set.set_tables.size(), set.set_tables[mfa::SET_H_WORDS], set.set_tables[mfa::SET_H_DEPTH]);
}

}  // namespace emul
