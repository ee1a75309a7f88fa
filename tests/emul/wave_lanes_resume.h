// TEST INFRASTRUCTURE ONLY: the host form of the primitives csrc/nfa_set_wave_core.h adds for strings in pieces (the record of
// mfa_match_batch_resume_set_wide: a tag quarter and 64 node words, lane l word l), on top of the 64-lanes-as-an-array primitives of
// wave_lanes.h (tests/emul/nfa_set_wave_resume_emul.cpp).  Nothing in the product includes this.
#pragma once
#include "wave_lanes.h"

namespace emul {

struct WaveHostResume : WaveHost {
    // every one of the 64 lanes stores its word: a record shorter than 272 bytes is a write a sanitizer sees
    static void store_row(uint32_t* row, const Reg& r) { memcpy(row, r.w, sizeof r.w); }
    // the nodes lane l's word has, of an image of n_nodes
    static Reg have(uint32_t n_nodes) {
        Reg r;
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t first = l * 32u;
            r.w[l] = n_nodes >= first + 32u ? 0xffffffffu : n_nodes > first ? (1u << (n_nodes - first)) - 1u : 0u;
        }
        return r;
    }
    // the tag quarter: one aligned 16-byte read, one aligned 16-byte store of (tag, 0, 0, 0)
    static void load_tag(const uint32_t* rec, uint32_t (&q)[4]) {
        if ((uintptr_t)rec & 15u) abort();
        memcpy(q, rec, 16);
    }
    static void store_tag(uint32_t* rec, uint32_t tag) {
        if ((uintptr_t)rec & 15u) abort();
        const uint32_t q[4] = {tag, 0u, 0u, 0u};
        memcpy(rec, q, 16);
    }
};

}  // namespace emul
