// The part of the resume path for memory-less automata (the RESUME instantiations of the kernels, dfa_split.h: a string given in pieces,
// its state carried from call to call) that can be wrong without a GPU: which state a piece is entered with, when that state is an error, the walk of one piece
// from a given state, the answer that belongs to a state.  Included by the kernels and, with the one-lane shim of tests/emul/, by
// the host harness tests/emul/dfa_resume_emul.cpp.
//
// The state of a tabulated automaton between two bytes of its input is ONE number, the state set it is in (0 = the empty set, dead;
// 1 = {start}); the walk is a fold over the input, so a string may be cut anywhere and the pieces walked one call after the other.
// The fold from a given state over the maps of a long piece's chunks is split_fold_run (dfa_split_core.h) started at that state.
#ifndef MFA_DFA_RESUME_CORE_H
#define MFA_DFA_RESUME_CORE_H

#include "dfa_split_core.h"

namespace mfa {

static constexpr uint32_t kResumeInvalid = 0xffffffffu;      // MFA_DFA_STATE_INVALID: sticky, answered 2
static constexpr uint64_t kResumeMaxPiece = 0x00ffffffu;     // MFA_MAX_STRING_BYTES: per piece, the sum of a string's pieces has no limit

// The state a piece of `len` bytes is entered with, given the word the caller handed in: that word if it names a state set of this
// image and the piece is within the limit, else the error state (an error state handed in names no state set, so it stays).
__host__ __device__ inline uint32_t resume_enter(uint32_t st_in, uint32_t n_states, uint64_t len) {
    return (st_in < n_states && len <= kResumeMaxPiece) ? st_in : kResumeInvalid;
}

// false: the piece's bytes are not looked at -- the dead state is absorbing, the error state is sticky; the state leaves as it came
__host__ __device__ inline bool resume_walks(uint32_t st) { return st != 0u && st != kResumeInvalid; }

// the result byte of a string that has reached st: what mfa_match_batch answers for the concatenation of the pieces so far
__host__ __device__ inline uint8_t resume_result(const uint8_t* accept_tab, uint32_t st) {
    return st == kResumeInvalid ? (uint8_t)2 : accept_tab[st];
}

// One lane, the fused table of dfa_walk_kernel (up to 127 state sets): the state reached from st over the piece [b, e), scanned
// upwards or (REV) downwards.  Plain state numbers in and out.
template <bool REV>
__device__ inline uint32_t resume_piece(const uint16_t* s_next, const uint8_t* bytes, uint64_t b, uint64_t e, uint32_t st) {
    return split_chunk_walk<REV>(s_next, bytes, b, e, st * kDfaRow) / kDfaRow;
}

// The same on the plain table trans[state][class] of dfa_spec_big_kernel (16- or 32-bit entries, any number of state sets).
template <bool REV, class T>
__device__ inline uint32_t resume_piece_big(const T* trans, const uint8_t* byte_class, uint32_t n_classes, const uint8_t* bytes, uint64_t b,
                                            uint64_t e, uint32_t st) {
    uint64_t p = REV ? e : b;
    while ((REV ? p > b : p < e) && st != 0u) {
        const uint64_t blk = (REV ? p - 1u : p) & ~(uint64_t)15;
        const uint4 d = split_load16(bytes, blk);
        const uint32_t w[4] = {d.x, d.y, d.z, d.w};
        const uint32_t lo = b > blk ? (uint32_t)(b - blk) : 0u, hi = (e - blk) < 16u ? (uint32_t)(e - blk) : 16u;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int k = REV ? 15 - j : j;
            if ((uint32_t)k >= lo && (uint32_t)k < hi) st = trans[(uint64_t)st * n_classes + byte_class[(w[k >> 2] >> (8 * (k & 3))) & 0xffu]];
        }
        p = REV ? blk : blk + 16u;
    }
    return st;
}

}  // namespace mfa

#endif
