// The part of the split path for long strings of LARGE-table memory-less automata (dfa_spec.hip: 255 state sets and more, table in
// L2) that can be wrong without a GPU: which bytes a chunk looks back over, the guess of its start state, when a chunk is walked
// again, the loop that takes a string's state through its chunks' records, and the host's choice of the image's home state.
// Included by the kernels and, with the one-lane shim of tests/emul/, by the host harness tests/emul/dfa_spec_emul.cpp.
//
// A chunk of a long string is a piece with a start state (dfa_resume_core.h: resume_piece_big walks one).  The scheme of
// dfa_split.hip walks every chunk from EVERY start state, which a table of up to 2^20 state sets forbids.  Here every chunk is
// walked from ONE state:
//   round 0   chunk 0 from the string's true state, every other chunk from a GUESS; the record {start_used, end} is kept
//   repair    a fixed number of rounds: a chunk whose start_used is not what its predecessor ended in is walked again from there
//   resolve   one lane per string follows the records from the true state; at the first record that does not continue the state
//             it holds, it walks the REST of the string serially.  This makes the answer exact whatever the guesses were.
// The guess is a matter of speed only.  Two pathologies, both slow and never wrong: a text on which both seeds of the guess die
// (the guess is then the home state itself), and a table whose state never converges (a counter, (a^150)*): guesses stay wrong,
// every round repairs one more chunk per string, and the resolve step walks what is left.
#ifndef MFA_DFA_SPEC_CORE_H
#define MFA_DFA_SPEC_CORE_H

#include "dfa_resume_core.h"

namespace mfa {

// words of the plan header (dfa_split.h) behind the plan's own: what the speculative path did
enum : uint32_t {
    SPEC_H_REWALKED = 4,          // chunks walked again by a repair round
    SPEC_H_SERIAL_STRINGS = 5,    // strings whose records did not join up: the resolve step walked their rest serially
    SPEC_H_SERIAL_BYTES = 6,      // ... and how many bytes that was (64 bits: words 6 and 7)
};

static constexpr uint32_t kSpecLookback = 256;      // MFA_DFA_SPEC_LOOKBACK
static constexpr uint32_t kSpecRounds = 3;          // MFA_DFA_SPEC_ROUNDS
static constexpr uint32_t kSpecRoundsMax = 8;

// ---- the guess -----------------------------------------------------------------------------------------
// The `lookback` bytes that PRECEDE the chunk [lo, hi) of the string [b, e) in scan order, clipped at the string's scan start: below
// lo for a forward scan, above hi for a reversed one (which scans from e down to b).  Empty for lookback 0 and for the first chunk.
template <bool REV>
__host__ __device__ inline void spec_lookback_range(uint64_t b, uint64_t e, uint64_t lo, uint64_t hi, uint64_t lookback, uint64_t* from, uint64_t* to) {
    if (REV) { *from = hi; *to = e - hi < lookback ? e : hi + lookback; }
    else     { *from = lo - b < lookback ? b : lo - lookback; *to = lo; }
}

// The start state guessed for a chunk: the state reached over the lookback bytes [from, to) from a seed.  Seeds in this order: state 1
// ({start}), then the image's home state (spec_home_state); the first whose walk does not die gives the guess, and when both die the
// guess is the home state itself.  home != 0, so the guess is never 0: the dead state is absorbing, a chunk "walked" from it would
// have start_used == end == 0 for ever and no later round could tell it from a chunk whose predecessor really died.
template <bool REV, class T>
__device__ inline uint32_t spec_guess(const T* trans, const uint8_t* byte_class, uint32_t n_classes, const uint8_t* bytes, uint64_t from, uint64_t to,
                                      uint32_t home) {
    uint32_t g = resume_piece_big<REV, T>(trans, byte_class, n_classes, bytes, from, to, 1u);
    if (g == 0u && home != 1u) g = resume_piece_big<REV, T>(trans, byte_class, n_classes, bytes, from, to, home);
    return g != 0u ? g : home;
}

// ---- repair --------------------------------------------------------------------------------------------
// chunk k (scan order) of a string, walked from start_used; prev_end: the state its predecessor ended in as the round before left it
__host__ __device__ inline bool spec_needs_rewalk(uint32_t k, uint32_t start_used, uint32_t prev_end) { return k != 0u && start_used != prev_end; }

// ---- resolve -------------------------------------------------------------------------------------------
// The records of one string's nc chunks, in scan order; *cur = the string's true start state.  Follows the records while they continue
// the state held.  Returns nc when they do to the end or the state died on the way (*cur = the string's final state), else the index
// c of the first chunk that was walked from another state than *cur (= the true state in front of chunk c): the caller walks the
// string from that chunk's scan begin to the string's scan end from *cur.
__host__ __device__ inline uint32_t spec_resolve(const uint32_t* start_used, const uint32_t* end, uint32_t nc, uint32_t* cur) {
    uint32_t st = *cur, c = 0;
    for (; c < nc && st != 0u; c++) {
        if (start_used[c] != st) break;
        st = end[c];
    }
    *cur = st;
    return st == 0u ? nc : c;
}

// the bytes the resolve step walks serially when chunk c of nc (range [lo, hi)) is the first that does not join up
template <bool REV>
__host__ __device__ inline void spec_rest_range(uint64_t b, uint64_t e, uint64_t lo, uint64_t hi, uint64_t* from, uint64_t* to) {
    *from = REV ? b : lo;
    *to = REV ? hi : e;
}

// ---- the home state (host, once per image) -------------------------------------------------------------
// The second seed of the guess, for texts on which a walk from {start} dies in mid-text (a regex with a literal prefix in front of a
// loop: the prefix is not found at an arbitrary offset).  The state a deterministic pseudo-random walk of the table from state 1
// ends in: every step draws a byte class (xorshift32, fixed seed) and takes the first class from there on, cyclically, whose
// transition is not into state 0; a state with no such class ends the walk.  4096 steps: far beyond any literal prefix, so the walk
// ends where long texts spend their time -- inside the automaton's loops -- when it has any.  Never 0.
inline uint32_t spec_home_state(const uint32_t* trans, uint32_t n_states, uint32_t n_classes) {
    if (n_states < 2u || n_classes == 0u) return 1u;
    uint32_t st = 1u, x = 0x9e3779b9u;
    for (uint32_t step = 0; step < 4096u; step++) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        const uint32_t c0 = x % n_classes;
        uint32_t nx = 0u;
        for (uint32_t k = 0; k < n_classes && nx == 0u; k++) nx = trans[(size_t)st * n_classes + (c0 + k) % n_classes];
        if (nx == 0u) break;
        st = nx;
    }
    return st;
}

}  // namespace mfa

#endif
