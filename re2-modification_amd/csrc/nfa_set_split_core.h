// The part of the split path for long strings of SET-WALK images (nfa_set_split.hip) that can be wrong without a GPU: the record of a
// chunk, the guess of its start set, what one lane does in round 0 and in a repair round, and the loop that takes a string's set through
// its chunks' records.  Included by the kernels and, with the one-lane shim of tests/emul/, by the host harness
// tests/emul/nfa_set_split_emul.cpp.
//
// The scheme is dfa_spec_core.h's, with a node set where that one has a state number (a tabulated state number IS a node set):
//   round 0   chunk 0 from the string's true set, every other chunk from a GUESS; the records {start_used, end} are kept
//   repair    a fixed number of rounds: a chunk whose start_used is not what its predecessor ended in is walked again from there
//   resolve   one lane per string follows the records from the true set; at the first chunk that does not continue the set it holds,
//             or that ended in error, it walks the REST of the string serially.  The answer is exact whatever the guesses were.
// Per-chunk maps are NOT composed here: the reference's step skips edges into nodes already visited in this byte, and the visited mask is
// shared by all nodes of the set, so step(A u B) != step(A) u step(B).  A chunk is only ever walked from one whole set.
//
// Record: the mfa_set_state layout (nfa_set_core.h), twelve words as three 16-byte quarters, written by nfa_set_state_encode and read by
// nfa_set_state_decode.  Tag LIVE with the empty set = dead (absorbing); tag INVALID = the chunk's walk overflowed its stack, such an end
// joins nothing.  Two records are equal when their tags and all eight node words are.
#ifndef MFA_NFA_SET_SPLIT_CORE_H
#define MFA_NFA_SET_SPLIT_CORE_H

#include "dfa_spec_core.h"      // spec_lookback_range, spec_rest_range, SPEC_H_*, and through it split_chunk_range, split_chunks_of
#include "nfa_set_core.h"

namespace mfa {

// From the sweep of tools/nfa_setwalk.py long (profiles/r13_nfa_set_split.jsonl); correctness does not depend on them.
// A batch of long strings has far fewer chunks than the device has lanes until the arena is full, so a call takes as long as ONE lane
// takes for chunk + lookback bytes: the smallest chunk swept wins by far on the slow image (k = 20: 16.6 ms at 256, 28.8 at 512, 55 at
// 1024) and loses a tenth on the fast one; the lookback costs its bytes and repaired nothing on the swept texts at any size, 64 is three
// times the k = 20 image's memory; repair rounds that find nothing to do cost nothing measurable.
static constexpr uint32_t kSetSplitChunkMin = 256;      // MFA_DFA_CHUNK of a set-walk image
static constexpr uint32_t kSetSplitLookback = 64;       // MFA_SET_SPLIT_LOOKBACK
static constexpr uint32_t kSetSplitRounds = 3;          // MFA_SET_SPLIT_ROUNDS, at most kSpecRoundsMax

static constexpr uint32_t kSetRecQuarters = 3;          // 16-byte quarters per record

// the image's home set (image_host.cpp: nfa_set_home), a kernel argument; words beyond the image's W are zero
struct SetHome { uint32_t w[kSetStateNodeWords]; };

// ---- records ---------------------------------------------------------------------------------------------
struct SetRec { uint4 q0, q1, q2; };

__host__ __device__ __forceinline__ SetRec set_rec_load(const uint4* recs, uint64_t i) {
    const uint4* p = recs + i * kSetRecQuarters;
    SetRec r;
    r.q0 = p[0]; r.q1 = p[1]; r.q2 = p[2];
    return r;
}
__host__ __device__ __forceinline__ void set_rec_store(uint4* recs, uint64_t i, const SetRec& r) {
    uint4* p = recs + i * kSetRecQuarters;
    p[0] = r.q0; p[1] = r.q1; p[2] = r.q2;
}
__host__ __device__ __forceinline__ bool set_rec_equal(const SetRec& a, const SetRec& b) {
    return a.q0.x == b.q0.x && a.q1.x == b.q1.x && a.q1.y == b.q1.y && a.q1.z == b.q1.z && a.q1.w == b.q1.w && a.q2.x == b.q2.x && a.q2.y == b.q2.y &&
           a.q2.z == b.q2.z && a.q2.w == b.q2.w;
}
__host__ __device__ __forceinline__ bool set_rec_invalid(const SetRec& r) { return r.q0.x != kSetStateLive; }
// LIVE with the empty set
__host__ __device__ __forceinline__ bool set_rec_dead(const SetRec& r) {
    return r.q0.x == kSetStateLive && (r.q1.x | r.q1.y | r.q1.z | r.q1.w | r.q2.x | r.q2.y | r.q2.z | r.q2.w) == 0u;
}

template <int W>
__host__ __device__ __forceinline__ SetRec set_rec_of(uint32_t tag, const uint32_t (&cur)[W]) {
    SetRec r;
    nfa_set_state_encode<W>(tag, cur, r.q0, r.q1, r.q2);
    return r;
}
// the set of a record of this path (or of the caller's, for chunk 0 of a piece): LIVE or INVALID, as nfa_set_state_decode says
template <int W>
__host__ __device__ __forceinline__ uint32_t set_rec_set(const NfaSetView& t, uint32_t n_nodes, const SetRec& r, uint32_t (&cur)[W]) {
    return nfa_set_state_decode<W>(t, n_nodes, r.q0, r.q1, r.q2, 0u, cur);
}

template <int W>
__host__ __device__ __forceinline__ uint32_t set_any(const uint32_t (&cur)[W]) {
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < W; k++) any |= cur[k];
    return any;
}

// The bytes [lo, hi) from the set in cur, as a record: LIVE with the set reached (empty: the walk died, or cur was empty), INVALID on a
// stack overflow.
template <bool REV, int W>
__device__ inline SetRec set_chunk_walk(const NfaSetView& t, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t lo, uint64_t hi, uint32_t (&cur)[W]) {
    uint32_t tag = kSetStateLive;
    if (set_any<W>(cur) != 0u && nfa_set_walk_from<REV, W>(t, stack, stride, bytes, lo, hi, cur) == 2u) tag = kSetStateInvalid;
    return set_rec_of<W>(tag, cur);
}

// ---- the guess -------------------------------------------------------------------------------------------
// The start set guessed for a chunk: the set reached over the lookback bytes [from, to) from a seed.  Seeds in this order: {start}, then
// the image's home set; the first whose walk neither dies nor overflows gives the guess, and when both fail the guess is the home set
// itself.  The home set is not empty, so the guess never is: the empty set is absorbing, a chunk "walked" from it would have
// start_used == end == dead for ever and no later round could tell it from a chunk whose predecessor really died.
template <bool REV, int W>
__device__ inline void set_spec_guess(const NfaSetView& t, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t from, uint64_t to, const SetHome& home,
                                      uint32_t (&cur)[W]) {
    nfa_set_start<W>(t, cur);
    if (nfa_set_walk_from<REV, W>(t, stack, stride, bytes, from, to, cur) == 1u) return;
#pragma unroll
    for (int k = 0; k < W; k++) cur[k] = home.w[k];
    if (nfa_set_walk_from<REV, W>(t, stack, stride, bytes, from, to, cur) == 1u) return;
#pragma unroll
    for (int k = 0; k < W; k++) cur[k] = home.w[k];
}

// ---- round 0 ---------------------------------------------------------------------------------------------
// The lane of chunk k (scan order, bytes [lo, hi)) of the string [b, e).  first: the record the string enters with (chunk 0 starts from
// it; a queued string's is LIVE or START and not empty).  Writes start_used[c] and end0[c].
template <bool REV, int W>
__device__ inline void set_spec_round0(const NfaSetView& t, uint32_t n_nodes, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t b, uint64_t e,
                                       uint64_t lo, uint64_t hi, uint32_t k, const SetRec& first, const SetHome& home, uint32_t lookback, uint4* start_used,
                                       uint4* end0, uint64_t c) {
    uint32_t cur[W];
    uint32_t tag = kSetStateLive;
    if (k == 0u) tag = set_rec_set<W>(t, n_nodes, first, cur);
    else {
        uint64_t from, to;
        spec_lookback_range<REV>(b, e, lo, hi, lookback, &from, &to);
        set_spec_guess<REV, W>(t, stack, stride, bytes, from, to, home, cur);
    }
    const SetRec used = set_rec_of<W>(tag, cur);
    set_rec_store(start_used, c, used);
    set_rec_store(end0, c, tag == kSetStateLive ? set_chunk_walk<REV, W>(t, stack, stride, bytes, lo, hi, cur) : used);
}

// ---- repair ----------------------------------------------------------------------------------------------
// chunk k of a string, walked from `used`; prev: what its predecessor ended in as the round before left it.  An INVALID end joins nothing:
// there is no set to walk from, the resolve step stops in front of it.
__host__ __device__ inline bool set_spec_needs_rewalk(uint32_t k, const SetRec& used, const SetRec& prev) {
    return k != 0u && !set_rec_invalid(prev) && !set_rec_equal(used, prev);
}

// The lane of arena chunk c = chunk k of its string in one repair round: reads start_used[c], end_prev[c - 1] and end_prev[c], writes
// start_used[c] and end_next[c] -- no word another lane of the same round writes.  true: the bytes were walked again (a chunk behind a
// dead one gets the dead record without a walk and is not counted).
template <bool REV, int W>
__device__ inline bool set_spec_repair(const NfaSetView& t, uint32_t n_nodes, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t lo, uint64_t hi,
                                       uint32_t k, uint4* start_used, const uint4* end_prev, uint4* end_next, uint64_t c) {
    const SetRec used = set_rec_load(start_used, c);
    if (k != 0u) {
        const SetRec prev = set_rec_load(end_prev, c - 1u);
        if (set_spec_needs_rewalk(k, used, prev)) {
            set_rec_store(start_used, c, prev);
            if (set_rec_dead(prev)) { set_rec_store(end_next, c, prev); return false; }
            uint32_t cur[W];
            (void)set_rec_set<W>(t, n_nodes, prev, cur);
            set_rec_store(end_next, c, set_chunk_walk<REV, W>(t, stack, stride, bytes, lo, hi, cur));
            return true;
        }
    }
    set_rec_store(end_next, c, set_rec_load(end_prev, c));
    return false;
}

// ---- resolve ---------------------------------------------------------------------------------------------
// The records of one string's nc chunks, in scan order; *held = the record of the string's true set (LIVE).  Follows the records while
// they continue the set held.  Returns nc when they do to the end or the set died on the way (*held = the string's final record), else
// the index c of the first chunk that was walked from another set than *held or that ended INVALID (*held = the true set in front of
// chunk c): the caller walks the string from that chunk's scan begin to the string's scan end from *held.
__host__ __device__ inline uint32_t set_spec_resolve(const uint4* start_used, const uint4* end, uint32_t nc, SetRec* held) {
    SetRec h = *held;
    uint32_t c = 0;
    for (; c < nc && !set_rec_dead(h); c++) {
        if (!set_rec_equal(set_rec_load(start_used, c), h)) break;
        const SetRec en = set_rec_load(end, c);
        if (set_rec_invalid(en)) break;
        h = en;
    }
    *held = h;
    return set_rec_dead(h) ? nc : c;
}

// One lane, one queued string [b, e) of nc chunks of `chunk` bytes whose records start at start_used / end_fin: the record behind the
// string, from `first` (the record it enters with).  *serial = the bytes walked serially (0: the records joined up).
template <bool REV, int W>
__device__ inline SetRec set_spec_resolve_string(const NfaSetView& t, uint32_t n_nodes, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t b, uint64_t e,
                                                 uint64_t chunk, uint32_t nc, const uint4* start_used, const uint4* end_fin, const SetRec& first, uint64_t* serial) {
    uint32_t cur[W];
    const uint32_t tag = set_rec_set<W>(t, n_nodes, first, cur);
    SetRec held = set_rec_of<W>(tag, cur);                              // (a START record becomes LIVE {start}, as round 0 wrote it)
    *serial = 0u;
    if (tag != kSetStateLive) return held;
    const uint32_t c = set_spec_resolve(start_used, end_fin, nc, &held);
    if (c < nc) {
        uint64_t lo, hi, from, to;
        split_chunk_range<REV>(b, e, chunk, nc, c, &lo, &hi);
        spec_rest_range<REV>(b, e, lo, hi, &from, &to);
        (void)set_rec_set<W>(t, n_nodes, held, cur);
        held = set_chunk_walk<REV, W>(t, stack, stride, bytes, from, to, cur);
        *serial = to - from;
    }
    return held;
}

// the result byte of a string whose final record is r
template <int W>
__host__ __device__ inline uint8_t set_rec_result(const NfaSetView& t, uint32_t n_nodes, const SetRec& r) {
    uint32_t cur[W];
    const uint32_t tag = set_rec_set<W>(t, n_nodes, r, cur);
    return nfa_set_state_result<W>(t, tag, cur);
}

}  // namespace mfa

#endif
