// The part of the split path for long strings of WAVE images (nfa_set_wave_split.hip) that can be wrong without a GPU: the record of a
// chunk, the guess of its start set, what one wave does in round 0 and in a repair round, and the loop that takes a string's set through
// its chunks' records.  Templates over the primitive set P of nfa_set_wave_core.h: the kernels instantiate them with WaveDev, the host
// harness tests/emul/nfa_set_wave_split_emul.cpp with the 64-lanes-as-an-array primitives of tests/emul/wave_lanes_resume.h.
//
// The scheme is nfa_set_split_core.h's with a WAVE where that one has a lane and the wide record where that one has the 48-byte record:
//   round 0   chunk 0 from the string's true set, every other chunk from a GUESS; the records {start_used, end} are kept
//   repair    a fixed number of rounds: a chunk whose start_used is not what its predecessor ended in is walked again from there
//   resolve   one wave per string follows the records from the true set; at the first chunk that does not continue the set it holds,
//             or that ended in error, it walks the REST of the string serially.  The answer is exact whatever the guesses were.
// Per-chunk maps are not composed, for the reason nfa_set_split_core.h gives: a chunk is only ever walked from one whole set.
//
// Record: the mfa_set_state_wide layout (nfa_set_wave_core.h), 68 words -- a tag quarter, then lane l's word -- written by
// nfa_wave_state_encode, so a record whose tag is not LIVE holds no node.  Tag LIVE with the empty set = dead (absorbing); tag INVALID =
// the chunk's walk overflowed its stack, such an end joins nothing.  Two records are equal when their tags and all 64 node words are:
// the words are compared per lane and reduced with one P::any.  In a wave every value but a record's node words is wave-uniform.
#ifndef MFA_NFA_SET_WAVE_SPLIT_CORE_H
#define MFA_NFA_SET_WAVE_SPLIT_CORE_H

#include "dfa_spec_core.h"      // spec_lookback_range, spec_rest_range, SPEC_H_*, and through it split_chunk_range, split_chunks_of
#include "nfa_set_wave_core.h"

namespace mfa {

// MFA_DFA_CHUNK of a wave image.  Not from a sweep yet (DESIGN.md section 4.9 says what is measured): a device keeps at most 8 192 waves
// resident where the lane path has half a million lanes, and a chunk costs its lookback bytes on top, so the minimum is four times the
// lane path's: the lookback (kSetSplitLookback = 64, shared) then adds a sixteenth to a chunk's bytes, and a string of split_min = 64 KiB
// is still cut into 64 chunks.  Correctness does not depend on it.
static constexpr uint32_t kWaveSplitChunkMin = 1024;
// Chunks of arena a wave image's workspace reserves at the most: four per resident wave of 256 CUs x 32 waves.  The plan kernel grows the
// chunk size above it, as it does above kSplitArenaChunks for every other engine.
static constexpr uint32_t kWaveSplitArenaChunks = 32768;

// a record in registers: the tag (wave-uniform) and this lane's word of the set
template <class P>
struct WaveRec { uint32_t tag; typename P::Reg nodes; };

// record i of an array of records of this path (written by wave_rec_store: the reserved words are zero)
template <class P>
__device__ inline WaveRec<P> wave_rec_load(const uint32_t* recs, uint64_t i) {
    const uint32_t* rec = recs + i * kWaveStateWords;
    uint32_t q[4];
    P::load_tag(rec, q);
    WaveRec<P> r;
    r.tag = q[0];
    r.nodes = P::load_row(rec + 4, kWaveLanes);
    return r;
}
template <class P>
__device__ inline void wave_rec_store(uint32_t* recs, uint64_t i, const WaveRec<P>& r) {
    nfa_wave_state_encode<P>(r.tag, r.nodes, recs + i * kWaveStateWords);
}
template <class P>
__device__ inline bool wave_rec_equal(const WaveRec<P>& a, const WaveRec<P>& b) {
    return a.tag == b.tag && !P::any((a.nodes & ~b.nodes) | (b.nodes & ~a.nodes));
}
template <class P>
__device__ inline bool wave_rec_invalid(const WaveRec<P>& r) { return r.tag != kSetStateLive; }
// LIVE with the empty set
template <class P>
__device__ inline bool wave_rec_dead(const WaveRec<P>& r) { return r.tag == kSetStateLive && !P::any(r.nodes); }

template <class P>
__device__ inline WaveRec<P> wave_rec_of(uint32_t tag, const typename P::Reg& cur) {
    WaveRec<P> r;
    r.tag = tag;
    r.nodes = tag == kSetStateLive ? cur : P::zero();
    return r;
}

// The record a string enters with: the caller's record `rec` as nfa_wave_state_decode reads it (START becomes LIVE {start}; a record the
// image cannot have written becomes INVALID), or LIVE {start} for rec == nullptr (the plain call).
template <class P>
__device__ inline WaveRec<P> wave_rec_first(const NfaSetView& t, uint32_t n_nodes, const uint32_t* rec) {
    typename P::Reg cur;
    uint32_t tag = kSetStateLive;
    if (rec != nullptr) tag = nfa_wave_state_decode<P>(t, n_nodes, rec, 0u, cur);
    else cur = nfa_wave_start<P>(t);
    return wave_rec_of<P>(tag, cur);
}

// The bytes [lo, hi) from the set in cur, as a record: LIVE with the set reached (empty: the walk died, or cur was empty), INVALID on a
// stack overflow.
template <bool REV, class P>
__device__ inline WaveRec<P> wave_chunk_walk(const NfaSetView& t, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t lo, uint64_t hi, typename P::Reg& cur) {
    uint32_t tag = kSetStateLive;
    if (P::any(cur) && nfa_wave_walk_from<REV, P>(t, W, stack, bytes, lo, hi, cur) == 2u) tag = kSetStateInvalid;
    return wave_rec_of<P>(tag, cur);
}

// ---- the guess -------------------------------------------------------------------------------------------
// The start set guessed for a chunk: the set reached over the lookback bytes [from, to) from a seed.  Seeds in this order: {start}, then
// the image's home set (image_host.cpp: nfa_set_home_wide; 64 words, lane l its word l); the first whose walk neither dies nor overflows
// gives the guess, and when both fail the guess is the home set itself.  The home set is not empty, so the guess never is
// (nfa_set_split_core.h: set_spec_guess says why it must not be).
template <bool REV, class P>
__device__ inline void wave_spec_guess(const NfaSetView& t, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t from, uint64_t to, const uint32_t* home,
                                       typename P::Reg& cur) {
    cur = nfa_wave_start<P>(t);
    if (nfa_wave_walk_from<REV, P>(t, W, stack, bytes, from, to, cur) == 1u) return;
    cur = P::load_row(home, kWaveLanes);
    if (nfa_wave_walk_from<REV, P>(t, W, stack, bytes, from, to, cur) == 1u) return;
    cur = P::load_row(home, kWaveLanes);
}

// ---- round 0 ---------------------------------------------------------------------------------------------
// The wave of chunk k (scan order, bytes [lo, hi)) of the string [b, e).  first: the caller's record the string enters with, or nullptr
// for {start} (chunk 0 starts from it; a queued string's decodes to LIVE and is not empty).  Writes start_used[c] and end0[c].
template <bool REV, class P>
__device__ inline void wave_spec_round0(const NfaSetView& t, uint32_t n_nodes, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e, uint64_t lo,
                                        uint64_t hi, uint32_t k, const uint32_t* first, const uint32_t* home, uint32_t lookback, uint32_t* start_used, uint32_t* end0,
                                        uint64_t c) {
    WaveRec<P> used;
    if (k == 0u) used = wave_rec_first<P>(t, n_nodes, first);
    else {
        uint64_t from, to;
        spec_lookback_range<REV>(b, e, lo, hi, lookback, &from, &to);
        typename P::Reg g;
        wave_spec_guess<REV, P>(t, W, stack, bytes, from, to, home, g);
        used = wave_rec_of<P>(kSetStateLive, g);
    }
    wave_rec_store<P>(start_used, c, used);
    if (used.tag == kSetStateLive) {
        typename P::Reg cur = used.nodes;
        wave_rec_store<P>(end0, c, wave_chunk_walk<REV, P>(t, W, stack, bytes, lo, hi, cur));
    } else wave_rec_store<P>(end0, c, used);
}

// ---- repair ----------------------------------------------------------------------------------------------
// set_spec_needs_rewalk's rule on wide records: chunk k of a string, walked from `used`; prev: what its predecessor ended in as the round
// before left it.  An INVALID end joins nothing: there is no set to walk from, the resolve step stops in front of it.
template <class P>
__device__ inline bool wave_spec_needs_rewalk(uint32_t k, const WaveRec<P>& used, const WaveRec<P>& prev) {
    return k != 0u && !wave_rec_invalid<P>(prev) && !wave_rec_equal<P>(used, prev);
}

// The wave of arena chunk c = chunk k of its string in one repair round: reads start_used[c], end_prev[c - 1] and end_prev[c], writes
// start_used[c] and end_next[c] -- no word another wave of the same round writes.  true: the bytes were walked again (a chunk behind a
// dead one gets the dead record without a walk and is not counted).
template <bool REV, class P>
__device__ inline bool wave_spec_repair(const NfaSetView& t, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t lo, uint64_t hi, uint32_t k,
                                        uint32_t* start_used, const uint32_t* end_prev, uint32_t* end_next, uint64_t c) {
    if (k != 0u) {
        const WaveRec<P> used = wave_rec_load<P>(start_used, c);
        const WaveRec<P> prev = wave_rec_load<P>(end_prev, c - 1u);
        if (wave_spec_needs_rewalk<P>(k, used, prev)) {
            wave_rec_store<P>(start_used, c, prev);
            if (wave_rec_dead<P>(prev)) { wave_rec_store<P>(end_next, c, prev); return false; }
            typename P::Reg cur = prev.nodes;
            wave_rec_store<P>(end_next, c, wave_chunk_walk<REV, P>(t, W, stack, bytes, lo, hi, cur));
            return true;
        }
    }
    wave_rec_store<P>(end_next, c, wave_rec_load<P>(end_prev, c));
    return false;
}

// ---- resolve ---------------------------------------------------------------------------------------------
// The records of one string's nc chunks, in scan order; *held = the record of the string's true set (LIVE).  Follows the records while
// they continue the set held.  Returns nc when they do to the end or the set died on the way (*held = the string's final record), else
// the index c of the first chunk that was walked from another set than *held or that ended INVALID (*held = the true set in front of
// chunk c): the caller walks the string from that chunk's scan begin to the string's scan end from *held.
template <class P>
__device__ inline uint32_t wave_spec_resolve(const uint32_t* start_used, const uint32_t* end, uint32_t nc, WaveRec<P>* held) {
    WaveRec<P> h = *held;
    uint32_t c = 0;
    for (; c < nc && !wave_rec_dead<P>(h); c++) {
        if (!wave_rec_equal<P>(wave_rec_load<P>(start_used, c), h)) break;
        const WaveRec<P> en = wave_rec_load<P>(end, c);
        if (wave_rec_invalid<P>(en)) break;
        h = en;
    }
    *held = h;
    return wave_rec_dead<P>(h) ? nc : c;
}

// One wave, one queued string [b, e) of nc chunks of `chunk` bytes whose records start at start_used / end_fin: the record behind the
// string, from `first` (the caller's record it enters with, nullptr: {start}).  *serial = the bytes walked serially (0: the records
// joined up).
template <bool REV, class P>
__device__ inline WaveRec<P> wave_spec_resolve_string(const NfaSetView& t, uint32_t n_nodes, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e,
                                                      uint64_t chunk, uint32_t nc, const uint32_t* start_used, const uint32_t* end_fin, const uint32_t* first,
                                                      uint64_t* serial) {
    WaveRec<P> held = wave_rec_first<P>(t, n_nodes, first);            // (a START record becomes LIVE {start}, as round 0 wrote it)
    *serial = 0u;
    if (held.tag != kSetStateLive) return held;
    const uint32_t c = wave_spec_resolve<P>(start_used, end_fin, nc, &held);
    if (c < nc) {
        uint64_t lo, hi, from, to;
        split_chunk_range<REV>(b, e, chunk, nc, c, &lo, &hi);
        spec_rest_range<REV>(b, e, lo, hi, &from, &to);
        typename P::Reg cur = held.nodes;
        held = wave_chunk_walk<REV, P>(t, W, stack, bytes, from, to, cur);
        *serial = to - from;
    }
    return held;
}

// the result byte of a string whose final record is r: what nfa_wave_resume_piece answers
template <class P>
__device__ inline uint8_t wave_rec_result(const NfaSetView& t, uint32_t W, const WaveRec<P>& r) {
    return r.tag == kSetStateLive ? nfa_wave_accepts<P>(t, W, r.nodes) : (uint8_t)2;
}

// ---- the hand-over in nfa_set_wave_resume_kernel ---------------------------------------------------------
// nfa_wave_resume_piece behind its decode: the kernel decodes, asks whether the piece is queued (a LIVE, non-empty set only), and walks
// here what is not.  The record at rec is replaced by the one behind the piece; returns the result byte.
template <bool REV, class P>
__device__ inline uint8_t wave_resume_entered(const NfaSetView& t, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e, uint32_t tag,
                                              typename P::Reg& cur, uint32_t* rec) {
    if (tag == kSetStateLive && P::any(cur) && nfa_wave_walk_from<REV, P>(t, W, stack, bytes, b, e, cur) == 2u) tag = kSetStateInvalid;
    nfa_wave_state_encode<P>(tag, cur, rec);
    return tag == kSetStateLive ? nfa_wave_accepts<P>(t, W, cur) : (uint8_t)2;
}

}  // namespace mfa

#endif
