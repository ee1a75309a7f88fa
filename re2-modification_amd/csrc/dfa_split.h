// What the one-string-per-lane kernels (kernels.hip, dfa_spec.hip) and the split paths (dfa_split.hip, dfa_spec.hip) share on the device:
// the plan header, the queue of long strings, the one place where a string is handed from the former to the latter, and the policy that
// says where a string's state comes from and where it goes (every kernel has a plain and a resume instantiation of ONE body).
#ifndef MFA_DFA_SPLIT_H
#define MFA_DFA_SPLIT_H

#include "dfa_resume_core.h"      // and dfa_split_core.h
#include "memless_plan.h"         // kSplitChunkMin and the other figures of the host side

namespace mfa {

// plan header, 32-bit words of device memory, zeroed in front of every launch that uses it
enum : uint32_t {
    SPLIT_H_SEEN = 0,        // strings with len >= split_min that asked for a queue slot (the main kernel counts them)
    SPLIT_H_STRINGS = 1,     // strings queued = min(seen, queue capacity)           (the plan kernel writes this and the following)
    SPLIT_H_CHUNKS = 2,      // chunks they are cut into
    SPLIT_H_CHUNK = 3,       // chunk size in bytes
    SPLIT_H_WORDS = 8,
};

struct SplitEntry {
    uint64_t sid;            // string number
    uint32_t first, nc;      // its first map in the arena, its chunk count; maps are stored in scan order
    uint32_t dead_at, pad;   // lowest scan index of a chunk whose map is all 0 (0xffffffff: none known): later chunks need no walk
};
static_assert(sizeof(SplitEntry) == kSplitEntryBytes && kDfaRow == kMemlessRow, "memless_plan.h lays out the workspace and sizes the tables");

// argument of the main kernels.  split_min == 0: the split path is off, the kernel behaves as it always has.
struct SplitArgs {
    uint64_t    split_min;
    uint32_t*   hdr;         // NULL: no split kernels follow this launch -- every string is walked here, a long one is reported to *seen
    SplitEntry* queue;
    uint32_t    qcap;
    uint32_t*   seen;        // pinned host word (may be NULL): a launch with the split kernels behind it writes 1 (met no long string) or 2, one without writes 3 when it meets one
};

// A lane of a main kernel that holds a string with len >= split_min calls this.  true: the string is on the queue, the lane treats it
// as empty and leaves its result byte alone (dfa_fold_kernel writes it, later on the same stream).  false: the lane walks it.
// NO STRING IS LOST: the lane that skips a string is the lane that was given the queue slot for it, in this very call -- there is no
// second place that decides what "long" means.  A full queue, or a launch without split kernels behind it, answers false.
#ifdef __HIPCC__
__device__ __forceinline__ bool split_take(const SplitArgs& sp, uint64_t sid) {
    if (sp.hdr == nullptr) {
        if (sp.seen != nullptr) *sp.seen = 3u;
        return false;
    }
    const uint32_t slot = atomicAdd(&sp.hdr[SPLIT_H_SEEN], 1u);
    if (slot >= sp.qcap) return false;
    sp.queue[slot].sid = sid;
    return true;
}

// ---- one lane per chunk (dfa_spec.hip, nfa_set_split.hip) -------------------------------------------------
struct SpecChunk { uint32_t q, k; uint64_t b, e, lo, hi; };     // chunk k (scan order) of queued string q = [b, e): the bytes [lo, hi)

// the string of arena chunk c: the last queue entry with first <= c (c < the plan's chunk count, n_q >= 1)
template <bool REV>
__device__ __forceinline__ SpecChunk spec_chunk(const SplitEntry* __restrict__ queue, uint32_t n_q, const uint64_t* __restrict__ offsets, uint32_t chunk, uint32_t c) {
    uint32_t lo = 0u, hi = n_q;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (queue[mid].first <= c) lo = mid; else hi = mid;
    }
    SpecChunk r;
    r.q = lo; r.k = c - queue[lo].first;
    const uint64_t sid = queue[lo].sid;
    r.b = offsets[sid]; r.e = offsets[sid + 1u];
    split_chunk_range<REV>(r.b, r.e, chunk, queue[lo].nc, r.k, &r.lo, &r.hi);
    return r;
}

// ---- state policy --------------------------------------------------------------------------------------
// RESUME == false (mfa_match_batch): every string starts at state 1 = {start}, is always walked, and results[sid] = accept_tab[state].
// RESUME == true (mfa_match_batch_resume): the state is read from and written back to states[sid] under the rules of dfa_resume_core.h
// (resume_enter, resume_walks, resume_result), and results may be NULL.  A compile-time parameter: the plain instantiations read no
// word of `states` and test nothing.
// What a lane does with string sid of `len` bytes: the state it enters with (`st`, a plain state number), whether it walks the bytes
// (`walks`; false: the state leaves as it came), and whether the split path has taken the string (`taken`: the lane then leaves word
// and result alone -- the fold or the resolve kernel behind it writes them).  Dead and invalid words are never queued.
struct StateEntry { uint32_t st; bool walks, taken; };

template <bool RESUME>
__device__ __forceinline__ StateEntry state_begin(const uint32_t* states, uint32_t n_states, uint64_t sid, uint64_t len, const SplitArgs& sp) {
    StateEntry r;
    r.st = RESUME ? resume_enter(states[sid], n_states, len) : 1u;
    r.walks = !RESUME || resume_walks(r.st);
    r.taken = r.walks && sp.split_min != 0u && len >= sp.split_min && split_take(sp, sid);
    return r;
}

template <bool RESUME>
__device__ __forceinline__ void state_end(uint32_t* states, uint8_t* results, const uint8_t* accept_tab, uint64_t sid, uint32_t st) {
    if (RESUME) {
        states[sid] = st;
        if (results != nullptr) results[sid] = resume_result(accept_tab, st);
    } else {
        results[sid] = accept_tab[st];
    }
}

// a queued string in the kernel that finishes it (fold, resolve): it was taken with a state that walks, still in its word
template <bool RESUME>
__device__ __forceinline__ uint32_t state_of_queued(const uint32_t* states, uint64_t sid) { return RESUME ? states[sid] : 1u; }
#endif

}  // namespace mfa

#endif
