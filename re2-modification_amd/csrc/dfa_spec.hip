// Memory-less automata whose table is walked in L2 (255 to 2^20 state sets): the main kernel, and its long strings cut across the whole GPU
// (gfx950).  dfa_split.hip walks every chunk from every start state; that is out of the question here, so every chunk is walked from
// ONE state -- a guess -- and wrong guesses are repaired a bounded number of times, then resolved exactly (dfa_spec_core.h has the scheme
// and is checked on the CPU: tests/emul).  Queue, plan, chunk geometry, knobs and the quiet-workspace rule are dfa_split.hip's:
//   memset(header) -> dfa_spec_big_kernel (queues long strings: split_take) -> dfa_plan_kernel -> dfa_spec_walk_kernel
//     -> MFA_DFA_SPEC_ROUNDS x dfa_spec_repair_kernel -> dfa_spec_resolve_kernel
// all on the caller's stream, with no read-back; the number of launches is fixed when the call is enqueued.  Successive launches on one
// stream are the only ordering: no kernel here spins or waits for another workgroup, every loop is bounded by a chunk's or a string's bytes.
// Records: per chunk start_used and TWO end words.  Repair round r reads the ends round r - 1 left in end[(r - 1) & 1] and writes every
// chunk's end to end[r & 1] (walked again, or copied), so no lane reads a word another lane of the same launch writes; start_used[c]
// is read and written by the lane of chunk c alone.
#include <hip/hip_runtime.h>

#include "mfa_internal.h"
#include "dfa_spec_core.h"

namespace mfa {

// ---- main kernel ------------------------------------------------------------------------------------------
// THE kernel for tables in L2 (launch_dfa_walk, launch_dfa_resume: spec_main is the one place that launches it).  One string per lane, 32-bit
// state, table in global memory -- resident in L2 up to a few MiB, 16-bit entries up to 65535 state sets and 32-bit entries beyond -- and
// only the byte classes in LDS; the walk is resume_piece_big.  A string of sp.split_min bytes or more is handed to the kernels below
// (split_take); with sp.hdr == NULL (quiet workspace) the lane walks it and split_take reports it; sp.split_min == 0 (MFA_DFA_SPEC=0,
// MFA_DFA_SPLIT=0, n >= 2^31): the queue is off and every string is walked here.  RESUME: dfa_split.h has the policy.
template <bool REV, class T, bool RESUME>
__global__ void __launch_bounds__(256)
dfa_spec_big_kernel(const T* __restrict__ trans, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ byte_class, uint32_t n_states,
                    uint32_t n_classes, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                    uint32_t* __restrict__ states, uint8_t* __restrict__ results, const SplitArgs sp) {
    __shared__ uint8_t s_class[256];
    s_class[threadIdx.x] = byte_class[threadIdx.x];
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < n; sid += stride) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        const StateEntry r = state_begin<RESUME>(states, n_states, sid, e - b, sp);
        if (r.taken) continue;                                        // queued: word and result are dfa_spec_resolve_kernel's
        state_end<RESUME>(states, results, accept_tab, sid, r.walks ? resume_piece_big<REV, T>(trans, s_class, n_classes, bytes, b, e, r.st) : r.st);
    }
}

// ---- chunks (spec_chunk: dfa_split.h) ------------------------------------------------------------------
// Round 0, one lane per chunk: chunk 0 of a string from its true state (1, or its word of `states`), every other from a guess.
template <bool REV, class T>
__global__ void __launch_bounds__(256)
dfa_spec_walk_kernel(const T* __restrict__ trans, const uint8_t* __restrict__ byte_class, uint32_t n_classes, const uint8_t* __restrict__ bytes,
                     const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue,
                     uint32_t* __restrict__ start_used, uint32_t* __restrict__ end0, const uint32_t* __restrict__ states, uint32_t home, uint32_t lookback) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if ((uint64_t)blockIdx.x * blockDim.x >= n_chunks) return;      // (no long string: every block leaves here)
    __shared__ uint8_t s_class[256];
    s_class[threadIdx.x] = byte_class[threadIdx.x];
    __syncthreads();
    const uint32_t chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += stride) {
        const SpecChunk ch = spec_chunk<REV>(queue, n_q, offsets, chunk, (uint32_t)c);
        uint32_t st;
        if (ch.k == 0u) st = states != nullptr ? states[queue[ch.q].sid] : 1u;
        else {
            uint64_t from, to;
            spec_lookback_range<REV>(ch.b, ch.e, ch.lo, ch.hi, lookback, &from, &to);
            st = spec_guess<REV, T>(trans, s_class, n_classes, bytes, from, to, home);
        }
        start_used[c] = st;
        end0[c] = resume_piece_big<REV, T>(trans, s_class, n_classes, bytes, ch.lo, ch.hi, st);
    }
}

// One repair round, one lane per chunk: walked again from what its predecessor ended in, if that is not what it was walked from.
template <bool REV, class T>
__global__ void __launch_bounds__(256)
dfa_spec_repair_kernel(const T* __restrict__ trans, const uint8_t* __restrict__ byte_class, uint32_t n_classes, const uint8_t* __restrict__ bytes,
                       const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue,
                       uint32_t* __restrict__ start_used, const uint32_t* __restrict__ end_prev, uint32_t* __restrict__ end_next) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if ((uint64_t)blockIdx.x * blockDim.x >= n_chunks) return;
    __shared__ uint8_t s_class[256];
    s_class[threadIdx.x] = byte_class[threadIdx.x];
    __syncthreads();
    const uint32_t chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += stride) {
        const SpecChunk ch = spec_chunk<REV>(queue, n_q, offsets, chunk, (uint32_t)c);
        const uint32_t used = start_used[c], prev = ch.k != 0u ? end_prev[c - 1u] : used;
        if (!spec_needs_rewalk(ch.k, used, prev)) { end_next[c] = end_prev[c]; continue; }
        start_used[c] = prev;
        end_next[c] = resume_piece_big<REV, T>(trans, s_class, n_classes, bytes, ch.lo, ch.hi, prev);
        atomicAdd(&hdr[SPEC_H_REWALKED], 1u);
    }
}

// ---- resolve -----------------------------------------------------------------------------------------
// One lane per queued string: the state it reaches from st over its records, walking the rest serially where they do not join up.
template <bool REV, class T>
__device__ __forceinline__ uint32_t spec_resolve_string(const T* __restrict__ trans, const uint8_t* s_class, uint32_t n_classes, const uint8_t* __restrict__ bytes,
                                                        const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue,
                                                        uint32_t q, const uint32_t* __restrict__ start_used, const uint32_t* __restrict__ end_fin, uint32_t st) {
    const uint32_t first = queue[q].first, nc = queue[q].nc;
    const uint32_t c = spec_resolve(start_used + first, end_fin + first, nc, &st);
    if (c < nc) {
        const uint64_t sid = queue[q].sid, b = offsets[sid], e = offsets[sid + 1u];
        uint64_t lo, hi, from, to;
        split_chunk_range<REV>(b, e, hdr[SPLIT_H_CHUNK], nc, c, &lo, &hi);
        spec_rest_range<REV>(b, e, lo, hi, &from, &to);
        st = resume_piece_big<REV, T>(trans, s_class, n_classes, bytes, from, to, st);
        atomicAdd(&hdr[SPEC_H_SERIAL_STRINGS], 1u);
        atomicAdd(reinterpret_cast<unsigned long long*>(&hdr[SPEC_H_SERIAL_BYTES]), (unsigned long long)(to - from));
    }
    return st;
}

// RESUME (mfa_match_batch_resume): from the string's word (a state that walks: the main kernel queues no other), which gets the state reached
template <bool REV, class T, bool RESUME>
__global__ void __launch_bounds__(256)
dfa_spec_resolve_kernel(const T* __restrict__ trans, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ byte_class, uint32_t n_classes,
                        const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue,
                        const uint32_t* __restrict__ start_used, const uint32_t* __restrict__ end_fin, uint32_t* __restrict__ states,
                        uint8_t* __restrict__ results) {
    const uint32_t n_q = hdr[SPLIT_H_STRINGS];
    if ((uint64_t)blockIdx.x * blockDim.x >= n_q) return;
    __shared__ uint8_t s_class[256];
    s_class[threadIdx.x] = byte_class[threadIdx.x];
    __syncthreads();
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n_q; q += gridDim.x * blockDim.x) {
        const uint64_t sid = queue[q].sid;
        const uint32_t st = spec_resolve_string<REV, T>(trans, s_class, n_classes, bytes, offsets, hdr, queue, q, start_used, end_fin,
                                                        state_of_queued<RESUME>(states, sid));
        state_end<RESUME>(states, results, accept_tab, sid, st);
    }
}

// ---- host side ---------------------------------------------------------------------------------------
bool spec_applies(const HostImage& img) {
    // the tables launch_dfa_walk and launch_dfa_resume give the L2 kernels: beyond 16-bit pre-multiplied states, 255 state sets and more
    // (dfa_split.hip has those up to 127; 128 to 254 are outside both, as they are outside mfa_match_batch)
    return img.h.kind == MFA_KIND_NFA && (size_t)img.dfa_states * kDfaRow > 0xffffu;
}

static_assert(kSplitSchemeL2.per_chunk == 3 * sizeof(uint32_t) && kSplitSchemeL2.rounds == kSpecRounds && kSplitSchemeL2.lookback == kSpecLookback &&
              kSplitRoundsMax == kSpecRoundsMax, "memless_plan.h: the L2 scheme");

template <bool REV, class T>
static int spec_main_go(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                        uint8_t* d_results, hipStream_t s, uint32_t* d_states, unsigned blocks) {
    auto kern = d_states != nullptr ? dfa_spec_big_kernel<REV, T, true> : dfa_spec_big_kernel<REV, T, false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, (const T*)ds.d_dfa_trans, ds.d_dfa_accept, ds.d_byte_class, img.dfa_states, img.n_classes,
                       d_bytes, d_offsets, n, d_states, d_results, sl.args);
    return MFA_OK;                                                    // (memless_bracket asks for the launch's error)
}

// (A workspace starts QUIET here, kSplitSchemeL2: traffic of short strings never pays for the seven launches below, and the first batch with
// long strings on a workspace is walked whole, as it was before this path existed.  MFA_DFA_SPLIT=2 launches them from the first call on.)
template <bool REV, class T>
static int spec_tail_go(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                        uint8_t* d_results, hipStream_t s, uint32_t* d_states) {
    const T* trans = (const T*)ds.d_dfa_trans;
    const SplitEntry* queue = sl.args.queue;
    // one lane per chunk, the chunk count is the plan's: a grid for every chunk the arena holds, blocks beyond the count leave at once
    const unsigned blocks = persistent_grid(sl.map_cap, 256, (uint64_t)ds.n_cus, 8), q_blocks = (sl.args.qcap + 255u) / 256u;
    return guess_tail<uint32_t>(sl, 1, d_offsets, s,
        [&](uint32_t* start_used, uint32_t* end0) {
            hipLaunchKernelGGL((dfa_spec_walk_kernel<REV, T>), dim3(blocks), dim3(256), 0, s, trans, ds.d_byte_class, img.n_classes, d_bytes, d_offsets,
                               (const uint32_t*)sl.args.hdr, queue, start_used, end0, (const uint32_t*)d_states, img.dfa_home, sl.spec_lookback);
            return MFA_OK;
        },
        [&](uint32_t* start_used, const uint32_t* end_prev, uint32_t* end_next) {
            hipLaunchKernelGGL((dfa_spec_repair_kernel<REV, T>), dim3(blocks), dim3(256), 0, s, trans, ds.d_byte_class, img.n_classes, d_bytes, d_offsets,
                               sl.args.hdr, queue, start_used, end_prev, end_next);
            return MFA_OK;
        },
        [&](const uint32_t* start_used, const uint32_t* end_fin) {
            auto resolve = d_states != nullptr ? dfa_spec_resolve_kernel<REV, T, true> : dfa_spec_resolve_kernel<REV, T, false>;
            hipLaunchKernelGGL(resolve, dim3(q_blocks), dim3(256), 0, s, trans, ds.d_dfa_accept, ds.d_byte_class, img.n_classes, d_bytes, d_offsets, sl.args.hdr,
                               queue, start_used, end_fin, d_states, d_results);
            return MFA_OK;
        });
}

#define MFA_SPEC_DISPATCH(FN, ...)                                                                                  \
    (img.h.is_reversed ? (img.dfa_states <= 0xffffu ? FN<true, uint16_t>(__VA_ARGS__) : FN<true, uint32_t>(__VA_ARGS__))  \
                       : (img.dfa_states <= 0xffffu ? FN<false, uint16_t>(__VA_ARGS__) : FN<false, uint32_t>(__VA_ARGS__)))

int spec_main(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
              uint8_t* d_results, void* stream, uint32_t* d_states, unsigned blocks) {
    return MFA_SPEC_DISPATCH(spec_main_go, img, ds, sl, d_bytes, d_offsets, n, d_results, (hipStream_t)stream, d_states, blocks);
}

int spec_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
              uint8_t* d_results, void* stream, uint32_t* d_states) {
    if (sl.args.hdr == nullptr) return MFA_OK;
    return MFA_SPEC_DISPATCH(spec_tail_go, img, ds, sl, d_bytes, d_offsets, d_results, (hipStream_t)stream, d_states);
}

#undef MFA_SPEC_DISPATCH

}  // namespace mfa
