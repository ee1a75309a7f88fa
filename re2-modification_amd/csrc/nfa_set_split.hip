// Long strings of set-walk images, cut across the whole GPU (gfx950).  The kernels of nfa_set.hip walk one string per lane at 10^5 to 10^6
// bytes per second, so one string of a megabyte holds a call for seconds while the rest of the device idles.  Here a string with
// len >= split_min is cut into chunks and every chunk is walked from ONE set -- a guess -- by a lane of its own; wrong guesses are
// repaired a bounded number of times, then resolved exactly (nfa_set_split_core.h has the scheme and is checked on the CPU: tests/emul).
// Composing per-chunk maps from single nodes is not available: the step's visited mask is shared by the nodes of a set.
// Queue, plan, chunk geometry and the shared knobs are dfa_split.hip's:
//   memset(header) -> nfa_set_kernel / nfa_set_resume_kernel (queue long strings: split_take) -> dfa_plan_kernel -> nfa_set_chunk_kernel
//     -> MFA_SET_SPLIT_ROUNDS x nfa_set_repair_kernel -> nfa_set_resolve_kernel
// all on the caller's stream, with no read-back; the number of launches is fixed when the call is enqueued.  Successive launches on one
// stream are the only ordering: no kernel here spins or waits for another workgroup, every loop is bounded by a chunk's or a string's bytes.
// Records: per chunk start_used and TWO ends, each a mfa_set_state of three 16-byte quarters moved by aligned 16-byte loads and stores.
// Repair round r reads the ends round r - 1 left in end[(r - 1) & 1] and writes every chunk's end to end[r & 1] (walked again, or copied),
// so no lane reads a word another lane of the same launch writes; start_used[c] is read and written by the lane of chunk c alone.
// LDS: the layout of nfa_set_kernel (nfa_set.h), the same residency cap.  The workspace is not quiet: the tail is launched from the first
// call on -- one long string walked whole costs seconds here, not milliseconds.
#include <hip/hip_runtime.h>

#include "nfa_set.h"
#include "nfa_set_split_core.h"

namespace mfa {

// Round 0, one lane per chunk: chunk 0 of a string from its true set ({start}, or its record of `states`), every other from a guess.
template <bool REV, int W>
__global__ void __launch_bounds__(256)
nfa_set_chunk_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t stack_words, uint32_t tables_in_lds,
                     const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ hdr,
                     const SplitEntry* __restrict__ queue, uint4* __restrict__ start_used, uint4* __restrict__ end0, const uint4* __restrict__ states,
                     const SetHome home, uint32_t lookback) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if ((uint64_t)blockIdx.x * 256u >= n_chunks) return;            // (no long string: every block leaves here, before it touches LDS)
    extern __shared__ uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const NfaSetView t = nfa_set_view(tables, set_tables_base(lds, tables, table_words, stack_words, tables_in_lds));
    const uint32_t n_nodes = tables[SET_H_NODES], chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < n_chunks; c += stride) {
        const SpecChunk ch = spec_chunk<REV>(queue, n_q, offsets, chunk, (uint32_t)c);
        SetRec first;
        first.q0 = first.q1 = first.q2 = make_uint4(0u, 0u, 0u, 0u);                      // kSetStateStart: {start}
        if (ch.k == 0u && states != nullptr) first = set_rec_load(states, queue[ch.q].sid);
        set_spec_round0<REV, W>(t, n_nodes, stack, 256u, bytes, ch.b, ch.e, ch.lo, ch.hi, ch.k, first, home, lookback, start_used, end0, c);
    }
}

// One repair round, one lane per chunk: walked again from what its predecessor ended in, if that is not what it was walked from.
template <bool REV, int W>
__global__ void __launch_bounds__(256)
nfa_set_repair_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t stack_words, uint32_t tables_in_lds,
                      const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr,
                      const SplitEntry* __restrict__ queue, uint4* __restrict__ start_used, const uint4* __restrict__ end_prev, uint4* __restrict__ end_next) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if ((uint64_t)blockIdx.x * 256u >= n_chunks) return;
    extern __shared__ uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const NfaSetView t = nfa_set_view(tables, set_tables_base(lds, tables, table_words, stack_words, tables_in_lds));
    const uint32_t n_nodes = tables[SET_H_NODES], chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < n_chunks; c += stride) {
        const SpecChunk ch = spec_chunk<REV>(queue, n_q, offsets, chunk, (uint32_t)c);
        if (set_spec_repair<REV, W>(t, n_nodes, stack, 256u, bytes, ch.lo, ch.hi, ch.k, start_used, end_prev, end_next, c)) atomicAdd(&hdr[SPEC_H_REWALKED], 1u);
    }
}

// One lane per queued string: the set it reaches from its true set over its records, walking the rest serially where they do not join up.
// RESUME (mfa_match_batch_resume_set): from the string's record (live: the main kernel queues no other), which gets the set reached;
// results may then be NULL.
template <bool REV, int W, bool RESUME>
__global__ void __launch_bounds__(256)
nfa_set_resolve_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t stack_words, uint32_t tables_in_lds,
                       const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr,
                       const SplitEntry* __restrict__ queue, const uint4* __restrict__ start_used, const uint4* __restrict__ end_fin, uint4* __restrict__ states,
                       uint8_t* __restrict__ results) {
    const uint32_t n_q = hdr[SPLIT_H_STRINGS];
    if ((uint64_t)blockIdx.x * 256u >= n_q) return;
    extern __shared__ uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const NfaSetView t = nfa_set_view(tables, set_tables_base(lds, tables, table_words, stack_words, tables_in_lds));
    const uint32_t n_nodes = tables[SET_H_NODES], chunk = hdr[SPLIT_H_CHUNK];
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n_q; q += gridDim.x * 256u) {
        const uint64_t sid = queue[q].sid, b = offsets[sid], e = offsets[sid + 1u];
        const uint32_t first_chunk = queue[q].first, nc = queue[q].nc;
        SetRec first;
        first.q0 = first.q1 = first.q2 = make_uint4(0u, 0u, 0u, 0u);
        if (RESUME) first = set_rec_load(states, sid);
        uint64_t serial;
        const SetRec fin = set_spec_resolve_string<REV, W>(t, n_nodes, stack, 256u, bytes, b, e, chunk, nc, start_used + (uint64_t)first_chunk * kSetRecQuarters,
                                                           end_fin + (uint64_t)first_chunk * kSetRecQuarters, first, &serial);
        if (serial != 0u) {
            atomicAdd(&hdr[SPEC_H_SERIAL_STRINGS], 1u);
            atomicAdd(reinterpret_cast<unsigned long long*>(&hdr[SPEC_H_SERIAL_BYTES]), (unsigned long long)serial);
        }
        if (RESUME) set_rec_store(states, sid, fin);
        if (!RESUME || results != nullptr) results[sid] = set_rec_result<W>(t, n_nodes, fin);
    }
}

// ---- host side ---------------------------------------------------------------------------------------
static_assert(kSplitSchemeSet.per_chunk == 3u * kSetRecQuarters * sizeof(uint4) && kSplitSchemeSet.chunk_min == kSetSplitChunkMin &&
              kSplitSchemeSet.rounds == kSetSplitRounds && kSplitSchemeSet.lookback == kSetSplitLookback, "memless_plan.h: the lane scheme");

template <bool REV, int W>
static int set_split_tail_go(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                             uint8_t* d_results, hipStream_t s, uint32_t* d_states) {
    const SetLds l = set_lds_of(img);
    const uint32_t* tables = (const uint32_t*)ds.d_set_tables;
    const SplitEntry* queue = sl.args.queue;
    SetHome home;
    for (int k = 0; k < kSetStateNodeWords; k++) home.w[k] = img.set_home[k];
    // one lane per chunk, the chunk count is the plan's: a grid for every chunk the arena holds, capped by what the CUs keep resident;
    // blocks beyond the count leave at once
    const uint64_t per_cu = lds_blocks_per_cu(l.bytes);
    const unsigned blocks = persistent_grid(sl.map_cap, 256, (uint64_t)ds.n_cus, per_cu), q_blocks = persistent_grid(sl.args.qcap, 256, (uint64_t)ds.n_cus, per_cu);
    return guess_tail<uint4>(sl, kSetRecQuarters, d_offsets, s,
        [&](uint4* start_used, uint4* end0) {
            int rc = set_allow_lds<nfa_set_chunk_kernel<REV, W>>(ds.device);
            if (rc == MFA_OK) rc = set_allow_lds<nfa_set_repair_kernel<REV, W>>(ds.device);
            if (rc != MFA_OK) return rc;
            hipLaunchKernelGGL((nfa_set_chunk_kernel<REV, W>), dim3(blocks), dim3(256), l.bytes, s, tables, l.words, l.stack_words, l.in_lds, d_bytes, d_offsets,
                               (const uint32_t*)sl.args.hdr, queue, start_used, end0, reinterpret_cast<const uint4*>(d_states), home, sl.spec_lookback);
            return MFA_OK;
        },
        [&](uint4* start_used, const uint4* end_prev, uint4* end_next) {
            hipLaunchKernelGGL((nfa_set_repair_kernel<REV, W>), dim3(blocks), dim3(256), l.bytes, s, tables, l.words, l.stack_words, l.in_lds, d_bytes, d_offsets,
                               sl.args.hdr, queue, start_used, end_prev, end_next);
            return MFA_OK;
        },
        [&](const uint4* start_used, const uint4* end_fin) {
            const int rc = d_states != nullptr ? set_allow_lds<nfa_set_resolve_kernel<REV, W, true>>(ds.device) : set_allow_lds<nfa_set_resolve_kernel<REV, W, false>>(ds.device);
            if (rc != MFA_OK) return rc;
            hipLaunchKernelGGL((d_states != nullptr ? nfa_set_resolve_kernel<REV, W, true> : nfa_set_resolve_kernel<REV, W, false>), dim3(q_blocks), dim3(256), l.bytes, s,
                               tables, l.words, l.stack_words, l.in_lds, d_bytes, d_offsets, sl.args.hdr, queue, start_used, end_fin, reinterpret_cast<uint4*>(d_states), d_results);
            return MFA_OK;
        });
}

int set_split_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                   uint8_t* d_results, void* stream, uint32_t* d_states) {
    if (sl.args.hdr == nullptr) return MFA_OK;
    MFA_SET_DISPATCH(set_split_tail_go, img, ds, sl, d_bytes, d_offsets, d_results, (hipStream_t)stream, d_states);
}

}  // namespace mfa
