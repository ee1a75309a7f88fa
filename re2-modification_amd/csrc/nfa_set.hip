// The set walk of memory-less automata, written for gfx950 (MI355X): Automata::match (reference automata.cpp:177-210) for an automaton
// whose determinisation passes the tabulation limit (image_host.cpp: nfa_image_build).  One input string per lane; the lane's state is
// the set of live nodes, W words of bit mask in registers, and every byte runs the reference's step on it (nfa_set_core.h).
//   LDS: the stacks of the 256 lanes, [slot][lane] -- a slot's 256 words are consecutive, so the lanes of a wave that push or pop at the
//   same depth hit 64 different banks, and the stack pointer stays a register (a private array indexed by it would live in scratch
//   memory) -- and behind them the automaton's tables when both fit 64 KiB; else the tables are read through L2.
//   Input: 16 bytes per lane per load, in aligned blocks that hold a byte of the string: nothing beyond offsets[n] rounded up to 16.
//   Grid: persistent, capped by what the CUs keep resident (lds_blocks_per_cu), strings dealt out by lane number.
// Supported: up to 256 nodes (W = 1, 2, 4, 8 words for up to 32, 64, 128, 256), 255 byte classes, epsilon chains of up to 49 nodes.
// A long string is cut across the whole GPU by nfa_set_split.hip, behind the main kernel of this file.
#include <hip/hip_runtime.h>

#include "nfa_set.h"

namespace mfa {

// A string of sp.split_min bytes or more (and within the limit) is handed to nfa_set_split.hip (split_take: the one hand-over, no string
// is lost); sp.split_min == 0: the queue is off and every string is walked here, as before that path existed.
template <bool REV, int W>
__global__ void __launch_bounds__(256)
nfa_set_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t stack_words, uint32_t tables_in_lds,
               const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n, uint8_t* __restrict__ results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;                               // slot s of this lane: stack[s * 256]
    const NfaSetView t = nfa_set_view(tables, set_tables_base(lds, tables, table_words, stack_words, tables_in_lds));
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t sid = (uint64_t)blockIdx.x * 256u + threadIdx.x; sid < n; sid += stride) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        if (sp.split_min != 0u && e - b >= sp.split_min && e - b <= kSetMaxString && split_take(sp, sid)) continue;      // queued: the result is nfa_set_resolve_kernel's
        results[sid] = nfa_set_walk<REV, W>(t, stack, 256u, bytes, b, e);
    }
}

// The same walk for strings in pieces (mfa_match_batch_resume_set): the lane's set comes from its record of `states` (twelve words, read as
// three aligned 16-byte loads) instead of {start}, and goes back into it behind the piece (three 16-byte stores); `results` may be NULL.
// Same grid, same LDS layout, same residency cap.  Record and rule: nfa_set_core.h.  Only a piece that enters with a live set is queued:
// dead, invalid and over-long records are answered here, and a queued piece's record is left as it came for the kernels behind this one.
template <bool REV, int W>
__global__ void __launch_bounds__(256)
nfa_set_resume_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t stack_words, uint32_t tables_in_lds,
                      const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n, uint4* __restrict__ states,
                      uint8_t* __restrict__ results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const NfaSetView t = nfa_set_view(tables, set_tables_base(lds, tables, table_words, stack_words, tables_in_lds));
    const uint32_t n_nodes = tables[SET_H_NODES];
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t sid = (uint64_t)blockIdx.x * 256u + threadIdx.x; sid < n; sid += stride) {
        uint4* rec = states + sid * 3u;
        uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        uint32_t cur[W];
        const uint32_t tag = nfa_set_state_decode<W>(t, n_nodes, q0, q1, q2, e - b, cur);
        if (sp.split_min != 0u && e - b >= sp.split_min && tag == kSetStateLive) {
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < W; k++) any |= cur[k];
            if (any != 0u && split_take(sp, sid)) continue;
        }
        const uint8_t r = nfa_set_resume_entered<REV, W>(t, stack, 256u, bytes, b, e, tag, cur, q0, q1, q2);
        rec[0] = q0; rec[1] = q1; rec[2] = q2;
        if (results) results[sid] = r;
    }
}

// d_states != nullptr: nfa_set_resume_kernel on these records; else nfa_set_kernel.  Behind either, the kernels of nfa_set_split.hip for the
// strings it queued; ev_start and ev_stop enclose all of it.
template <bool REV, int W>
static int launch_set(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint32_t* d_states, uint8_t* d_results, hipStream_t s) {
    const SetLds l = set_lds_of(img);
    const bool resume = d_states != nullptr;
    const MemlessKnobs kn = memless_knobs();
    const EnginePlan p = plan_memless_engine(set_image(img), resume, kn, n, (uint64_t)ds.n_cus);
    const uint32_t* tables = (const uint32_t*)ds.d_set_tables;
    const int rc = resume ? set_allow_lds<nfa_set_resume_kernel<REV, W>>(ds.device) : set_allow_lds<nfa_set_kernel<REV, W>>(ds.device);
    if (rc != MFA_OK) return rc;
    return memless_bracket(kSplitSchemeSet, kn, cx, n, s,
        [&](const SplitLaunch& sl) {
            if (resume)
                hipLaunchKernelGGL((nfa_set_resume_kernel<REV, W>), dim3(p.grid), dim3(256), p.lds, s, tables, l.words, l.stack_words, l.in_lds, d_bytes, d_offsets, n,
                                   reinterpret_cast<uint4*>(d_states), d_results, sl.args);
            else
                hipLaunchKernelGGL((nfa_set_kernel<REV, W>), dim3(p.grid), dim3(256), p.lds, s, tables, l.words, l.stack_words, l.in_lds, d_bytes, d_offsets, n, d_results, sl.args);
            return MFA_OK;
        },
        [&](const SplitLaunch& sl) { return set_split_tail(img, ds, sl, d_bytes, d_offsets, d_results, s, d_states); });
}

int launch_nfa_set(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                   uint8_t* d_results, void* stream) {
    if (!img.set_walk || !ds.d_set_tables || img.set_tables.size() < SET_H_SIZE) return MFA_ERR_UNSUPPORTED;
    MFA_SET_DISPATCH(launch_set, img, ds, cx, d_bytes, d_offsets, n, nullptr, d_results, (hipStream_t)stream);
}

int launch_nfa_set_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                          uint32_t* d_states, uint8_t* d_results, void* stream) {
    if (!img.set_walk || !ds.d_set_tables || img.set_tables.size() < SET_H_SIZE) return MFA_ERR_UNSUPPORTED;
    MFA_SET_DISPATCH(launch_set, img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, (hipStream_t)stream);
}

}  // namespace mfa
