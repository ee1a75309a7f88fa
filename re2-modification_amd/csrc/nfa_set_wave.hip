// The wave-cooperative set walk of memory-less automata, written for gfx950 (MI355X): Automata::match (reference automata.cpp:177-210)
// for a set-walk image of more nodes than a lane holds as a mask (257 to 2048), or for any set-walk image under MFA_SET_WAVE=1.  ONE
// input string per WAVE: the node set lies across the lanes, lane l the nodes 32 l .. 32 l + 31, and everything else -- node, item
// position, stack pointer, byte, class -- is wave-uniform (nfa_set_wave_core.h has the rule and the primitives).
//   LDS: the stacks of the four waves of a block, `depth` slots of 4 bytes each (the image's longest epsilon chain, at most its node
//   count: 32 KiB at the most), and behind them the automaton's tables when both fit 64 KiB; else the tables are read through L2.
//   Input: up to 64 aligned 16-byte blocks per wave and round, lane l block l; only blocks that hold a byte of the string.
//   Grid: persistent, capped by what the CUs keep resident (lds_blocks_per_cu), strings dealt out by wave number.
// Strings in pieces (mfa_match_batch_resume_set_wide): nfa_set_wave_resume_kernel, the same grid and LDS, a record of 68 words per
// string (mfa_set_state_wide) read before the piece and written behind it.  mfa_match_batch_resume_set (the 48-byte record) keeps
// refusing the image (capi.hip).  The lane kernel (nfa_set.hip) stays the default for every image it can walk.
// A long string, or a long piece that enters with a live set, is cut across the whole GPU by nfa_set_wave_split.hip, behind the main
// kernel of this file: the wave that holds it hands it over (split_take, dfa_split.h: the one hand-over, no string is lost).
#include <hip/hip_runtime.h>

#include "nfa_set_wave.h"
#include "nfa_set_wave_split_core.h"

namespace mfa {

// What a wave does with a string it may hand to nfa_set_wave_split.hip: lane 0 asks for the queue slot, the answer is made wave-uniform.
// true: the string is queued, its result (and record) are nfa_set_wave_resolve_kernel's.
static __device__ __forceinline__ bool wave_split_take(const SplitArgs& sp, uint64_t sid) {
    uint32_t taken = 0u;
    if (WaveDev::lane() == 0u) taken = split_take(sp, sid) ? 1u : 0u;
    return WaveDev::uni(taken) != 0u;
}

// IN_LDS: the tables' sections are read from their copy behind the stacks (LDS), else from global memory; a template parameter, so that
// the compiler knows the address space of every table read.  sp.split_min == 0: the queue is off and every string is walked here, as
// before that path existed.
template <bool REV, bool IN_LDS>
__global__ void __launch_bounds__(256)
nfa_set_wave_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t depth, const uint8_t* __restrict__ bytes,
                    const uint64_t* __restrict__ offsets, uint64_t n, uint8_t* __restrict__ results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    const uint32_t wave = WaveDev::uni(threadIdx.x >> 6);
    uint32_t* stack = lds + wave * depth;                              // slot s of this wave: stack[s]
    const NfaSetView t = nfa_set_view(tables, wave_tables_base<IN_LDS>(lds, tables, table_words, depth));
    const uint32_t W = tables[SET_H_WORDS];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t sid = (uint64_t)blockIdx.x * 4u + wave; sid < n; sid += n_waves) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        if (sp.split_min != 0u && e - b >= sp.split_min && e - b <= kSetMaxString && wave_split_take(sp, sid)) continue;      // ({start} is never empty)
        const uint8_t r = nfa_wave_walk<REV, WaveDev>(t, W, stack, bytes, b, e);
        if (WaveDev::lane() == 0u) results[sid] = r;
    }
}

// The same walk for strings in pieces: the wave's set comes from its string's record of `states` (kWaveStateWords words, 16-byte
// aligned: a tag quarter, then lane l's word) and goes back there behind the piece (nfa_set_wave_core.h: nfa_wave_resume_piece).  A
// record is read and written by the one wave that has its string.  results may be NULL.  Only a piece whose record decodes to a live,
// non-empty set is queued: dead, invalid and over-long records are answered here, and a queued piece's record is left as it came.
template <bool REV, bool IN_LDS>
__global__ void __launch_bounds__(256)
nfa_set_wave_resume_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t depth, const uint8_t* __restrict__ bytes,
                           const uint64_t* __restrict__ offsets, uint64_t n, uint32_t* states, uint8_t* results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    const uint32_t wave = WaveDev::uni(threadIdx.x >> 6);
    uint32_t* stack = lds + wave * depth;
    const NfaSetView t = nfa_set_view(tables, wave_tables_base<IN_LDS>(lds, tables, table_words, depth));
    const uint32_t W = tables[SET_H_WORDS], n_nodes = tables[SET_H_NODES];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t sid = (uint64_t)blockIdx.x * 4u + wave; sid < n; sid += n_waves) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        uint32_t* rec = states + sid * kWaveStateWords;
        WaveDev::Reg cur;
        const uint32_t tag = nfa_wave_state_decode<WaveDev>(t, n_nodes, rec, e - b, cur);
        if (sp.split_min != 0u && e - b >= sp.split_min && tag == kSetStateLive && WaveDev::any(cur) && wave_split_take(sp, sid)) continue;
        const uint8_t r = wave_resume_entered<REV, WaveDev>(t, W, stack, bytes, b, e, tag, cur, rec);      // (nfa_wave_resume_piece behind its decode)
        if (results && WaveDev::lane() == 0u) results[sid] = r;
    }
}

// d_states != nullptr: nfa_set_wave_resume_kernel on these records; else nfa_set_wave_kernel.  Behind either, the kernels of
// nfa_set_wave_split.hip for the strings it queued; ev_start and ev_stop enclose all of it.
template <bool REV, bool IN_LDS>
static int launch_wave(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t* d_states,
                       uint8_t* d_results, hipStream_t s) {
    const bool resume = d_states != nullptr;
    const MemlessKnobs kn = memless_knobs();
    const EnginePlan p = plan_memless_engine(set_image(img), resume, kn, n, (uint64_t)ds.n_cus);
    const uint32_t* tables = (const uint32_t*)ds.d_set_tables;
    const uint32_t words = (uint32_t)img.set_tables.size(), depth = img.set_tables[SET_H_DEPTH];
    const int rc = resume ? set_allow_lds<nfa_set_wave_resume_kernel<REV, IN_LDS>>(ds.device) : set_allow_lds<nfa_set_wave_kernel<REV, IN_LDS>>(ds.device);
    if (rc != MFA_OK) return rc;
    return memless_bracket(kSplitSchemeWave, kn, cx, n, s,
        [&](const SplitLaunch& sl) {
            if (resume)
                hipLaunchKernelGGL((nfa_set_wave_resume_kernel<REV, IN_LDS>), dim3(p.grid), dim3(256), p.lds, s, tables, words, depth, d_bytes, d_offsets, n, d_states, d_results, sl.args);
            else
                hipLaunchKernelGGL((nfa_set_wave_kernel<REV, IN_LDS>), dim3(p.grid), dim3(256), p.lds, s, tables, words, depth, d_bytes, d_offsets, n, d_results, sl.args);
            return MFA_OK;
        },
        [&](const SplitLaunch& sl) { return set_wave_split_tail(img, ds, sl, d_bytes, d_offsets, d_results, s, d_states); });
}

int launch_nfa_set_wave(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                        uint8_t* d_results, void* stream) {
    if (!wave_tables_ok(img, ds)) return MFA_ERR_UNSUPPORTED;
    return MFA_WAVE_DISPATCH(launch_wave, set_lds_of(img).in_lds != 0u, img, ds, cx, d_bytes, d_offsets, n, nullptr, d_results, (hipStream_t)stream);
}

int launch_nfa_set_wave_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                               uint32_t* d_states, uint8_t* d_results, void* stream) {
    if (!wave_tables_ok(img, ds)) return MFA_ERR_UNSUPPORTED;
    return MFA_WAVE_DISPATCH(launch_wave, set_lds_of(img).in_lds != 0u, img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, (hipStream_t)stream);
}

}  // namespace mfa
