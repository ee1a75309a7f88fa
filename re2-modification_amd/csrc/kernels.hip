// HIP kernels for memory-less automata, written for gfx950 (MI355X): Automata::match (reference automata.cpp:177-210) on the
// tabulated step function (image_host.cpp: tabulate_nfa).  One input string per lane, 64 strings per wavefront.
// (Memory automata: regions.hip + walk.hip, or the kernels jit_gen.cpp generates.)
#include <hip/hip_runtime.h>

#include <cstring>

#include "mfa_internal.h"
#ifndef MFA_DFA_LINE
#define MFA_DFA_LINE 128
#endif
#include "device_common.h"

namespace mfa {

// ---- table walk for memory-less automata -------------------------------------------------------
// One string per lane.  LDS holds one fused table: next[state][byte] (16-bit entries, the state
// pre-multiplied by the row stride), so a step is: extract byte, OR it into the state word, one
// ds_read_u16.  Rows are padded by one dword so that equal bytes in different states fall into
// different banks.  State 0 is the empty set: absorbing and rejecting, the reference's early
// `break` (automata.cpp:186-188,196-198).  Input is read 16 bytes per lane per load.
// (kDfaRow, the row stride: 16-bit entries per state row, 256 + 2 pad -- dfa_split_core.h)
// sp: strings of sp.split_min bytes and more go to the split path (dfa_split.h: split_take); sp.split_min == 0: none does.
// RESUME: where a string's state comes from and where it goes (dfa_split.h has the policy; mfa_match_batch: false, mfa_match_batch_resume: true).
// (Tables beyond 16-bit pre-multiplied states stay in global memory: dfa_spec.hip has their kernel.)

// One lane: the state reached from st (= state * kDfaRow) over [b, e), one 16-byte block per round.
template <bool REV>
__device__ __forceinline__ uint32_t dfa_walk_blocks(const uint16_t* s_next, const uint8_t* __restrict__ bytes, uint64_t b, uint64_t e, uint32_t st) {
    uint64_t p = REV ? e : b;                                         // forward: next byte to consume; reverse: one past it
    while ((REV ? p > b : p < e) && st != 0u) {
        const uint64_t blk = (REV ? p - 1u : p) & ~(uint64_t)15;
        const uint32_t lo = REV ? (b > blk ? (uint32_t)(b - blk) : 0u) : (uint32_t)(p - blk);
        const uint32_t hi = REV ? (uint32_t)(p - blk) : ((e - blk) < 16u ? (uint32_t)(e - blk) : 16u);
        st = split_step16<REV>(s_next, st, load16(bytes, blk), lo, hi);
        p = REV ? blk : blk + 16u;
    }
    return st;
}

// Two byte loops, chosen by the policy: the plain instantiation walks block by block (dfa_walk_blocks: 32 VGPRs, 8 waves per SIMD), the
// resume one with four blocks in flight (split_chunk_walk: twice the registers).  DESIGN.md section 4.7 has what was measured.
template <bool REV, bool RESUME>
__global__ void __launch_bounds__(256)
dfa_walk_kernel(const uint16_t* __restrict__ trans, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ byte_class,
                uint32_t n_states, uint32_t n_classes, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                uint32_t* __restrict__ states, uint8_t* __restrict__ results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    uint16_t* s_next = reinterpret_cast<uint16_t*>(lds);             // [n_states][kDfaRow], entry = next_state * kDfaRow
    dfa_fill_table(s_next, trans, byte_class, n_states, n_classes, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < n; sid += stride) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        const StateEntry r = state_begin<RESUME>(states, n_states, sid, e - b, sp);
        if (r.taken) continue;                                        // queued: dfa_fold_kernel writes word and result
        uint32_t st = r.st;
        if (r.walks) st = (RESUME ? split_chunk_walk<REV>(s_next, bytes, b, e, st * kDfaRow) : dfa_walk_blocks<REV>(s_next, bytes, b, e, st * kDfaRow)) / kDfaRow;
        state_end<RESUME>(states, results, accept_tab, sid, st);
    }
}

// ---- tiled table walk -----------------------------------------------------------------------------
// Same walk, input staged through LDS so that HBM is read in whole 128-byte lines (MFA_DFA_LINE; 64-byte
// rows double the resident waves but measured 3.7 against 4.55 TB/s; a second table stepping two bytes per
// dependent read -- n_states * classes^2 entries -- measured 4.4: the walk is not bound by that chain): a wave owns 64
// strings; each round, groups of 8 lanes fetch one 128-byte line of one string (8 x 16 B, a single
// contiguous segment per group), the 64 lines are written to a padded LDS tile, and every lane then
// reads its own string's line back with ds_read_b128.  The pad (144-byte row stride) keeps the 16
// lanes of a ds_read_b128 group on distinct banks.
//   PACKED: automata with <= 8 state sets and <= 7 literal byte classes keep the whole table in
//   SGPRs -- one 32-bit word per class, 4 bits per state -- so a step is a byte compare/select
//   (independent of the state) plus a 2-instruction dependent chain (shift, bit-field extract)
//   instead of an LDS round trip.
struct DfaPacked {
    uint32_t n_lit;          // literal classes
    uint32_t lit[7];         // their bytes
    uint32_t tab[8];         // tab[c]: nibble s = next state of s on class c; tab[n_lit] = every other byte
    uint32_t accept_mask;    // bit s = state s accepts
};

static constexpr uint32_t kLine = MFA_DFA_LINE;          // bytes of a string staged per round (one row of the tile)
static constexpr uint32_t kTileRow = kLine + 16;         // row stride in the LDS tile: the pad keeps ds_read_b128 groups on distinct banks
static constexpr uint32_t kLineLanes = kLine / 16;       // lanes that fetch one row, 16 bytes each
static constexpr uint32_t kFetches = kLineLanes;         // 64 / kLineLanes strings per load instruction -> kLineLanes instructions per round

template <bool REV, bool PACKED, int NLIT, bool RESUME>
__global__ void __launch_bounds__(256)
dfa_tiled_kernel(DfaPacked pk, const uint16_t* __restrict__ trans, const uint8_t* __restrict__ accept_tab,
                 const uint8_t* __restrict__ byte_class, uint32_t n_states, uint32_t n_classes,
                 const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                 uint32_t* __restrict__ states, uint8_t* __restrict__ results, const SplitArgs sp) {
    static_assert(!(PACKED && RESUME), "the SGPR-packed form carries no state across calls: such a call takes the LDS form");
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint8_t* tile = reinterpret_cast<uint8_t*>(lds) + wave * (64u * kTileRow);
    uint16_t* s_next = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(lds) + 4u * 64u * kTileRow);
    if (!PACKED) {
        dfa_fill_table(s_next, trans, byte_class, n_states, n_classes, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const uint64_t total16 = (offsets[n] + 15u) & ~(uint64_t)15;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    uint32_t lit[NLIT > 0 ? NLIT : 1], tabs[NLIT + 1];
#pragma unroll
    for (int c = 0; c < NLIT; c++) lit[c] = pk.lit[c];
#pragma unroll
    for (int c = 0; c <= NLIT; c++) tabs[c] = pk.tab[c];
    for (uint64_t w0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u; w0 < n; w0 += n_waves * 64u) {
        const uint64_t sid = w0 + lane;
        const bool have = sid < n;
        const uint64_t b = have ? offsets[sid] : 0;
        uint64_t e = have ? offsets[sid + 1] : 0;
        StateEntry r{RESUME ? 0u : 1u, !RESUME, false};
        if (have) r = state_begin<RESUME>(states, n_states, sid, e - b, sp);
        if (!r.walks || r.taken) e = b;           // dead, in error, or queued for the split path (word and result are dfa_fold_kernel's): empty here
        uint64_t p = REV ? e : b;                 // forward: next byte to consume; reverse: one past it
        uint32_t st = PACKED ? 1u : (r.walks ? r.st : 0u) * kDfaRow;
        bool active = have && (REV ? p > b : p < e);
        if (__any(active)) {                      // (a wave of empty strings has nothing to read)
        uint64_t line = (REV ? p - 1u : p) & ~(uint64_t)(kLine - 1u);
        // fetch: lane group g = lane>>3 serves strings g, g+8, ..., one 128-byte line each
        uint4 v[kFetches];
        auto fetch = [&](uint64_t ln, bool act) {
#pragma unroll
            for (int k = 0; k < (int)kFetches; k++) {
                const int src = k * (int)(64u / kLineLanes) + (int)(lane / kLineLanes);
                const uint32_t lo = __shfl((uint32_t)ln, src), hi = __shfl((uint32_t)(ln >> 32), src);
                const int a = __shfl((int)act, src);
                const uint64_t addr = (((uint64_t)hi << 32) | lo) + (lane % kLineLanes) * 16u;
                v[k] = (a && addr < total16) ? load16(bytes, addr) : make_uint4(0, 0, 0, 0);
            }
        };
        fetch(line, active);
        for (;;) {
#pragma unroll
            for (int k = 0; k < (int)kFetches; k++) {
                const uint32_t src = (uint32_t)k * (64u / kLineLanes) + lane / kLineLanes;
                *reinterpret_cast<uint4*>(tile + src * kTileRow + (lane % kLineLanes) * 16u) = v[k];
            }
            __builtin_amdgcn_wave_barrier();
            // the next line of every string (if it has one) is requested now and arrives while this one is walked
            const uint64_t p_next = REV ? line : line + kLine;
            fetch((REV ? p_next - 1u : p_next) & ~(uint64_t)(kLine - 1u), active && (REV ? p_next > b : p_next < e));
            // walk this lane's line
            const uint32_t lo_b = active ? (uint32_t)((REV ? (b > line ? b - line : 0) : p - line)) : 0u;
            const uint32_t hi_b = active ? (uint32_t)((REV ? p - line : (e - line < kLine ? e - line : kLine))) : 0u;
            const bool full = __all(!active || (lo_b == 0u && hi_b == kLine));
            if (!PACKED && full && __all(active)) {
                // every lane walks a whole line: nothing to mask (the dead state 0 maps to itself, so a string that
                // dies inside the line stays dead) -- three instructions per byte: extract, add, table read
#pragma unroll 1
                for (int q = 0; q < (int)kLineLanes; q++) {
                    const int qq = REV ? (int)kLineLanes - 1 - q : q;
                    const uint4 d = *reinterpret_cast<const uint4*>(tile + lane * kTileRow + (uint32_t)qq * 16u);
                    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                    for (int kk = 0; kk < 16; kk++) {
                        const int k = REV ? 15 - kk : kk;
                        st = s_next[st + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
                    }
                }
            } else
#pragma unroll 1
            for (int q = 0; q < (int)kLineLanes; q++) {
                const int qq = REV ? (int)kLineLanes - 1 - q : q;
                const uint4 d = *reinterpret_cast<const uint4*>(tile + lane * kTileRow + (uint32_t)qq * 16u);
                const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int kk = 0; kk < 16; kk++) {
                    const int k = REV ? 15 - kk : kk;
                    const uint32_t byte = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
                    uint32_t nx;
                    if (PACKED) {
                        uint32_t sel = tabs[NLIT];
#pragma unroll
                        for (int c = 0; c < NLIT; c++) sel = (byte == lit[c]) ? tabs[c] : sel;
                        nx = __builtin_amdgcn_ubfe(sel, st << 2, 4u);
                    } else {
                        nx = s_next[st + byte];
                    }
                    const uint32_t idx = (uint32_t)qq * 16u + (uint32_t)k;
                    st = (full || (idx >= lo_b && idx < hi_b)) ? (active ? nx : st) : st;
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (active) p = p_next;
            if (!REV && p > e) p = e;
            active = have && st != 0u && (REV ? p > b : p < e);
            if (!__any(active)) break;
            line = (REV ? p - 1u : p) & ~(uint64_t)(kLine - 1u);
        }
        }
        if (have && !r.taken) {
            if (PACKED) results[sid] = (uint8_t)((pk.accept_mask >> st) & 1u);
            else state_end<RESUME>(states, results, accept_tab, sid, r.walks ? st / kDfaRow : r.st);
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------
static bool make_packed(const HostImage& img, DfaPacked& pk) {
    if (img.dfa_states > 8 || img.n_classes > 8 || img.n_classes < 1) return false;
    std::memset(&pk, 0, sizeof pk);
    pk.n_lit = img.n_classes - 1;                      // tabulate_nfa: literal classes first, "every other byte" last
    for (uint32_t c = 0; c < pk.n_lit; c++) {
        int rep = -1;
        for (int b = 0; b < 256; b++)
            if (img.byte_class[b] == c) { if (rep >= 0) return false; rep = b; }
        if (rep < 0) return false;
        pk.lit[c] = (uint32_t)rep;
    }
    for (uint32_t c = 0; c < img.n_classes; c++)
        for (uint32_t s = 0; s < img.dfa_states; s++) pk.tab[c] |= (uint32_t)img.dfa_trans[s * img.n_classes + c] << (4 * s);
    for (uint32_t s = 0; s < img.dfa_states; s++) pk.accept_mask |= (uint32_t)(img.dfa_accept[s] != 0) << s;
    return true;
}

static_assert(kMemlessTileBytes == 4 * 64 * kTileRow, "memless_plan.h sizes the tile");

// One launch of a kernel with the fused table in LDS (p.lds bytes of it and, tiled, the input tile), with dfa_split.hip's tail behind it.
// head: what the kernel takes in front of the arguments all of them share.
template <class Kern, class... Head>
static int launch_lds(Kern kern, const EnginePlan& p, const MemlessKnobs& kn, const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes,
                      const uint64_t* d_offsets, uint64_t n, uint32_t* d_states, uint8_t* d_results, hipStream_t s, const Head&... head) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    const bool maps = img.dfa_states >= 2 && img.dfa_states <= 127;      // a lane per live state set and chunk (dfa_split.hip); beyond: no split path
    return memless_bracket(maps ? split_scheme_lds(split_lanes_log2(img.dfa_states)) : kSplitSchemeNone, kn, cx, n, s,
        [&](const SplitLaunch& sl) {
            hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, s, head..., (const uint16_t*)ds.d_dfa_trans, ds.d_dfa_accept, ds.d_byte_class,
                               img.dfa_states, img.n_classes, d_bytes, d_offsets, n, d_states, d_results, sl.args);
            return MFA_OK;
        },
        [&](const SplitLaunch& sl) { return split_tail(img, ds, sl, d_bytes, d_offsets, d_results, s, d_states); });
}

// Which kernel: plan_memless_engine (memless_plan.h) says; the packed form also asks the byte classes (make_packed).
// measured on MI355X, (a|b)*abb, 1M x 1 KiB: table in LDS 4.58 TB/s (3.25 when the packed form was measured: 2.65), untiled 1.0 TB/s -- the
// LDS table is the default, MFA_DFA_KERNEL=packed selects the SGPR form (which has no resume instantiation), "simple" the untiled walk
template <bool REV, bool RESUME>
static int launch_dfa(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint32_t* d_states, uint8_t* d_results, hipStream_t s) {
    const MemlessImage im{img.dfa_states, img.n_classes, false, false, 0, 0};
    MemlessKnobs kn = memless_knobs();
    EnginePlan p = plan_memless_engine(im, RESUME, kn, n, (uint64_t)ds.n_cus);
    DfaPacked pk{};
    if (p.engine == ENGINE_PACKED && !(make_packed(img, pk) && pk.n_lit <= 4)) {
        kn.kernel = 0;
        p = plan_memless_engine(im, RESUME, kn, n, (uint64_t)ds.n_cus);
    }
#define MFA_DFA_PACKED(NL) launch_lds(dfa_tiled_kernel<REV, true, NL, false>, p, kn, img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s, pk)
    switch (p.engine) {
        case ENGINE_L2:
            // long strings of such a table are cut by dfa_spec.hip; MFA_DFA_SPLIT=0, MFA_DFA_SPEC=0 and n >= 2^31 leave split_min 0: the same
            // kernel with the queue off, and no tail
            return memless_bracket(kSplitSchemeL2, kn, cx, n, s,
                [&](const SplitLaunch& sl) { return spec_main(img, ds, sl, d_bytes, d_offsets, n, d_results, s, d_states, p.grid); },
                [&](const SplitLaunch& sl) { return spec_tail(img, ds, sl, d_bytes, d_offsets, d_results, s, d_states); });
        case ENGINE_PACKED:
            switch (pk.n_lit) {
                case 0: return MFA_DFA_PACKED(0); case 1: return MFA_DFA_PACKED(1); case 2: return MFA_DFA_PACKED(2); case 3: return MFA_DFA_PACKED(3);
                default: return MFA_DFA_PACKED(4);
            }
        case ENGINE_TILED: return launch_lds(dfa_tiled_kernel<REV, false, 0, RESUME>, p, kn, img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s, pk);
        case ENGINE_UNTILED: return launch_lds(dfa_walk_kernel<REV, RESUME>, p, kn, img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s);
        default: return MFA_ERR_UNSUPPORTED;      // 128 to 254 state sets: mfa_match_batch has always refused them
    }
#undef MFA_DFA_PACKED
}

// d_states == NULL: mfa_match_batch; else mfa_match_batch_resume
static int launch_dfa_any(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                          uint32_t* d_states, uint8_t* d_results, hipStream_t s) {
    if (d_states != nullptr)
        return img.h.is_reversed ? launch_dfa<true, true>(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s)
                                 : launch_dfa<false, true>(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s);
    return img.h.is_reversed ? launch_dfa<true, false>(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s)
                             : launch_dfa<false, false>(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, s);
}

int launch_dfa_walk(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                    uint64_t n, uint8_t* d_results, void* stream) {
    if (img.set_wave) return launch_nfa_set_wave(img, ds, cx, d_bytes, d_offsets, n, d_results, stream);   // no table, wave tables: one string per wave (nfa_set_wave.hip)
    if (img.set_walk) return launch_nfa_set(img, ds, cx, d_bytes, d_offsets, n, d_results, stream);      // no table: the set walk (nfa_set.hip)
    return launch_dfa_any(img, ds, cx, d_bytes, d_offsets, n, nullptr, d_results, (hipStream_t)stream);
}

int launch_dfa_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint32_t* d_states, uint8_t* d_results, void* stream) {
    if (img.set_walk) return MFA_ERR_UNSUPPORTED;                              // a set-walk image's state is a set, not one number
    return launch_dfa_any(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, (hipStream_t)stream);
}

}  // namespace mfa
