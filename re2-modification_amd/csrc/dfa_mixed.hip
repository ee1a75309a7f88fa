// The memory-less segments of a mixed call in ONE launch, written for gfx950 (MI355X): any workgroup any automaton.
// The call's eligible segments (walk_plan.h: plan_dfa_items) arrive as kernel arguments -- automaton, first string, string count each --
// and are cut into slices of 256 strings, one per lane.  A workgroup takes a run of consecutive slices (dfa_slice_lo), fills the
// fused table of a slice's automaton into LDS only when it differs from the one it holds, and walks the slice the way
// dfa_tiled_kernel (kernels.hip) walks: a wave stages one 128-byte line of each of its 64 strings through a padded LDS tile, in whole
// lines from HBM, and every lane reads its own line back 16 bytes at a time; the next line is on its way while this one is walked.
// The scan direction belongs to the automaton: one branch per slice, uniform for the workgroup.
// A string of any length is walked whole by its lane (the split path for long strings belongs to launches of their own), and the
// slices are dealt out by their number, not by their bytes: a segment of long strings beside segments of short ones leaves the grid
// unbalanced.  The launch is for many small segments of strings of similar length; MFA_MIXED_DFA_OWN moves a segment out of it.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mfa_internal.h"
#include "dfa_mixed.h"
#include "dfa_mixed_core.h"

namespace mfa {

struct MixDfaArgs {
    uint32_t n_items, pad;
    DfaItem  items[kDfaMaxItems];
};

template <bool REV>
__device__ __forceinline__ void mix_walk_slice(const uint16_t* s_next, uint8_t* tile, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ bytes,
                                               const uint64_t* __restrict__ offsets, uint64_t total16, uint64_t first, uint32_t count,
                                               uint8_t* __restrict__ results, uint32_t lane) {
    const bool have = threadIdx.x < count;
    const uint64_t sid = first + threadIdx.x;
    MixCursor<REV> c;
    c.start(have, have ? offsets[sid] : 0, have ? offsets[sid + 1] : 0);
    if (__any(c.active)) {                        // (a wave of empty strings has nothing to read)
        uint64_t line = c.line();
        // fetch: lane group g = lane / 8 serves strings g, g + 8, ..., one 128-byte line each
        uint4 v[kMixLineLanes];
        auto fetch = [&](uint64_t ln, bool act) {
#pragma unroll
            for (int k = 0; k < (int)kMixLineLanes; k++) {
                const int src = k * (int)(64u / kMixLineLanes) + (int)(lane / kMixLineLanes);
                const uint32_t lo = __shfl((uint32_t)ln, src), hi = __shfl((uint32_t)(ln >> 32), src);
                const int a = __shfl((int)act, src);
                v[k] = mix_stage16(bytes, (((uint64_t)hi << 32) | lo) + (lane % kMixLineLanes) * 16u, total16, a != 0);
            }
        };
        fetch(line, c.active);
        for (;;) {
#pragma unroll
            for (int k = 0; k < (int)kMixLineLanes; k++) {
                const uint32_t src = (uint32_t)k * (64u / kMixLineLanes) + lane / kMixLineLanes;
                *reinterpret_cast<uint4*>(tile + src * kMixTileRow + (lane % kMixLineLanes) * 16u) = v[k];
            }
            __builtin_amdgcn_wave_barrier();
            uint64_t next;
            const bool more = c.next_line(line, &next);
            fetch(next, more);
            uint32_t lo_b, hi_b;
            c.bounds(line, &lo_b, &hi_b);
            const bool whole = __all(c.active && lo_b == 0u && hi_b == kMixLine);
            c.st = mix_walk_row<REV>(s_next, tile + lane * kMixTileRow, c.st, lo_b, hi_b, whole);
            __builtin_amdgcn_wave_barrier();
            c.advance(line);
            if (!__any(c.active)) break;
            line = c.line();
        }
    }
    if (have) results[sid] = c.result(accept_tab);
}

__global__ void __launch_bounds__(256)
dfa_mixed_kernel(const MixDfaArgs a, const uint8_t* __restrict__ tables, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                 uint64_t n, uint8_t* __restrict__ results, uint64_t slices) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint8_t* tile = reinterpret_cast<uint8_t*>(lds) + wave * (64u * kMixTileRow);
    uint16_t* s_next = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(lds) + kMixTileBytes);
    const MixDfaDesc* descs = reinterpret_cast<const MixDfaDesc*>(tables);
    const uint64_t total16 = (offsets[n] + 15u) & ~(uint64_t)15;
    const uint64_t s_lo = dfa_slice_lo(slices, blockIdx.x, gridDim.x), s_hi = dfa_slice_lo(slices, blockIdx.x + 1u, gridDim.x);
    uint32_t it = 0, held = 0xffffffffu;
    uint64_t base = 0;                            // slices in front of item `it`
    for (uint64_t s = s_lo; s < s_hi; s++) {
        while (it < a.n_items && s >= base + dfa_slices_of(a.items[it].count)) { base += dfa_slices_of(a.items[it].count); it++; }
        if (it >= a.n_items) break;
        const uint32_t image = a.items[it].image;
        const MixDfaDesc d = descs[image];
        if (image != held) {
            __syncthreads();                      // (the other waves may still be walking with the table that goes)
            dfa_fill_table(s_next, reinterpret_cast<const uint16_t*>(tables + d.trans_at), tables + d.class_at, d.n_states, d.n_classes, threadIdx.x, 256u);
            __syncthreads();
            held = image;
        }
        const uint64_t in_item = (s - base) * kDfaSliceStrings;
        const uint64_t left = (uint64_t)a.items[it].count - in_item;
        const uint32_t count = left < kDfaSliceStrings ? (uint32_t)left : kDfaSliceStrings;
        if (wave * 64u < count) {
            if (d.reversed) mix_walk_slice<true>(s_next, tile, tables + d.accept_at, bytes, offsets, total16, a.items[it].first + in_item, count, results, lane);
            else mix_walk_slice<false>(s_next, tile, tables + d.accept_at, bytes, offsets, total16, a.items[it].first + in_item, count, results, lane);
        }
    }
}

// the items [i0, i1) of the plan in one launch on `stream`
int launch_dfa_mixed(const DfaPlan& plan, size_t i0, size_t i1, const uint8_t* d_tables, int n_cus, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                     uint8_t* d_results, void* stream) {
    if (i1 <= i0 || i1 - i0 > kDfaMaxItems || i1 > plan.items.size() || plan.table_bytes + kMixTileBytes > kMixLdsMax) return MFA_ERR_INVALID_ARG;
    MixDfaArgs a{};
    uint64_t slices = 0;
    for (size_t i = i0; i < i1; i++) {
        const DfaItem& it = plan.items[i];
        if (it.count == 0 || it.first + it.count > n) return MFA_ERR_INVALID_ARG;
        a.items[a.n_items++] = it;
        slices += dfa_slices_of(it.count);
    }
    const size_t lds = kMixTileBytes + plan.table_bytes;
    uint64_t blocks = slices, cap = (uint64_t)(n_cus > 0 ? n_cus : 256) * lds_blocks_per_cu(lds);
    if (blocks > cap) blocks = cap;
    static bool lds_allowed[64] = {false};                   // per device, once: the kernel may take up to 64 KiB of dynamic LDS
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !lds_allowed[dev]) {
        HIP_TRY(hipFuncSetAttribute((const void*)dfa_mixed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMixLdsMax));
        if (dev >= 0 && dev < 64) lds_allowed[dev] = true;
    }
    hipLaunchKernelGGL(dfa_mixed_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, a, d_tables, d_bytes, d_offsets, n, d_results, slices);
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}

}  // namespace mfa
