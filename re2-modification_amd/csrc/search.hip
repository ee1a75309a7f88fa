// Search inside lines (include/mfa_hip.h, "search inside lines"): the leftmost-longest match of a tabulated memory-less automaton in
// every string of a batch, by two table walks per line -- what `grep` and `grep -o` ask where mfa_match_batch answers `grep -x`.
//   pass 1   from the line's end down to its begin over an injecting table (search_tables.h): the last accepting position is the
//            leftmost begin of a match.  Reads every byte of the batch once: the hot path.  Tiled where table and input tile fit 64 KiB
//            -- the staging of dfa_tiled_kernel<REV = true> (kernels.hip), a copy of its own: whole 128-byte lines, a 144-byte row
//            stride, the next line in flight while this one is walked, a fast path for full lines -- and untiled with 16-byte loads else.
//   pass 2   from that begin up, over a plain table, until the dead state: the last accepting position is the match's end.  One lane per
//            line, 16-byte loads.  Not launched without d_spans.
// The walk of a lane, what it leaves in the outputs and the plan of a call: search_core.h (tests/emul/search/search_emul.cpp runs them on a CPU).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfa_internal.h"
#include "search_core.h"

namespace mfa {

static_assert(kSearchMaxLine == MFA_MAX_STRING_BYTES, "the limit of the header");
static_assert(kSearchMaxSets * kDfaRow <= 0xffffu, "pre-multiplied states are 16-bit entries");

static constexpr uint32_t kLine = 128;                   // bytes of a line staged per round (one row of the tile)
static constexpr uint32_t kTileRow = kLine + 16;         // row stride in the LDS tile: the pad keeps ds_read_b128 groups on distinct banks
static constexpr uint32_t kLineLanes = kLine / 16;       // lanes that fetch one row, 16 bytes each
static constexpr uint32_t kFetches = kLineLanes;         // 64 / kLineLanes lines per load instruction -> kLineLanes instructions per round
static_assert(kMemlessTileBytes == 4 * 64 * kTileRow, "memless_plan.h sizes the tile");

// what a lane knows of its line before it walks
struct SearchLine { uint64_t b, e; bool too_long; uint32_t last; };
__device__ __forceinline__ SearchLine search_line(const SearchArgs& t, const uint64_t* __restrict__ offsets, uint64_t sid, bool have) {
    SearchLine ln;
    ln.b = have ? offsets[sid] : 0;
    ln.e = have ? offsets[sid + 1] : 0;
    ln.too_long = ln.e - ln.b > kSearchMaxLine;
    if (ln.too_long || t.n_states == 0u) ln.e = ln.b;          // not read
    ln.last = (have && !ln.too_long && t.n_states != 0u) ? search_first<true>(t.start_accepts, ln.b, ln.e) : kSearchNone;
    return ln;
}

// ---- pass 1, tiled ---------------------------------------------------------------------------------------------------------------------
// A wave owns 64 lines; each round, groups of 8 lanes fetch one 128-byte line of memory of one of them, the 64 rows are written to the
// padded tile, and every lane reads its own row back with ds_read_b128, from the top down.
__global__ void __launch_bounds__(256)
search_pass1_tiled_kernel(const SearchArgs t, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                          uint8_t* __restrict__ results, uint64_t* __restrict__ spans) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint8_t* tile = reinterpret_cast<uint8_t*>(lds) + wave * (64u * kTileRow);
    uint16_t* s_next = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(lds) + 4u * 64u * kTileRow);
    dfa_fill_table(s_next, t.trans, t.byte_class, t.n_states, t.n_classes, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint64_t total16 = (offsets[n] + 15u) & ~(uint64_t)15;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    if (spans != nullptr && blockIdx.x == 0 && threadIdx.x == 0) spans[2u * n] = offsets[n];
    for (uint64_t w0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u; w0 < n; w0 += n_waves * 64u) {
        const uint64_t sid = w0 + lane;
        const bool have = sid < n;
        const SearchLine ln = search_line(t, offsets, sid, have);
        const uint64_t b = ln.b;
        uint64_t p = ln.e;                                     // one past the next byte to take
        uint32_t st = kDfaRow, last = ln.last;                 // state 1, the start set
        bool active = have && p > b;
        if (__any(active)) {                                   // (a wave of empty lines has nothing to read)
            uint64_t line = (p - 1u) & ~(uint64_t)(kLine - 1u);
            // fetch: lane group g = lane >> 3 serves lines g, g + 8, ..., 128 bytes each
            uint4 v[kFetches];
            auto fetch = [&](uint64_t at, bool act) {
#pragma unroll
                for (int k = 0; k < (int)kFetches; k++) {
                    const int src = k * (int)(64u / kLineLanes) + (int)(lane / kLineLanes);
                    const uint32_t lo = __shfl((uint32_t)at, src), hi = __shfl((uint32_t)(at >> 32), src);
                    const int a = __shfl((int)act, src);
                    const uint64_t addr = (((uint64_t)hi << 32) | lo) + (lane % kLineLanes) * 16u;
                    v[k] = (a && addr < total16) ? split_load16(bytes, addr) : make_uint4(0, 0, 0, 0);
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
                // the line below (if this lane's string reaches into it) is requested now and arrives while this one is walked
                const uint64_t p_next = line;
                fetch((p_next - 1u) & ~(uint64_t)(kLine - 1u), active && p_next > b);
                const uint32_t lo_b = active ? (uint32_t)(b > line ? b - line : 0u) : 0u;
                const uint32_t hi_b = active ? (uint32_t)(p - line) : 0u;
                const uint32_t rel = (uint32_t)(line - b);     // modulo 2^32: the bytes taken lie at or above b
                if (__all(active && lo_b == 0u && hi_b == kLine)) {
#pragma unroll 1
                    for (int q = (int)kLineLanes - 1; q >= 0; q--) {
                        const uint4 d = *reinterpret_cast<const uint4*>(tile + lane * kTileRow + (uint32_t)q * 16u);
                        search_step16<true>(s_next, t.accept_from, d, 0u, 16u, rel + (uint32_t)q * 16u, st, last);
                    }
                } else {
#pragma unroll 1
                    for (int q = (int)kLineLanes - 1; q >= 0; q--) {
                        const uint4 d = *reinterpret_cast<const uint4*>(tile + lane * kTileRow + (uint32_t)q * 16u);
                        const uint32_t q0 = (uint32_t)q * 16u;
                        const uint32_t lo = lo_b > q0 ? (lo_b - q0 < 16u ? lo_b - q0 : 16u) : 0u;
                        const uint32_t hi = hi_b > q0 ? (hi_b - q0 < 16u ? hi_b - q0 : 16u) : 0u;
                        // (a block taken whole by this lane only is still walked masked: the branch is the wave's)
                        search_step16<true>(s_next, t.accept_from, d, lo, hi == 16u && lo == 0u ? 17u : hi, rel + q0, st, last);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (active) p = p_next;
                active = have && p > b;                        // no early end: an injecting table has no dead state
                if (!__any(active)) break;
                line = (p - 1u) & ~(uint64_t)(kLine - 1u);
            }
        }
        if (have) search_put_pass1(results, spans, sid, b, ln.too_long, last);
    }
}

// ---- pass 1, untiled --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
search_pass1_walk_kernel(const SearchArgs t, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                         uint8_t* __restrict__ results, uint64_t* __restrict__ spans) {
    extern __shared__ uint32_t lds[];
    uint16_t* s_next = reinterpret_cast<uint16_t*>(lds);
    dfa_fill_table(s_next, t.trans, t.byte_class, t.n_states, t.n_classes, threadIdx.x, blockDim.x);
    __syncthreads();
    if (spans != nullptr && blockIdx.x == 0 && threadIdx.x == 0) spans[2u * n] = offsets[n];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < n; sid += stride) {
        const SearchLine ln = search_line(t, offsets, sid, true);
        uint32_t last = ln.last;
        (void)search_walk<true>(s_next, t.accept_from, bytes, ln.b, ln.e, kDfaRow, &last);
        search_put_pass1(results, spans, sid, ln.b, ln.too_long, last);
    }
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------------------------
// (results and spans are what pass 1 left, earlier on the same stream)
__global__ void __launch_bounds__(256)
search_pass2_kernel(const SearchArgs t, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                    const uint8_t* __restrict__ results, uint64_t* __restrict__ spans, uint8_t* __restrict__ span_results) {
    extern __shared__ uint32_t lds[];
    uint16_t* s_next = reinterpret_cast<uint16_t*>(lds);
    dfa_fill_table(s_next, t.trans, t.byte_class, t.n_states, t.n_classes, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < n; sid += stride) {
        const uint32_t result = results[sid];
        uint64_t i = 0;
        uint32_t last = 0;                                     // the begin itself: where pass 1 found a match, an end is met at or above it
        if (result == 1u) {
            i = spans[2u * sid];
            (void)search_walk<false>(s_next, t.accept_from, bytes, i, offsets[sid + 1], kDfaRow, &last);
        }
        search_put_pass2(spans, span_results, sid, result, i, last);
    }
}

// ---- launch ----------------------------------------------------------------------------------------------------------------------------
static int search_upload_one(const SearchTable& tb, uint16_t** dst) {
    HIP_TRY(hipMalloc((void**)dst, tb.trans.empty() ? 4 : tb.trans.size() * 2));
    if (!tb.trans.empty()) HIP_TRY(hipMemcpy(*dst, tb.trans.data(), tb.trans.size() * 2, hipMemcpyHostToDevice));
    return MFA_OK;
}

int search_upload(const SearchTables& tb, DeviceState& ds) {
    if (ds.d_search[0] != nullptr) return MFA_OK;
    uint16_t* a = nullptr; uint16_t* b = nullptr;
    int rc = search_upload_one(tb.pass1, &a);
    if (rc == MFA_OK) rc = search_upload_one(tb.pass2, &b);
    if (rc != MFA_OK) { if (a) (void)hipFree(a); if (b) (void)hipFree(b); return rc; }
    ds.d_search[0] = a; ds.d_search[1] = b;
    return MFA_OK;
}

static SearchArgs search_args(const HostImage& img, const SearchTable& tb, const uint16_t* d_trans, const DeviceState& ds) {
    return SearchArgs{d_trans, ds.d_byte_class, tb.states, img.n_classes, tb.accept_from * kDfaRow, tb.start_accepts};
}

int launch_search(const HostImage& img, const SearchTables& tb, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                  uint64_t n, uint8_t* d_results, uint64_t* d_spans, uint8_t* d_span_results, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const SearchPlan p = plan_search(tb.pass1.states, tb.pass2.states, n, (uint64_t)ds.n_cus);
    const SearchArgs a1 = search_args(img, tb.pass1, ds.d_search[0], ds), a2 = search_args(img, tb.pass2, ds.d_search[1], ds);
    HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_start, s));
    if (p.form1 == SEARCH_TILED) {
        HIP_TRY(hipFuncSetAttribute((const void*)search_pass1_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds1));
        hipLaunchKernelGGL(search_pass1_tiled_kernel, dim3(p.grid1), dim3(256), p.lds1, s, a1, d_bytes, d_offsets, n, d_results, d_spans);
    } else {
        HIP_TRY(hipFuncSetAttribute((const void*)search_pass1_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds1));
        hipLaunchKernelGGL(search_pass1_walk_kernel, dim3(p.grid1), dim3(256), p.lds1, s, a1, d_bytes, d_offsets, n, d_results, d_spans);
    }
    HIP_TRY(hipGetLastError());
    if (d_spans != nullptr) {
        HIP_TRY(hipFuncSetAttribute((const void*)search_pass2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds2));
        hipLaunchKernelGGL(search_pass2_kernel, dim3(p.grid2), dim3(256), p.lds2, s, a2, d_bytes, d_offsets, n, (const uint8_t*)d_results, d_spans, d_span_results);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_stop, s));
    return MFA_OK;
}

}  // namespace mfa
