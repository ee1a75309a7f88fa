// Long strings of memory-less automata, cut across the whole GPU (gfx950).  The kernels of kernels.hip walk one string per lane, so
// the time of a call is set by its longest string.  Here a string with len >= split_min is cut into chunks; dfa_chunk_kernel
// computes every chunk's map (state reached, for every live start state: lanes are (chunk, start state) pairs), dfa_fold_kernel
// composes a string's maps in scan order and writes its result (and, for a string in pieces, its state).  Everything runs on the caller's
// stream, behind the main kernel that queued the strings, with no read-back: the device counts the long strings, chooses the chunk size and hands the chunks out.
//   memset(header) -> main kernel (queues long strings: split_take) -> dfa_plan_kernel -> dfa_chunk_kernel -> dfa_fold_kernel
// Geometry, chunk size, the chunk walk and the composition of maps are in dfa_split_core.h (checked on the CPU: tests/emul).
#include <hip/hip_runtime.h>

#include "mfa_internal.h"

namespace mfa {

static constexpr uint32_t kFoldTileBytes = 32768;           // maps of one string staged in LDS per round of the fold
static constexpr uint32_t kPlanThreads = 1024;

// ---- plan --------------------------------------------------------------------------------------------
// inclusive scan over the block's values; s[kPlanThreads - 1] is the total
__device__ inline uint64_t plan_scan(uint64_t* s, uint64_t v) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kPlanThreads; d <<= 1) {
        const uint64_t add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    return s[t];
}

// One block.  Sums the queued strings' bytes, chooses the chunk size, gives every string its range of maps.
__global__ void __launch_bounds__(kPlanThreads)
dfa_plan_kernel(const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr, SplitEntry* __restrict__ queue, uint32_t qcap,
                uint32_t arena_chunks, uint32_t chunk_min, uint32_t map_cap, uint32_t* seen) {
    __shared__ uint64_t s[kPlanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t n_seen = hdr[SPLIT_H_SEEN], n_q = n_seen < qcap ? n_seen : qcap;
    if (t == 0 && seen != nullptr) *seen = n_seen ? 2u : 1u;
    if (n_q == 0) return;                                     // (the header was zeroed: the kernels behind this one see no chunk)
    const uint32_t per = (n_q + kPlanThreads - 1u) / kPlanThreads;
    const uint32_t q0 = t * per < n_q ? t * per : n_q, q1 = q0 + per < n_q ? q0 + per : n_q;
    uint64_t sum = 0;
    for (uint32_t q = q0; q < q1; q++) sum += offsets[queue[q].sid + 1u] - offsets[queue[q].sid];
    plan_scan(s, sum);
    const uint64_t long_bytes = s[kPlanThreads - 1u];
    uint64_t chunk = split_chunk_size(long_bytes, arena_chunks, chunk_min);
    uint64_t cnt, incl, total;
    for (;;) {
        cnt = 0;
        for (uint32_t q = q0; q < q1; q++) cnt += split_chunks_of(offsets[queue[q].sid], offsets[queue[q].sid + 1u], chunk);
        incl = plan_scan(s, cnt);
        total = s[kPlanThreads - 1u];
        if (total <= map_cap) break;                          // always at once (split_map_capacity); the arena is never overrun
        chunk *= 2u;
    }
    uint64_t at = incl - cnt;
    for (uint32_t q = q0; q < q1; q++) {
        const uint64_t nc = split_chunks_of(offsets[queue[q].sid], offsets[queue[q].sid + 1u], chunk);
        queue[q].first = (uint32_t)at; queue[q].nc = (uint32_t)nc; queue[q].dead_at = 0xffffffffu;
        at += nc;
    }
    if (t == 0) { hdr[SPLIT_H_STRINGS] = n_q; hdr[SPLIT_H_CHUNKS] = (uint32_t)total; hdr[SPLIT_H_CHUNK] = (uint32_t)chunk; }
}

// ---- chunk maps --------------------------------------------------------------------------------------
// The fused table of dfa_walk_kernel in LDS.  A block of 256 lanes carries 256 >> lanes_log2 chunks, lane = (chunk, start state
// j + 1); converged lanes of a chunk read one LDS address (a broadcast), all lanes of a chunk read the same 16 bytes of input.
// Chunks are handed out by striding: the grid is sized from the CUs, the chunk count is the plan's.
template <bool REV>
__global__ void __launch_bounds__(256)
dfa_chunk_kernel(const uint16_t* __restrict__ trans, const uint8_t* __restrict__ byte_class, uint32_t n_states, uint32_t n_classes,
                 const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ hdr,
                 SplitEntry* __restrict__ queue, uint8_t* __restrict__ maps, uint32_t lanes_log2) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if (n_chunks == 0) return;                                // no long string: nothing to load, nothing to do
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t s_alive[64];
    uint16_t* s_next = reinterpret_cast<uint16_t*>(lds);
    dfa_fill_table(s_next, trans, byte_class, n_states, n_classes, threadIdx.x, blockDim.x);
    const uint32_t chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint32_t lanes = 1u << lanes_log2, per_block = 256u >> lanes_log2;
    const uint32_t slot = threadIdx.x >> lanes_log2, j = threadIdx.x & (lanes - 1u);
    const uint32_t n_groups = (n_chunks + per_block - 1u) / per_block;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t c = g * per_block + slot;
        const bool have = c < n_chunks;
        if (threadIdx.x < 64u) s_alive[threadIdx.x] = 0u;
        __syncthreads();                                      // (also: the table is complete)
        uint32_t st = 0u, q = 0u, k = 0u;
        bool walked = false;
        if (have) {
            uint32_t lo = 0u, hi = n_q;                       // the string of chunk c: the last entry with first <= c
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (queue[mid].first <= c) lo = mid; else hi = mid;
            }
            q = lo; k = c - queue[q].first;
            // a chunk behind one whose map is all 0 cannot change the answer (0 is absorbing): it gets the all-0 map without a walk.
            // The flag is looked at, never waited for.
            walked = k <= __atomic_load_n(&queue[q].dead_at, __ATOMIC_RELAXED);
            if (walked && j + 1u < n_states) {
                const uint64_t sid = queue[q].sid;
                const uint64_t b = offsets[sid], e = offsets[sid + 1u];
                uint64_t from, to;
                split_chunk_range<REV>(b, e, chunk, queue[q].nc, k, &from, &to);
                st = split_chunk_walk<REV>(s_next, bytes, from, to, (j + 1u) * kDfaRow);
            }
        }
        if (have && st != 0u) s_alive[slot] = 1u;
        __syncthreads();
        if (have) {
            maps[((uint64_t)c << lanes_log2) + j] = (uint8_t)(st / kDfaRow);
            if (j == 0u && walked && s_alive[slot] == 0u) atomicMin(&queue[q].dead_at, k);
        }
        __syncthreads();
    }
}

// ---- fold ----------------------------------------------------------------------------------------------
// One block per queued string; maps are stored in scan order, so both directions fold alike.  The string's maps come into LDS a tile at a time with loads whose addresses do not depend on any
// state (so no global round trip waits for another), 256 >> lanes_log2 runs of the tile are composed side by side for every start
// state, and lane 0 takes the string's state through the runs' maps: per tile, tile / runs + runs dependent LDS reads.
// all 256 lanes of the block: the state string q reaches from st_in over its maps, left in *s_st (read it behind a barrier)
__device__ __forceinline__ void fold_string(const SplitEntry* __restrict__ queue, uint32_t q, const uint8_t* __restrict__ maps, uint32_t lanes_log2,
                                            uint32_t st_in, uint32_t* s_tile, uint8_t* s_runs, uint32_t* s_st) {
    const uint32_t lanes = 1u << lanes_log2, runs = 256u >> lanes_log2, tile_maps = kFoldTileBytes >> lanes_log2;
    const uint32_t r = threadIdx.x >> lanes_log2, j = threadIdx.x & (lanes - 1u);
    const uint32_t first = queue[q].first, nc = queue[q].nc;
    if (threadIdx.x == 0) *s_st = st_in;
    for (uint32_t t0 = 0; t0 < nc; t0 += tile_maps) {
        const uint32_t cnt = nc - t0 < tile_maps ? nc - t0 : tile_maps;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(maps + ((uint64_t)(first + t0) << lanes_log2));
        __syncthreads();                                  // the tile's last readers are done
        for (uint32_t w = threadIdx.x; w < (cnt << lanes_log2) / 4u; w += 256u) s_tile[w] = src[w];
        __syncthreads();
        const uint32_t per = split_fold_per(cnt, runs);
        const uint32_t m0 = r * per < cnt ? r * per : cnt, m1 = m0 + per < cnt ? m0 + per : cnt;
        s_runs[threadIdx.x] = (uint8_t)split_fold_run(reinterpret_cast<const uint8_t*>(s_tile), lanes, m0, m1, j + 1u);
        __syncthreads();
        if (threadIdx.x == 0) *s_st = split_fold_run(s_runs, lanes, 0u, runs, *s_st);
    }
    __syncthreads();
}

// RESUME (mfa_match_batch_resume): a queued string starts from its word of `states` instead of 1 and the state it reaches is written back
// there; results may then be NULL (dfa_split.h has the policy).
template <bool RESUME>
__global__ void __launch_bounds__(256)
dfa_fold_kernel(const uint8_t* __restrict__ accept_tab, const uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue,
                const uint8_t* __restrict__ maps, uint32_t lanes_log2, uint32_t* __restrict__ states, uint8_t* __restrict__ results) {
    const uint32_t n_q = hdr[SPLIT_H_STRINGS];
    if (n_q == 0) return;
    __shared__ uint32_t s_tile[kFoldTileBytes / 4];
    __shared__ uint8_t s_runs[256];
    __shared__ uint32_t s_st;
    for (uint32_t q = blockIdx.x; q < n_q; q += gridDim.x) {
        const uint64_t sid = queue[q].sid;
        fold_string(queue, q, maps, lanes_log2, state_of_queued<RESUME>(states, sid), s_tile, s_runs, &s_st);
        if (threadIdx.x == 0) state_end<RESUME>(states, results, accept_tab, sid, s_st);
    }
}

// ---- host side ---------------------------------------------------------------------------------------
// (memless_plan.h: plan_split has the knobs, the quiet-workspace rule and the layout; here are its four HIP calls)
int split_begin(const SplitScheme& sc, const MemlessKnobs& kn, LaunchCtx& cx, uint64_t n, void* stream, SplitLaunch* out) {
    *out = SplitLaunch{};
    cx.split_ran = cx.spec_ran = cx.set_split_ran = false;
    if (cx.split_seen == nullptr && split_on(sc, kn, n)) {
        if (hipHostMalloc((void**)&cx.split_seen, sizeof(uint32_t), hipHostMallocMapped) == hipSuccess) *cx.split_seen = 0u;
        else { (void)hipGetLastError(); cx.split_seen = nullptr; }
    }
    const bool has_word = cx.split_seen != nullptr;
    const SplitPlan p = plan_split(sc, kn, n, SplitWorkspace{has_word, has_word ? *(volatile uint32_t*)cx.split_seen : 0u, cx.split_keep, cx.split_quiet});
    cx.split_keep = p.keep; cx.split_quiet = p.quiet;
    out->args.split_min = p.split_min;
    if (p.split_min == 0) return MFA_OK;
    out->args.seen = cx.split_seen;
    out->spec_rounds = p.rounds; out->spec_lookback = p.lookback;
    if (!p.tail) return MFA_OK;                                       // args.hdr stays NULL
    out->chunk_min = p.chunk_min; out->arena_chunks = p.arena_chunks; out->map_cap = p.map_cap;
    const int rc = ctx_reserve((void**)&cx.d_split, &cx.split_bytes, p.bytes);
    if (rc != MFA_OK) return rc;
    out->args.hdr = reinterpret_cast<uint32_t*>(cx.d_split);
    out->args.queue = reinterpret_cast<SplitEntry*>(cx.d_split + p.queue_at);
    out->args.qcap = kSplitQueueCap;
    out->maps = cx.d_split + p.arena_at;
    HIP_TRY(hipMemsetAsync(cx.d_split, 0, SPLIT_H_WORDS * sizeof(uint32_t), (hipStream_t)stream));
    cx.split_ran = sc.tail != TAIL_SET; cx.spec_ran = sc.tail == TAIL_SPEC; cx.set_split_ran = sc.tail == TAIL_SET;
    return MFA_OK;
}

// the plan kernel behind a main kernel that was given sl.args (also launched by dfa_spec.hip: spec_tail)
int split_plan(const SplitLaunch& sl, const uint64_t* d_offsets, void* stream) {
    hipLaunchKernelGGL(dfa_plan_kernel, dim3(1), dim3(kPlanThreads), 0, (hipStream_t)stream, d_offsets, sl.args.hdr, sl.args.queue, sl.args.qcap,
                       sl.arena_chunks, sl.chunk_min, sl.map_cap, sl.args.seen);
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}

template <bool REV>
static int split_tail_dir(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                          uint8_t* d_results, hipStream_t s, uint32_t* d_states) {
    const int rc = split_plan(sl, d_offsets, s);
    if (rc != MFA_OK) return rc;
    // 127 state sets: 65 532 bytes of table + 256 static, just above 64 KiB -- more than any other kernel here asks for, within the 160 KiB
    // a workgroup may have on gfx950 (tests/test_dfa_split_gpu.py runs that shape)
    const size_t lds = (size_t)img.dfa_states * kDfaRow * sizeof(uint16_t);
    const uint64_t per_cu = lds_blocks_per_cu(lds + 512u);
    const unsigned n_cus = (unsigned)ds.n_cus;
    const uint32_t lanes_log2 = split_lanes_log2(img.dfa_states);
    HIP_TRY(hipFuncSetAttribute((const void*)dfa_chunk_kernel<REV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(dfa_chunk_kernel<REV>, dim3(n_cus * (unsigned)per_cu), dim3(256), lds, s, (const uint16_t*)ds.d_dfa_trans, ds.d_byte_class,
                       img.dfa_states, img.n_classes, d_bytes, d_offsets, (const uint32_t*)sl.args.hdr, sl.args.queue, sl.maps, lanes_log2);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(d_states != nullptr ? dfa_fold_kernel<true> : dfa_fold_kernel<false>, dim3(n_cus * 2u), dim3(256), 0, s, ds.d_dfa_accept,
                       (const uint32_t*)sl.args.hdr, (const SplitEntry*)sl.args.queue, (const uint8_t*)sl.maps, lanes_log2, d_states, d_results);
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}

int split_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
               uint8_t* d_results, void* stream, uint32_t* d_states) {
    if (sl.args.hdr == nullptr) return MFA_OK;
    return img.h.is_reversed ? split_tail_dir<true>(img, ds, sl, d_bytes, d_offsets, d_results, (hipStream_t)stream, d_states)
                             : split_tail_dir<false>(img, ds, sl, d_bytes, d_offsets, d_results, (hipStream_t)stream, d_states);
}

}  // namespace mfa
