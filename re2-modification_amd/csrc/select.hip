// Batch to text (include/mfa_hip.h, "batch to text"): the strings of a batch that a match call answered 1 (or 0, inverted) are compacted
// on the device -- their bytes back to back, optionally a 0x0a behind each, their output offsets and their indices -- so that only what
// matched travels back.  What `grep -x` and `grep -vx` print; the reference prints one answer per string (matchers/match_mfa.cpp:28-36).
//
// Four passes, stream-ordered launches only; no workgroup ever waits for another:
//   count   one workgroup per block of kSelectBlock strings: kept flags, output lengths in 64 bits, the block's totals, the list of
//           its kept strings
//   scan    one workgroup: the exclusive prefix of the blocks' totals in 64 bits, the info record
//   place   one workgroup per block of strings: the rank and the output offset of every kept string, one 8-byte store into
//           d_out_offsets and one into d_out_indices each, the closing offset, the overflow flag
//   gather  one workgroup per kSelectTileBytes of OUTPUT: the kept strings that reach into the tile by a search of the whole workgroup
//           in the blocks' prefixes and in d_out_offsets, their bytes through aligned 16-byte loads into a staging area in LDS -- each lane
//           a run of 64 bytes, or whole strings where the tile holds more strings than lanes -- and behind a barrier the tile out of it
//           through aligned 16-byte stores
// The rule, the workspace, the tile geometry and the whole of a chunk's way: select_core.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfa_internal.h"
#include "select_core.h"
#include "wave_scan.h"

namespace mfa {

static_assert(sizeof(mfa_select_info) == 32, "mfa_select_info is 32 bytes");
static_assert(sizeof(SelectTotals) == 16 && sizeof(SelectPrefix) == 16, "16 bytes per block and pass");
static_assert(kSelectInvert == MFA_SELECT_INVERT && kSelectNewline == MFA_SELECT_NEWLINE, "the flags of the header");

// this lane's strings of block `block`: kept[j] and out_len[j] of string first + j (not kept, 0 bytes behind the batch's end); returns
// how many of them are unanswered
__device__ __forceinline__ uint32_t lane_strings(const uint8_t* __restrict__ results, const uint64_t* __restrict__ offsets, uint64_t n, uint32_t flags,
                                                 uint64_t first, bool (&kept)[kSelectPerLane], uint64_t (&out_len)[kSelectPerLane]) {
    uint32_t unanswered = 0;
    uint64_t begin = first < n ? offsets[first] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerLane; j++) {
        const bool inside = first + j < n;
        const uint64_t end = inside ? offsets[first + j + 1u] : begin;
        const uint32_t result = inside ? results[first + j] : 0xffu;
        kept[j] = inside && select_kept(result, flags);
        unanswered += (inside && select_unanswered(result)) ? 1u : 0u;
        out_len[j] = select_out_len(kept[j], end - begin, flags);
        begin = end;
    }
    return unanswered;
}

// the kept strings and output bytes of the lanes in front of this one, and of the whole workgroup
struct BlockScan { uint64_t bytes_before, bytes_total; uint32_t kept_before, kept_total; };
__device__ __forceinline__ BlockScan block_scan(uint64_t bytes, uint32_t kept, uint64_t (&s_bytes)[4], uint32_t (&s_kept)[4]) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b_incl = wave_scan_incl(bytes, lane);
    const uint32_t k_incl = (uint32_t)wave_scan_incl(kept, lane);
    if (lane == 63u) { s_bytes[wave] = b_incl; s_kept[wave] = k_incl; }
    __syncthreads();
    BlockScan s{b_incl - bytes, 0u, k_incl - kept, 0u};
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        if (w < wave) { s.bytes_before += s_bytes[w]; s.kept_before += s_kept[w]; }
        s.bytes_total += s_bytes[w]; s.kept_total += s_kept[w];
    }
    return s;
}

// ---- count ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSelectThreads) select_count_kernel(const uint8_t* __restrict__ results, const uint64_t* __restrict__ offsets, uint64_t n,
                                                                      uint32_t flags, SelectTotals* __restrict__ totals, uint16_t* __restrict__ list) {
    __shared__ uint64_t s_bytes[4];
    __shared__ uint32_t s_kept[4], s_unanswered;
    const uint32_t tid = threadIdx.x;
    const uint64_t block = blockIdx.x;
    if (tid == 0) s_unanswered = 0;
    bool kept[kSelectPerLane];
    uint64_t out_len[kSelectPerLane];
    const uint32_t unanswered = lane_strings(results, offsets, n, flags, block * kSelectBlock + tid * kSelectPerLane, kept, out_len);
    uint64_t bytes = 0;
    uint32_t count = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerLane; j++) { bytes += out_len[j]; count += kept[j] ? 1u : 0u; }
    const BlockScan s = block_scan(bytes, count, s_bytes, s_kept);      // (its barrier orders the zero above in front of the additions below)
    if (unanswered) atomicAdd(&s_unanswered, unanswered);
    uint32_t rank = s.kept_before;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerLane; j++)
        if (kept[j]) list[block * kSelectBlock + rank++] = (uint16_t)(tid * kSelectPerLane + j);
    __syncthreads();
    if (tid == 0) totals[block] = SelectTotals{s.bytes_total, s.kept_total, s_unanswered};
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kSelectScanPerThread = 16u;      // consecutive blocks a thread sums: 4096 blocks (4 Mi strings) per round of the workgroup

__global__ void __launch_bounds__(kSelectThreads) select_scan_kernel(const SelectTotals* __restrict__ totals, SelectPrefix* __restrict__ prefix,
                                                                     uint64_t n_blocks, mfa_select_info* __restrict__ info) {
    __shared__ uint64_t s_bytes[4], s_kept[4];
    __shared__ unsigned long long s_unanswered;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_unanswered = 0;
    uint64_t carry_bytes = 0, carry_kept = 0;               // of all blocks in front of this round: the same in every thread
    unsigned long long unanswered = 0;
    for (uint64_t round = 0; round < n_blocks; round += (uint64_t)kSelectThreads * kSelectScanPerThread) {
        const uint64_t first = round + (uint64_t)tid * kSelectScanPerThread;
        uint64_t b = 0, k = 0;
        for (uint32_t i = 0; i < kSelectScanPerThread && first + i < n_blocks; i++) {
            const SelectTotals t = totals[first + i];
            b += t.bytes; k += t.kept; unanswered += t.unanswered;
        }
        const uint64_t b_incl = wave_scan_incl(b, lane), k_incl = wave_scan_incl(k, lane);
        __syncthreads();                                    // (the sums of the round before have been read)
        if (lane == 63u) { s_bytes[wave] = b_incl; s_kept[wave] = k_incl; }
        __syncthreads();
        uint64_t at_bytes = carry_bytes + b_incl - b, at_kept = carry_kept + k_incl - k;
        for (uint32_t w = 0; w < 4u; w++) {
            if (w < wave) { at_bytes += s_bytes[w]; at_kept += s_kept[w]; }
            carry_bytes += s_bytes[w]; carry_kept += s_kept[w];
        }
        for (uint32_t i = 0; i < kSelectScanPerThread && first + i < n_blocks; i++) {
            const SelectTotals t = totals[first + i];
            prefix[first + i] = SelectPrefix{at_bytes, at_kept};
            at_bytes += t.bytes; at_kept += t.kept;
        }
    }
    __syncthreads();
    if (unanswered) atomicAdd(&s_unanswered, unanswered);
    __syncthreads();
    if (tid == 0) {
        prefix[n_blocks] = SelectPrefix{carry_bytes, carry_kept};
        info->n_selected = carry_kept;
        info->n_bytes = carry_bytes;
        info->n_unanswered = s_unanswered;
        info->overflow = 0;
        info->reserved = 0;
    }
}

// ---- place ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSelectThreads) select_place_kernel(const uint8_t* __restrict__ results, const uint64_t* __restrict__ offsets, uint64_t n,
                                                                      uint32_t flags, const SelectPrefix* __restrict__ prefix,
                                                                      mfa_select_info* __restrict__ info, uint64_t bytes_capacity,
                                                                      uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ out_indices,
                                                                      uint64_t max_selected) {
    __shared__ uint64_t s_bytes[4];
    __shared__ uint32_t s_kept[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t block = blockIdx.x, first = block * kSelectBlock + tid * kSelectPerLane;
    if (block == 0 && tid == 0) {                           // what no string fixes, and the field of the info record that belongs to this call
        const uint64_t n_selected = info->n_selected, n_bytes = info->n_bytes;
        if (n_selected <= max_selected) out_offsets[n_selected] = n_bytes;
        info->overflow = (n_selected > max_selected || n_bytes > bytes_capacity) ? 1u : 0u;
    }
    bool kept[kSelectPerLane];
    uint64_t out_len[kSelectPerLane];
    (void)lane_strings(results, offsets, n, flags, first, kept, out_len);
    uint64_t bytes = 0;
    uint32_t count = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerLane; j++) { bytes += out_len[j]; count += kept[j] ? 1u : 0u; }
    const BlockScan s = block_scan(bytes, count, s_bytes, s_kept);
    const SelectPrefix pre = prefix[block];
    uint64_t rank = pre.kept + s.kept_before, at = pre.bytes + s.bytes_before;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerLane; j++) {
        if (kept[j]) {
            if (rank <= max_selected) out_offsets[rank] = at;
            if (out_indices && rank < max_selected) out_indices[rank] = first + j;
            rank++;
            at += out_len[j];
        }
    }
}

// ---- gather --------------------------------------------------------------------------------------------------------------------------
// select_last_le by the whole workgroup (select_core.h): one load per lane and one barrier per round; the same answer in every lane
__device__ __forceinline__ uint64_t group_last_le(const SelectSearch q) {
    uint64_t lo = q.lo, hi = q.hi;
    while (lo < hi) {
        const uint64_t step = select_search_step(lo, hi);
        const uint32_t count = (uint32_t)__syncthreads_count(select_search_probe(q.a, q.stride, lo, hi, step, threadIdx.x, q.x) ? 1 : 0);
        select_search_narrow(lo, hi, step, count);
    }
    return lo;
}

__global__ void __launch_bounds__(kSelectThreads) select_gather_kernel(const uint8_t* __restrict__ d_bytes, const uint64_t* __restrict__ offsets, uint64_t n_blocks,
                                                                       uint32_t flags, const SelectPrefix* __restrict__ prefix, const uint16_t* __restrict__ list,
                                                                       const mfa_select_info* __restrict__ info, uint8_t* __restrict__ out_bytes,
                                                                       uint64_t bytes_capacity, const uint64_t* __restrict__ out_offsets,
                                                                       const uint64_t* __restrict__ out_indices, uint64_t max_selected) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kSelectTileBytes];      // the tile, byte x of it at its position line0 + x
    const uint32_t tid = threadIdx.x;
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(out_bytes) & 15u);
    const uint64_t v = select_min(info->n_selected, max_selected);
    const uint64_t limit = select_min(out_offsets[v], bytes_capacity);            // no byte at or beyond it is written
    const SelectTile t = select_tile(blockIdx.x, skew, limit);
    if (t.end <= t.begin) return;                           // behind the output or the capacity (every lane alike)
    // the ranks of the kept strings that reach into the tile, and the blocks of strings they come from (the same in every lane)
    SelectReach reach{0, 0, 0, 0};
    for (uint32_t which = 0; which < 4u; which++)
        select_reach_set(which, reach, group_last_le(select_reach_search(which, reach, prefix, n_blocks, out_offsets, v, t.begin - skew, t.end - skew - 1u)));
    const SelectSource src{d_bytes, offsets, out_offsets, out_indices, prefix, list, (flags & kSelectNewline) ? 1u : 0u};
    if (select_by_strings(reach)) {                         // many short strings: a lane takes whole strings (every lane alike)
        select_fill_strings(src, s_out, t, skew, reach, tid);
    } else {                                                // this lane's run of the staging area: chunks 4 tid .. 4 tid + 3
        const SelectChunk head = select_chunk(t, tid * kSelectPerLane), tail = select_chunk(t, tid * kSelectPerLane + kSelectPerLane - 1u);
        select_fill_run(src, s_out, t, head.begin, tail.end > head.begin ? tail.end : head.begin, skew, reach);
    }
    __syncthreads();
    uint8_t* const dst_line = out_bytes - skew + t.line0;   // 16-byte aligned; never touched below out_bytes
#pragma unroll
    for (uint32_t i = 0; i < kSelectPerLane; i++) select_store_chunk(s_out, dst_line, t, select_chunk(t, i * kSelectThreads + tid));
}

}  // namespace mfa

using namespace mfa;

extern "C" int mfa_select_workspace_bytes(uint64_t n_strings, size_t* bytes) {
    if (!bytes || n_strings >= kSelectMaxStrings) return MFA_ERR_INVALID_ARG;
    *bytes = (size_t)select_workspace_bytes(n_strings);
    return MFA_OK;
}

// what both calls refuse before the device is touched
static int select_check(const uint8_t* d_results, const uint64_t* d_offsets, uint64_t n, uint32_t flags, const void* d_workspace, const mfa_select_info* d_info) {
    if (!d_results || !d_offsets || !d_workspace || !d_info) return MFA_ERR_INVALID_ARG;
    if (flags & ~(MFA_SELECT_INVERT | MFA_SELECT_NEWLINE)) return MFA_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 15u) || (reinterpret_cast<uintptr_t>(d_info) & 7u) || (reinterpret_cast<uintptr_t>(d_offsets) & 7u))
        return MFA_ERR_INVALID_ARG;
    if (n >= kSelectMaxStrings) return MFA_ERR_INVALID_ARG;
    return MFA_OK;
}

extern "C" int mfa_select_count(const uint8_t* d_results, const uint64_t* d_offsets, uint64_t n, uint32_t flags, void* d_workspace,
                                mfa_select_info* d_info, int device, void* stream) {
    int rc = select_check(d_results, d_offsets, n, flags, d_workspace, d_info);
    if (rc != MFA_OK) return rc;
    rc = check_device(device);
    if (rc != MFA_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t blocks = select_blocks(n);
    uint8_t* const work = static_cast<uint8_t*>(d_workspace);
    SelectTotals* totals = reinterpret_cast<SelectTotals*>(work);
    SelectPrefix* prefix = reinterpret_cast<SelectPrefix*>(work + select_prefix_at(blocks));
    uint16_t* list = reinterpret_cast<uint16_t*>(work + select_list_at(blocks));
    if (blocks) {
        hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)blocks), dim3(kSelectThreads), 0, s, d_results, d_offsets, n, flags, totals, list);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kSelectThreads), 0, s, (const SelectTotals*)totals, prefix, blocks, d_info);      // (no string: the record of zeros)
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}

extern "C" int mfa_select_write(const uint8_t* d_bytes, const uint64_t* d_offsets, const uint8_t* d_results, uint64_t n, uint32_t flags,
                                const void* d_workspace, mfa_select_info* d_info, uint8_t* d_out_bytes, uint64_t bytes_capacity,
                                uint64_t* d_out_offsets, uint64_t* d_out_indices, uint64_t max_selected, int device, void* stream) {
    int rc = select_check(d_results, d_offsets, n, flags, d_workspace, d_info);
    if (rc != MFA_OK) return rc;
    if (!d_bytes || (!d_out_bytes && bytes_capacity) || !d_out_offsets) return MFA_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(d_out_offsets) & 7u) || (reinterpret_cast<uintptr_t>(d_out_indices) & 7u)) return MFA_ERR_INVALID_ARG;
    rc = check_device(device);
    if (rc != MFA_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t blocks = select_blocks(n);
    const uint8_t* const work = static_cast<const uint8_t*>(d_workspace);
    const SelectPrefix* prefix = reinterpret_cast<const SelectPrefix*>(work + select_prefix_at(blocks));
    const uint16_t* list = reinterpret_cast<const uint16_t*>(work + select_list_at(blocks));
    // (no string: one workgroup for out_offsets[0] and the overflow flag)
    hipLaunchKernelGGL(select_place_kernel, dim3((unsigned)(blocks ? blocks : 1u)), dim3(kSelectThreads), 0, s, d_results, d_offsets, n, flags, prefix, d_info,
                       bytes_capacity, d_out_offsets, d_out_indices, max_selected);
    HIP_TRY(hipGetLastError());
    if (blocks == 0 || bytes_capacity == 0) return MFA_OK;
    // one workgroup per tile the capacity can hold: the size of the output is known on the device only
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(d_out_bytes) & 15u);
    const uint64_t tiles = select_tiles(select_min(bytes_capacity, kSelectMaxCapacity), skew);
    hipLaunchKernelGGL(select_gather_kernel, dim3((unsigned)tiles), dim3(kSelectThreads), 0, s, d_bytes, d_offsets, blocks, flags, prefix, list,
                       (const mfa_select_info*)d_info, d_out_bytes, bytes_capacity, (const uint64_t*)d_out_offsets, (const uint64_t*)d_out_indices, max_selected);
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}
