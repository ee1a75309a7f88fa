// Text to batch (include/mfa_hip.h, "text to batch"): a text in device memory is split into strings -- lines, or whitespace-separated
// tokens up to an optional stop token -- and left as the batch every match entry point takes: the kept bytes back to back, offsets[0..n].
// What the host loops of the reference do per string (matchers/match.cpp:21-31: `cin >> text`; matchers/match_mfa.cpp:28-36: getline).
//
// Three passes over tiles of kSplitTileBytes, stream-ordered launches only; no workgroup ever waits for another:
//   count  one workgroup per tile: separator masks of its 16-byte blocks, the tile's kept bytes and events, its first stop token
//   scan   one workgroup: the exclusive prefix of the tiles' totals in 64 bits, the first stop token as a string index, the info record
//   write  one workgroup per tile: the masks again, a scan of them inside the workgroup, the kept bytes compacted in LDS and stored in
//          aligned 16-byte vectors, one offsets[] entry per event
// and a small kernel over the offsets for the longest string.  The rule, the marks and the geometry: text_split_core.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfa_internal.h"
#include "text_split_core.h"
#include "wave_scan.h"

namespace mfa {

static_assert(sizeof(mfa_split_info) == 32, "mfa_split_info is 32 bytes");
static_assert(sizeof(SplitTotals) == 16 && sizeof(SplitPrefix) == 16, "16 bytes per tile and pass");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The marks of this lane's four blocks of tile `tile`: d[r] the block's bytes (zero outside the text), kept[r] and events[r] its masks.
// Every lane of the wave calls this together.
template <uint32_t MODE>
__device__ __forceinline__ void lane_marks(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t tile, uint32_t wave, uint32_t lane,
                                           uint4 (&d)[kSplitRows], uint32_t (&kept)[kSplitRows], uint32_t (&events)[kSplitRows]) {
#pragma unroll
    for (uint32_t r = 0; r < kSplitRows; r++) {
        const uint64_t base = tile * kSplitTileBytes + (uint64_t)split_block_of(wave, r, lane) * 16u;
        const uint32_t valid = split_valid(base, n_text);
        d[r] = valid ? *reinterpret_cast<const uint4*>(text + base) : make_uint4(0, 0, 0, 0);      // base < n_text: inside the text rounded up to 16
        const uint32_t seps = split_block_seps(d[r], MODE);
        uint32_t prev = 0;
        if (MODE == kSplitTokens) {
            // the byte in front of the block: the last byte of the left neighbour's block (whole inside the text when this one begins
            // inside it), for lane 0 one byte of the text
            const uint32_t left = __shfl_up((valid & ~seps) >> 15, 1);
            prev = lane ? left : ((valid && base) ? (split_is_sep(text[base - 1u], MODE) ? 0u : 1u) : 0u);
        }
        const SplitMarks m = split_marks(seps, valid, prev, MODE);
        kept[r] = m.kept;
        events[r] = m.events;
    }
}

// ---- count ---------------------------------------------------------------------------------------------------------------------------
template <uint32_t MODE>
__global__ void __launch_bounds__(kSplitThreads) split_count_kernel(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t stop_lo,
                                                                    uint64_t stop_hi, uint32_t stop_len, SplitTotals* __restrict__ totals) {
    __shared__ uint32_t s_total[4], s_before[4], s_stop_pos;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t tile = blockIdx.x, tile_base = tile * kSplitTileBytes;
    if (tid == 0) s_stop_pos = kSplitNone;
    __syncthreads();
    uint4 d[kSplitRows];
    uint32_t kept[kSplitRows], events[kSplitRows];
    lane_marks<MODE>(text, n_text, tile, wave, lane, d, kept, events);
    // kept bytes in the low half, events in the high half: a tile has at most 16384 of either
    const uint64_t kept_bits = (uint64_t)kept[0] | (uint64_t)kept[1] << 16 | (uint64_t)kept[2] << 32 | (uint64_t)kept[3] << 48;
    const uint64_t event_bits = (uint64_t)events[0] | (uint64_t)events[1] << 16 | (uint64_t)events[2] << 32 | (uint64_t)events[3] << 48;
    const uint32_t sum = wave_sum((uint32_t)__popcll(kept_bits) | (uint32_t)__popcll(event_bits) << 16);
    if (lane == 0) s_total[wave] = sum;
    if (MODE == kSplitTokens && stop_len != 0u) {
        const SplitStop stop{stop_lo, stop_hi, stop_len};
#pragma unroll
        for (uint32_t r = 0; r < kSplitRows; r++) {
            const uint64_t base = tile_base + (uint64_t)split_block_of(wave, r, lane) * 16u;
            uint32_t cand = events[r] & split_block_eq(d[r], split_stop_byte(stop, 0));      // tokens that start with the stop token's first byte
            while (cand) {
                const uint32_t i = (uint32_t)__builtin_ctz(cand);
                if (split_stop_at(text, n_text, base + i, stop)) { atomicMin(&s_stop_pos, (uint32_t)(base + i - tile_base)); break; }
                cand &= cand - 1u;
            }
        }
    }
    __syncthreads();
    const uint32_t stop_pos = s_stop_pos;
    if (stop_pos != kSplitNone) {                        // (the same in every lane)
        uint32_t before = 0;
#pragma unroll
        for (uint32_t r = 0; r < kSplitRows; r++) {
            const uint64_t base = tile_base + (uint64_t)split_block_of(wave, r, lane) * 16u;
            before += split_popc(split_before(kept[r], base, tile_base + stop_pos)) | split_popc(split_before(events[r], base, tile_base + stop_pos)) << 16;
        }
        before = wave_sum(before);
        if (lane == 0) s_before[wave] = before;
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t t = s_total[0] + s_total[1] + s_total[2] + s_total[3];
        SplitTotals out{t & 0xffffu, t >> 16, kSplitNone, 0u};
        if (stop_pos != kSplitNone) {
            const uint32_t b = s_before[0] + s_before[1] + s_before[2] + s_before[3];
            out.stop_events = b >> 16;
            out.stop_kept = b & 0xffffu;
        }
        totals[tile] = out;
    }
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kScanPerThread = 16u;      // consecutive tiles a thread sums: 4096 tiles (64 MiB of text) per round of the workgroup

__global__ void __launch_bounds__(kSplitThreads) split_scan_kernel(const SplitTotals* __restrict__ totals, SplitPrefix* __restrict__ prefix,
                                                                   uint64_t n_tiles, const uint8_t* __restrict__ text, uint64_t n_text,
                                                                   uint32_t mode, mfa_split_info* __restrict__ info) {
    __shared__ uint64_t s_kept[4], s_events[4];
    __shared__ unsigned long long s_stop_index, s_stop_bytes;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) { s_stop_index = ~0ull; s_stop_bytes = ~0ull; }
    uint64_t carry_kept = 0, carry_events = 0;              // of all tiles in front of this round: the same in every thread
    uint64_t stop_index = ~0ull, stop_bytes = ~0ull;        // the first stop token this thread has met
    for (uint64_t round = 0; round < n_tiles; round += (uint64_t)kSplitThreads * kScanPerThread) {
        const uint64_t first = round + (uint64_t)tid * kScanPerThread;
        uint64_t k = 0, e = 0;
        for (uint32_t i = 0; i < kScanPerThread && first + i < n_tiles; i++) { k += totals[first + i].kept; e += totals[first + i].events; }
        const uint64_t k_incl = wave_scan_incl(k, lane), e_incl = wave_scan_incl(e, lane);
        __syncthreads();                                    // (the sums of the round before have been read)
        if (lane == 63u) { s_kept[wave] = k_incl; s_events[wave] = e_incl; }
        __syncthreads();
        uint64_t at_kept = carry_kept + k_incl - k, at_events = carry_events + e_incl - e;
        for (uint32_t w = 0; w < 4u; w++) {
            if (w < wave) { at_kept += s_kept[w]; at_events += s_events[w]; }
            carry_kept += s_kept[w]; carry_events += s_events[w];
        }
        for (uint32_t i = 0; i < kScanPerThread && first + i < n_tiles; i++) {
            const SplitTotals t = totals[first + i];
            prefix[first + i] = SplitPrefix{at_kept, at_events};
            if (t.stop_events != kSplitNone && stop_index == ~0ull) { stop_index = at_events + t.stop_events; stop_bytes = at_kept + t.stop_kept; }
            at_kept += t.kept; at_events += t.events;
        }
    }
    // string index and kept bytes both grow with the position in the text: the two minima belong to the same, the first, stop token
    __syncthreads();
    if (stop_index != ~0ull) { atomicMin(&s_stop_index, (unsigned long long)stop_index); atomicMin(&s_stop_bytes, (unsigned long long)stop_bytes); }
    __syncthreads();
    if (tid == 0) {
        const bool stopped = s_stop_index != ~0ull;
        const bool open_end = n_text != 0u && !split_is_sep(text[n_text - 1u], mode);
        info->n_strings = stopped ? (uint64_t)s_stop_index : split_string_count(carry_events, mode, open_end);
        info->n_bytes = stopped ? (uint64_t)s_stop_bytes : carry_kept;
        info->max_string_bytes = 0;
        info->stopped = stopped ? 1u : 0u;
        info->overflow = 0;
    }
}

// ---- write ---------------------------------------------------------------------------------------------------------------------------
// what no event fixes, and the fields of the info record that belong to the write call
__global__ void split_edges_kernel(mfa_split_info* __restrict__ info, uint64_t bytes_capacity, uint64_t* __restrict__ d_offsets, uint64_t max_strings) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t n_strings = info->n_strings, n_bytes = info->n_bytes;
    d_offsets[0] = 0;
    if (n_strings <= max_strings) d_offsets[n_strings] = n_bytes;
    info->max_string_bytes = 0;
    info->overflow = (n_strings > max_strings || n_bytes > bytes_capacity) ? 1u : 0u;
}

template <uint32_t MODE>
__global__ void __launch_bounds__(kSplitThreads) split_write_kernel(const uint8_t* __restrict__ text, uint64_t n_text,
                                                                    const SplitTotals* __restrict__ totals, const SplitPrefix* __restrict__ prefix,
                                                                    const mfa_split_info* __restrict__ info, uint8_t* __restrict__ d_bytes,
                                                                    uint64_t bytes_capacity, uint64_t* __restrict__ d_offsets, uint64_t max_strings) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kSplitTileBytes + 16u];      // the tile's kept bytes, compacted, from index `skew`
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t tile = blockIdx.x;
    const SplitPrefix pre = prefix[tile];
    const uint64_t n_strings = info->n_strings, n_bytes = info->n_bytes;
    const uint64_t limit_bytes = n_bytes < bytes_capacity ? n_bytes : bytes_capacity;      // no byte at or beyond it is written
    const uint64_t limit_index = n_strings < max_strings ? n_strings : max_strings;        // no offsets[] entry above it is written
    const uint32_t avail = split_clip(pre.kept, totals[tile].kept, limit_bytes);
    if (avail == 0u && split_event_index(pre.events, MODE) > limit_index) return;          // behind the stop token or the capacities (every lane alike)

    uint4 d[kSplitRows];
    uint32_t kept[kSplitRows], events[kSplitRows];
    lane_marks<MODE>(text, n_text, tile, wave, lane, d, kept, events);

    // where this lane's blocks begin among the tile's kept bytes (low half) and events (high half): blocks go by (wave, row, lane)
    uint32_t at[kSplitRows], rows_before = 0;
#pragma unroll
    for (uint32_t r = 0; r < kSplitRows; r++) {
        const uint32_t c = split_popc(kept[r]) | split_popc(events[r]) << 16;
        uint32_t incl = c;
#pragma unroll
        for (uint32_t s = 1; s < 64u; s <<= 1) {
            const uint32_t up = __shfl_up(incl, s);
            if (lane >= s) incl += up;
        }
        at[r] = rows_before + incl - c;
        rows_before += __shfl(incl, 63);
    }
    if (lane == 0) s_wave[wave] = rows_before;
    __syncthreads();
    uint32_t waves_before = 0;
    for (uint32_t w = 0; w < wave; w++) waves_before += s_wave[w];

    // stage the kept bytes; the skew makes a 16-byte piece of the destination a 16-byte piece of s_out
    const uintptr_t dst = reinterpret_cast<uintptr_t>(d_bytes) + pre.kept;
    const uint32_t skew = (uint32_t)(dst & 15u);
#pragma unroll
    for (uint32_t r = 0; r < kSplitRows; r++) {
        uint32_t to = skew + ((waves_before + at[r]) & 0xffffu);
        if (kept[r] == 0xffffu) {
            __builtin_memcpy(&s_out[to], &d[r], 16);
        } else {
            const uint32_t w[4] = {d[r].x, d[r].y, d[r].z, d[r].w};
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++)
                if ((kept[r] >> i) & 1u) s_out[to++] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
        }
    }

    // one offsets[] entry per event
#pragma unroll
    for (uint32_t r = 0; r < kSplitRows; r++) {
        const uint32_t here = waves_before + at[r];
        uint32_t ev = events[r];
        while (ev) {
            const uint32_t i = (uint32_t)__builtin_ctz(ev);
            const uint64_t index = split_event_index(pre.events + (here >> 16) + split_popc(split_below(events[r], i)), MODE);
            if (index <= limit_index) d_offsets[index] = pre.kept + (here & 0xffffu) + split_popc(split_below(kept[r], i));
            ev &= ev - 1u;
        }
    }
    __syncthreads();

    // the first `avail` staged bytes to d_bytes + pre.kept
    const SplitStorePlan plan = split_store_plan(skew, avail);
    uint8_t* const dst_line = reinterpret_cast<uint8_t*>(dst - skew);      // 16-byte aligned; s_out[x] belongs at dst_line[x]
    for (uint32_t x = plan.head_end + tid * 16u; x < plan.tail_begin; x += kSplitThreads * 16u)
        *reinterpret_cast<uint4*>(dst_line + x) = *reinterpret_cast<const uint4*>(&s_out[x]);
    if (tid < 16u) {
        const uint32_t x = skew + tid;
        if (x < plan.head_end) dst_line[x] = s_out[x];
    } else if (tid < 32u) {
        const uint32_t x = plan.tail_begin + (tid - 16u);
        if (x < plan.end) dst_line[x] = s_out[x];
    }
}

// ---- longest -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) split_longest_kernel(const uint64_t* __restrict__ d_offsets, uint64_t max_strings, mfa_split_info* __restrict__ info) {
    __shared__ unsigned long long s_max[4];
    const uint64_t n_strings = info->n_strings, n = n_strings < max_strings ? n_strings : max_strings;
    unsigned long long longest = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long len = d_offsets[k + 1u] - d_offsets[k];
        longest = len > longest ? len : longest;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long other = __shfl_xor(longest, s);
        longest = other > longest ? other : longest;
    }
    if ((threadIdx.x & 63u) == 0) s_max[threadIdx.x >> 6] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) longest = s_max[w] > longest ? s_max[w] : longest;
        if (longest) atomicMax(reinterpret_cast<unsigned long long*>(&info->max_string_bytes), longest);
    }
}

}  // namespace mfa

using namespace mfa;

extern "C" uint32_t mfa_split_tile_bytes(void) { return kSplitTileBytes; }

extern "C" int mfa_split_workspace_bytes(uint64_t n_text_bytes, size_t* bytes) {
    if (!bytes || split_tiles(n_text_bytes) > 0x7fffffffull) return MFA_ERR_INVALID_ARG;
    *bytes = (size_t)split_workspace_bytes(n_text_bytes);
    return MFA_OK;
}

// what both calls refuse before the device is touched
static int split_check(const uint8_t* d_text, uint64_t n_text_bytes, uint32_t mode, const void* d_workspace, const mfa_split_info* d_info) {
    if ((!d_text && n_text_bytes) || !d_workspace || !d_info) return MFA_ERR_INVALID_ARG;
    if (mode != MFA_SPLIT_LINES && mode != MFA_SPLIT_TOKENS) return MFA_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(d_text) & 15u) || (reinterpret_cast<uintptr_t>(d_workspace) & 15u) || (reinterpret_cast<uintptr_t>(d_info) & 7u))
        return MFA_ERR_INVALID_ARG;
    if (split_tiles(n_text_bytes) > 0x7fffffffull) return MFA_ERR_INVALID_ARG;
    return MFA_OK;
}

extern "C" int mfa_split_text_count(const uint8_t* d_text, uint64_t n_text_bytes, uint32_t mode, const char* stop_token, void* d_workspace,
                                    mfa_split_info* d_info, int device, void* stream) {
    int rc = split_check(d_text, n_text_bytes, mode, d_workspace, d_info);
    if (rc != MFA_OK) return rc;
    SplitStop stop;
    if (!split_stop_pack(stop_token, &stop) || (stop_token && mode != MFA_SPLIT_TOKENS)) return MFA_ERR_INVALID_ARG;
    rc = check_device(device);
    if (rc != MFA_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t tiles = split_tiles(n_text_bytes);
    if (tiles == 0) {                                       // no text: no strings, no tile launched
        HIP_TRY(hipMemsetAsync(d_info, 0, sizeof(mfa_split_info), s));
        return MFA_OK;
    }
    SplitTotals* totals = static_cast<SplitTotals*>(d_workspace);
    SplitPrefix* prefix = reinterpret_cast<SplitPrefix*>(totals + tiles);
    if (mode == MFA_SPLIT_LINES)
        hipLaunchKernelGGL(split_count_kernel<kSplitLines>, dim3((unsigned)tiles), dim3(kSplitThreads), 0, s, d_text, n_text_bytes, stop.lo, stop.hi, stop.len, totals);
    else
        hipLaunchKernelGGL(split_count_kernel<kSplitTokens>, dim3((unsigned)tiles), dim3(kSplitThreads), 0, s, d_text, n_text_bytes, stop.lo, stop.hi, stop.len, totals);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(kSplitThreads), 0, s, (const SplitTotals*)totals, prefix, tiles, d_text, n_text_bytes, mode, d_info);
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}

extern "C" int mfa_split_text_write(const uint8_t* d_text, uint64_t n_text_bytes, uint32_t mode, const void* d_workspace, mfa_split_info* d_info,
                                    uint8_t* d_bytes, uint64_t bytes_capacity, uint64_t* d_offsets, uint64_t max_strings, int device, void* stream) {
    int rc = split_check(d_text, n_text_bytes, mode, d_workspace, d_info);
    if (rc != MFA_OK) return rc;
    if ((!d_bytes && bytes_capacity) || !d_offsets || (reinterpret_cast<uintptr_t>(d_offsets) & 7u)) return MFA_ERR_INVALID_ARG;
    rc = check_device(device);
    if (rc != MFA_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t tiles = split_tiles(n_text_bytes);
    hipLaunchKernelGGL(split_edges_kernel, dim3(1), dim3(1), 0, s, d_info, bytes_capacity, d_offsets, max_strings);
    HIP_TRY(hipGetLastError());
    if (tiles == 0) return MFA_OK;
    const SplitTotals* totals = static_cast<const SplitTotals*>(d_workspace);
    const SplitPrefix* prefix = reinterpret_cast<const SplitPrefix*>(totals + tiles);
    if (mode == MFA_SPLIT_LINES)
        hipLaunchKernelGGL(split_write_kernel<kSplitLines>, dim3((unsigned)tiles), dim3(kSplitThreads), 0, s, d_text, n_text_bytes, totals, prefix,
                           (const mfa_split_info*)d_info, d_bytes, bytes_capacity, d_offsets, max_strings);
    else
        hipLaunchKernelGGL(split_write_kernel<kSplitTokens>, dim3((unsigned)tiles), dim3(kSplitThreads), 0, s, d_text, n_text_bytes, totals, prefix,
                           (const mfa_split_info*)d_info, d_bytes, bytes_capacity, d_offsets, max_strings);
    HIP_TRY(hipGetLastError());
    // the longest string written: a text of n bytes holds at most n + 1 strings (lines) and the caller's array max_strings
    const uint64_t most = max_strings < n_text_bytes + 1u ? max_strings : n_text_bytes + 1u;
    if (most) {
        const uint64_t blocks = (most + 255u) / 256u;
        hipLaunchKernelGGL(split_longest_kernel, dim3((unsigned)(blocks < 2048u ? blocks : 2048u)), dim3(256), 0, s, (const uint64_t*)d_offsets, max_strings, d_info);
        HIP_TRY(hipGetLastError());
    }
    return MFA_OK;
}
