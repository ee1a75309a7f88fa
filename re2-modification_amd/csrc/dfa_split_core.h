// The part of the split path for long strings of memory-less automata (dfa_split.hip) that can be wrong without a GPU: where a
// string is cut, how large the chunks are, the map of one chunk and the composition of maps.  Included by the kernels and, with
// the one-lane shim of tests/emul/, by the host harness tests/emul/dfa_split_emul.cpp.
//
// A tabulated automaton's step over a stretch of input is a map from state sets to state sets, and maps compose associatively
// (the data-parallel finite-state-machine construction).  So a long string is cut into chunks, every chunk's map is
// computed for every start state at once -- lanes are (chunk, start state) pairs -- and the maps are composed in scan order.
#ifndef MFA_DFA_SPLIT_CORE_H
#define MFA_DFA_SPLIT_CORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfa {

static constexpr uint32_t kDfaRow = 258;     // 16-bit entries per state row of the fused LDS table (256 + 2 pad)

// entry (state, byte) of the fused table = next state * kDfaRow; thread `tid` of `threads` fills its share
__host__ __device__ inline void dfa_fill_table(uint16_t* s_next, const uint16_t* trans, const uint8_t* byte_class, uint32_t n_states, uint32_t n_classes,
                                               uint32_t tid, uint32_t threads) {
    for (uint32_t k = tid; k < n_states * 256u; k += threads) {
        const uint32_t st = k >> 8, b = k & 255u;
        s_next[st * kDfaRow + b] = (uint16_t)(trans[st * n_classes + byte_class[b]] * kDfaRow);
    }
}

// ---- geometry ----------------------------------------------------------------------------------------
// The chunk grid of the string [b, e) is anchored at b rounded DOWN to 16 and has a pitch of `chunk` bytes (a multiple of 16):
// every chunk border inside the string is 16-byte aligned in memory, only the string's first and last chunk are ragged.
__host__ __device__ inline uint64_t split_chunks_of(uint64_t b, uint64_t e, uint64_t chunk) {
    return e > b ? (e - (b & ~(uint64_t)15) + chunk - 1u) / chunk : 0u;
}

// memory range [lo, hi) of the k-th chunk IN SCAN ORDER (a reversed automaton scans from e down to b) of a string of nc chunks
template <bool REV>
__host__ __device__ inline void split_chunk_range(uint64_t b, uint64_t e, uint64_t chunk, uint64_t nc, uint64_t k, uint64_t* lo, uint64_t* hi) {
    const uint64_t j = REV ? nc - 1u - k : k, a0 = b & ~(uint64_t)15;
    const uint64_t l = a0 + j * chunk, h = l + chunk;
    *lo = l < b ? b : l;
    *hi = h > e ? e : h;
}

// The chunk size the device chooses: with it the maps of `long_bytes` bytes of long strings fit an arena sized for
// split_map_capacity(arena_chunks, queue capacity) maps, whatever long_bytes is.
__host__ __device__ inline uint64_t split_chunk_size(uint64_t long_bytes, uint64_t arena_chunks, uint64_t chunk_min) {
    const uint64_t c = (long_bytes / arena_chunks + 15u) & ~(uint64_t)15;
    return c > chunk_min ? c : chunk_min;
}
// sum of split_chunks_of <= long_bytes / chunk + 2 per string, and long_bytes / chunk < arena_chunks * 17 / 16 (chunk >= 16 and
// chunk >= floor(long_bytes / arena_chunks)): the arena has room for this many maps
__host__ __device__ inline uint64_t split_map_capacity(uint64_t arena_chunks, uint64_t queue_cap) {
    return arena_chunks + arena_chunks / 16u + 2u * queue_cap + 2u;
}

// lanes per chunk: the live state sets (all but state 0, the empty set, which maps to itself and needs no lane) rounded up to a
// power of two, at least 4; log2 of it.  n_states <= 127 gives at most 128.
__host__ __device__ inline uint32_t split_lanes_log2(uint32_t n_states) {
    uint32_t l = 2;
    while ((1u << l) + 1u < n_states) l++;
    return l;
}

// ---- the map of one chunk ------------------------------------------------------------------------------
__device__ __forceinline__ uint4 split_load16(const uint8_t* bytes, uint64_t blk) { return *reinterpret_cast<const uint4*>(bytes + blk); }

// 16 bytes of input, bytes [lo, hi) of the block taken; st = state * kDfaRow as in dfa_walk_kernel
template <bool REV>
__device__ __forceinline__ uint32_t split_step16(const uint16_t* s_next, uint32_t st, const uint4 d, uint32_t lo, uint32_t hi) {
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
    if (lo == 0u && hi == 16u) {
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const int k = REV ? 15 - kk : kk;
            st = s_next[st + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const int k = REV ? 15 - kk : kk;
            const uint32_t nx = s_next[st + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
            st = ((uint32_t)k >= lo && (uint32_t)k < hi) ? nx : st;
        }
    }
    return st;
}

// One lane: the state reached from st over the bytes [lo, hi) of the batch, scanned upwards or (REV) downwards.  Only 16-byte blocks
// that hold a byte of [lo, hi) are read.  Four blocks are walked per round while the next four are on their way.  A wave whose
// lanes have all reached state 0 stops (state 0 is absorbing).
template <bool REV>
__device__ inline uint32_t split_chunk_walk(const uint16_t* s_next, const uint8_t* bytes, uint64_t lo, uint64_t hi, uint32_t st) {
    if (lo >= hi) return st;
    const uint64_t first = lo & ~(uint64_t)15, last = (hi - 1u) & ~(uint64_t)15;
    const uint64_t nblk = (last - first) / 16u + 1u;
    uint4 q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = (uint64_t)k < nblk ? split_load16(bytes, REV ? last - 16u * k : first + 16u * k) : make_uint4(0, 0, 0, 0);
    for (uint64_t i = 0; i < nblk; i += 4u) {
        uint4 nq[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t x = i + 4u + (uint64_t)k;
            nq[k] = x < nblk ? split_load16(bytes, REV ? last - 16u * x : first + 16u * x) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t x = i + (uint64_t)k;
            if (x < nblk) {
                const uint64_t a = REV ? last - 16u * x : first + 16u * x;
                const uint32_t l = lo > a ? (uint32_t)(lo - a) : 0u, h = hi - a < 16u ? (uint32_t)(hi - a) : 16u;
                st = split_step16<REV>(s_next, st, q[k], l, h);
            }
        }
        if (!__any(st != 0u)) break;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = nq[k];
    }
    return st;
}

// ---- composing maps ------------------------------------------------------------------------------------
// A map is `lanes` bytes: entry j = the state reached from state j + 1 (plain state numbers; state 0 maps to itself and is not
// stored).  The state reached from st over the maps m0 .. m1-1, stored back to back at `maps`.
__device__ inline uint32_t split_fold_run(const uint8_t* maps, uint32_t lanes, uint32_t m0, uint32_t m1, uint32_t st) {
    for (uint32_t m = m0; m < m1; m++) {
        const uint32_t nx = maps[m * lanes + (st ? st - 1u : 0u)];
        st = st ? nx : 0u;
    }
    return st;
}

// The fold of one string works on tiles of maps held in LDS: `runs` groups of lanes compose one run of consecutive maps each, for
// every start state, and one lane then takes the string's state through the `runs` results.  Maps of a run: [r * per, r * per + per)
// cut at cnt, per = split_fold_per(cnt, runs).
__host__ __device__ inline uint32_t split_fold_per(uint32_t cnt, uint32_t runs) { return (cnt + runs - 1u) / runs; }

}  // namespace mfa

#endif
