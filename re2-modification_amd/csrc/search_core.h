// Search inside lines (mfa_search_batch), the part that can be wrong without a GPU: the walk of one lane over one of the two tables of
// search_tables.h, what it leaves in the outputs, and which kernels a call launches.  Included by search.hip and, with the one-lane shim
// of tests/emul/, by the host harness tests/emul/search/search_emul.cpp.
//
// A walk looks at the positions BETWEEN bytes: it starts on one (pass 1 on the line's end, pass 2 on the match's begin), and every byte
// it takes puts it on the next one (pass 1 one down, pass 2 one up).  It remembers the last position at which its state accepted, as a
// 32-bit distance from the lower end of its range -- a line has at most MFA_MAX_STRING_BYTES bytes.  The accept test is one compare:
// the fused table's entries are states pre-multiplied by kDfaRow, and the accepting sets are numbered highest.
#ifndef MFA_SEARCH_CORE_H
#define MFA_SEARCH_CORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dfa_split_core.h"      // kDfaRow, dfa_fill_table, split_load16
#include "memless_plan.h"        // lds_blocks_per_cu, persistent_grid, kMemlessTileBytes

namespace mfa {

static constexpr uint32_t kSearchNone = 0xffffffffu;            // no accepting position met
static constexpr uint64_t kSearchMaxLine = 0x00ffffffu;         // MFA_MAX_STRING_BYTES

// what the kernels are given of one table (search_tables.h: SearchTable, on the device)
struct SearchArgs {
    const uint16_t* trans;               // [n_states][n_classes]
    const uint8_t*  byte_class;
    uint32_t        n_states, n_classes; // n_states == 0: no table, nothing walks
    uint32_t        accept_from;         // pre-multiplied: states at and above it accept
    uint32_t        start_accepts;
};

// 16 bytes of input, bytes [lo, hi) of the block taken, downwards (DOWN) or upwards.  rel: the distance of the block's byte 0 from the
// walk's origin, modulo 2^32 (a ragged first block begins below the origin; the bytes taken do not).
template <bool DOWN>
__device__ __forceinline__ void search_step16(const uint16_t* s_next, uint32_t accept_from, const uint4 d, uint32_t lo, uint32_t hi, uint32_t rel,
                                              uint32_t& st, uint32_t& last) {
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
    if (lo == 0u && hi == 16u) {
        // a whole block: extract, add, table read, and the one compare and select more than a whole-string walk has
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const int k = DOWN ? 15 - kk : kk;
            st = s_next[st + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
            last = st >= accept_from ? rel + (uint32_t)k + (DOWN ? 0u : 1u) : last;
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const int k = DOWN ? 15 - kk : kk;
            const uint32_t nx = s_next[st + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
            const bool take = (uint32_t)k >= lo && (uint32_t)k < hi;
            st = take ? nx : st;
            last = (take && nx >= accept_from) ? rel + (uint32_t)k + (DOWN ? 0u : 1u) : last;
        }
    }
}

// `last` before the first byte: the walk stands on its first position, whose state is the start set
template <bool DOWN>
__host__ __device__ inline uint32_t search_first(uint32_t start_accepts, uint64_t lo, uint64_t hi) {
    return start_accepts ? (DOWN ? (uint32_t)(hi - lo) : 0u) : kSearchNone;
}

// One lane: the bytes [lo, hi) of the batch from state st (pre-multiplied), from hi down to lo (DOWN: pass 1, which cannot stop early --
// an injecting table has no dead end) or from lo up to hi or the dead state (pass 2).  *last: the distance from lo of the last accepting
// position met, left alone when none is.  Only 16-byte blocks that hold a byte of [lo, hi) are read, the next one while this one is walked.
template <bool DOWN>
__device__ inline uint32_t search_walk(const uint16_t* s_next, uint32_t accept_from, const uint8_t* bytes, uint64_t lo, uint64_t hi, uint32_t st, uint32_t* last) {
    if (lo >= hi) return st;
    uint32_t l = *last;
    uint64_t blk = (DOWN ? hi - 1u : lo) & ~(uint64_t)15;
    uint4 d = split_load16(bytes, blk);
    for (;;) {
        const uint64_t nblk = DOWN ? blk - 16u : blk + 16u;                 // (DOWN below address 0: wraps, and more is then false)
        const bool more = DOWN ? blk > lo : nblk < hi;
        const uint4 dn = more ? split_load16(bytes, nblk) : make_uint4(0, 0, 0, 0);
        const uint32_t a = lo > blk ? (uint32_t)(lo - blk) : 0u, b = hi - blk < 16u ? (uint32_t)(hi - blk) : 16u;
        search_step16<DOWN>(s_next, accept_from, d, a, b, (uint32_t)(blk - lo), st, l);
        if (!more || (!DOWN && st == 0u)) break;
        blk = nblk; d = dn;
    }
    *last = l;
    return st;
}

// ---- what the passes leave ------------------------------------------------------------------------------------------------------------
// Pass 1, line k = [b, e): last = the distance from b of the leftmost begin of a match (kSearchNone: there is none).  A line beyond the
// limit is not read and answered 2.  Both ends of the span are put on the match's begin: pass 2 moves the upper one.
__host__ __device__ inline void search_put_pass1(uint8_t* results, uint64_t* spans, uint64_t k, uint64_t b, bool too_long, uint32_t last) {
    const bool found = !too_long && last != kSearchNone;
    results[k] = too_long ? (uint8_t)2 : found ? (uint8_t)1 : (uint8_t)0;
    if (spans != nullptr) {
        const uint64_t i = found ? b + last : b;
        spans[2u * k] = i; spans[2u * k + 1u] = i;
    }
}
// Pass 2, line k with result byte `result`: last = the distance from the match's begin i of its end
__host__ __device__ inline void search_put_pass2(uint64_t* spans, uint8_t* span_results, uint64_t k, uint32_t result, uint64_t i, uint32_t last) {
    if (result == 1u) spans[2u * k + 1u] = i + last;
    if (span_results != nullptr) { span_results[2u * k] = (uint8_t)result; span_results[2u * k + 1u] = 0; }
}

// ---- plan -----------------------------------------------------------------------------------------------------------------------------
// Pass 1 stages its input through LDS in whole 128-byte lines when table and tile fit 64 KiB -- the bound of plan_memless_engine -- and
// else walks untiled with 16-byte loads; pass 2 is always untiled.  Both are persistent: a workgroup of 256 lanes takes 256 lines per
// round, and the grid is what the CUs keep resident.
enum SearchForm : uint32_t { SEARCH_TILED = 1, SEARCH_UNTILED = 2 };
struct SearchPlan { SearchForm form1; size_t lds1, lds2; unsigned grid1, grid2; };

inline size_t search_table_bytes(uint32_t states) { return (size_t)states * kDfaRow * 2u; }

inline SearchPlan plan_search(uint32_t states1, uint32_t states2, uint64_t n, uint64_t n_cus) {
    SearchPlan p{};
    const size_t t1 = search_table_bytes(states1);
    p.form1 = t1 + kMemlessTileBytes <= 64u * 1024u ? SEARCH_TILED : SEARCH_UNTILED;
    p.lds1 = p.form1 == SEARCH_TILED ? t1 + kMemlessTileBytes : t1;
    p.lds2 = search_table_bytes(states2);
    p.grid1 = persistent_grid(n, 256, n_cus, lds_blocks_per_cu(p.lds1));
    p.grid2 = persistent_grid(n, 256, n_cus, lds_blocks_per_cu(p.lds2));
    return p;
}

}  // namespace mfa

#endif
