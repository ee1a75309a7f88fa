// The multi-table walk of a mixed call's memory-less segments (dfa_mixed.hip), the part that can be wrong without a GPU: what an
// automaton's tables look like in the object's upload, which 128-byte line of its string a lane walks
// next and which bytes of it, the walk of one line, and the 16-byte piece of a line that is staged.  Included by the kernel and,
// with the one-lane shim of tests/emul/, by the host harness tests/emul/dfa_mixed_emul.cpp.
#ifndef MFA_DFA_MIXED_CORE_H
#define MFA_DFA_MIXED_CORE_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "mfa_internal.h"      // HostImage; dfa_split_core.h: kDfaRow

namespace mfa {

// the input tile, as dfa_tiled_kernel's (kernels.hip): a wave stages one 128-byte line of each of its 64 strings per round; the row
// stride's pad keeps the 16 lanes of a ds_read_b128 group on distinct banks
static constexpr uint32_t kMixLine = 128;
static constexpr uint32_t kMixTileRow = kMixLine + 16;
static constexpr uint32_t kMixLineLanes = kMixLine / 16;                 // lanes that fetch one row, 16 bytes each
static constexpr uint32_t kMixTileBytes = 4u * 64u * kMixTileRow;        // four waves
static constexpr uint32_t kMixLdsMax = 64u * 1024u;                      // tile + table: the tiled kernel's rule (launch_dfa_walk)

// One automaton in the object's upload (all offsets in bytes from the start of the upload; trans_at is even): the 16-bit transition
// rows [n_states][n_classes], the accept bytes [n_states], the byte classes [256].  n_states == 0: not in the upload (a memory
// automaton, or a memory-less one that is not eligible).
struct MixDfaDesc { uint32_t trans_at, accept_at, class_at, n_states, n_classes, reversed; };

// 16 bytes of a line: nothing beyond offsets[n] of the whole batch rounded up to 16 is read (total16), and nothing for a lane without work
__device__ __forceinline__ uint4 mix_stage16(const uint8_t* bytes, uint64_t addr, uint64_t total16, bool wanted) {
    return (wanted && addr < total16) ? split_load16(bytes, addr) : make_uint4(0, 0, 0, 0);
}

// One lane's place in its string [b, e).  Forward: p = the next byte to consume; reversed: one past it.  st = state * kDfaRow; state 1 =
// {start}; state 0 = the empty set, absorbing and rejecting: a string that reaches it is done.  A string beyond MFA_MAX_STRING_BYTES is
// not walked (its result byte is 2).
template <bool REV>
struct MixCursor {
    uint64_t b, e, p;
    uint32_t st;
    bool too_long, active;
    __host__ __device__ void start(bool have, uint64_t b_, uint64_t e_) {
        b = b_; e = e_;
        too_long = have && e - b > (uint64_t)MFA_MAX_STRING_BYTES;
        p = REV ? e : b;
        st = kDfaRow;
        active = have && !too_long && e > b;
    }
    // the line that holds the next byte (of an active lane)
    __host__ __device__ uint64_t line() const { return (REV ? p - 1u : p) & ~(uint64_t)(kMixLine - 1u); }
    // the line after `ln` in scan order, and whether this string has bytes in it
    __host__ __device__ bool next_line(uint64_t ln, uint64_t* next) const {
        const uint64_t pn = REV ? ln : ln + kMixLine;
        *next = (REV ? pn - 1u : pn) & ~(uint64_t)(kMixLine - 1u);
        return active && (REV ? pn > b : pn < e);
    }
    // the bytes [lo, hi) of line `ln` that are this string's and not yet consumed (none for a lane without work)
    __host__ __device__ void bounds(uint64_t ln, uint32_t* lo, uint32_t* hi) const {
        *lo = active ? (uint32_t)(REV ? (b > ln ? b - ln : 0u) : p - ln) : 0u;
        *hi = active ? (uint32_t)(REV ? p - ln : (e - ln < kMixLine ? e - ln : kMixLine)) : 0u;
    }
    // line `ln` is walked
    __host__ __device__ void advance(uint64_t ln) {
        if (active) p = REV ? ln : ln + kMixLine;
        if (!REV && p > e) p = e;
        active = active && st != 0u && (REV ? p > b : p < e);
    }
    __host__ __device__ uint8_t result(const uint8_t* accept_tab) const { return too_long ? (uint8_t)2 : accept_tab[st / kDfaRow]; }
};

// One line from its row of the tile, 16 bytes per read, the bytes [lo, hi) taken.  whole: every lane of the wave takes the whole line --
// nothing to mask (state 0 maps to itself, so a string that dies inside the line stays dead): extract, add, table read per byte.
template <bool REV>
__device__ __forceinline__ uint32_t mix_walk_row(const uint16_t* s_next, const uint8_t* row, uint32_t st, uint32_t lo, uint32_t hi, bool whole) {
    if (whole) {
#pragma unroll 1
        for (int q = 0; q < (int)kMixLineLanes; q++) {
            const int qq = REV ? (int)kMixLineLanes - 1 - q : q;
            const uint4 d = *reinterpret_cast<const uint4*>(row + (uint32_t)qq * 16u);
            st = split_step16<REV>(s_next, st, d, 0u, 16u);
        }
    } else {
#pragma unroll 1
        for (int q = 0; q < (int)kMixLineLanes; q++) {
            const int qq = REV ? (int)kMixLineLanes - 1 - q : q;
            const uint32_t at = (uint32_t)qq * 16u;
            const uint4 d = *reinterpret_cast<const uint4*>(row + at);
            const uint32_t l = lo > at ? lo - at : 0u, h = hi > at ? (hi - at < 16u ? hi - at : 16u) : 0u;
            if (__any(l < h)) st = split_step16<REV>(s_next, st, d, l, h);
        }
    }
    return st;
}

// ---- host side: the upload ---------------------------------------------------------------------------------------------------------
// The automata's tables as the kernel reads them: one descriptor per image of the object, then the eligible images' tables back to back.
inline std::vector<uint8_t> dfa_mixed_pack(const std::vector<const HostImage*>& images, const std::vector<uint8_t>& eligible) {
    std::vector<uint8_t> out(((images.size() * sizeof(MixDfaDesc)) + 15u) & ~(size_t)15, 0);
    for (size_t k = 0; k < images.size(); k++) {
        if (!eligible[k]) continue;
        const HostImage& h = *images[k];
        MixDfaDesc d{};
        d.n_states = h.dfa_states; d.n_classes = h.n_classes; d.reversed = h.h.is_reversed ? 1u : 0u;
        d.trans_at = (uint32_t)out.size();
        for (uint32_t t : h.dfa_trans) { out.push_back((uint8_t)(t & 0xffu)); out.push_back((uint8_t)(t >> 8)); }
        d.accept_at = (uint32_t)out.size();
        out.insert(out.end(), h.dfa_accept.begin(), h.dfa_accept.end());
        d.class_at = (uint32_t)out.size();
        out.insert(out.end(), h.byte_class, h.byte_class + 256);
        out.resize((out.size() + 15u) & ~(size_t)15, 0);
        std::memcpy(out.data() + k * sizeof(MixDfaDesc), &d, sizeof d);
    }
    return out;
}

// exactly the images launch_dfa_walk gives dfa_tiled_kernel: 16-bit pre-multiplied states, table plus tile at most 64 KiB (a set-walk
// image has no table and takes a launch of its own)
inline bool dfa_mixed_eligible(const HostImage& img) {
    return img.h.kind == MFA_KIND_NFA && !img.set_walk && (size_t)img.dfa_states * kDfaRow <= 0xffffu && (size_t)img.dfa_states * kDfaRow * 2u + kMixTileBytes <= kMixLdsMax;
}
inline uint32_t dfa_mixed_table_bytes(const HostImage& img) { return img.dfa_states * kDfaRow * 2u; }

}  // namespace mfa

#endif
