// The set walk of a memory-less automaton with ONE STRING PER WAVE (nfa_set_wave.hip), the part that can be wrong without a GPU: the
// step of nfa_set_core.h (that header's lines 8-14 are the norm, image_host.cpp: Stepper is the judge) on a node set that lies ACROSS the
// lanes of a wave, the walk of one string, and the handful of lane-crossing primitives all of it goes through.  Included by the kernel
// with the device form of the primitives (WaveDev, below) and by the host harness tests/emul/nfa_set_wave_emul.cpp with the host form
// (tests/emul/wave_lanes.h: 64 lanes as an array).
//
// The reference's step is one sequential depth-first scan per byte: the node, the item position and the stack pointer are the same for
// the whole set, only the masks are wide.  So:
//   * cur, vis and nxt are ONE register each: lane l holds word l of the mask, the nodes 32 l .. 32 l + 31.  64 lanes x 32 bits: up to
//     kWaveMaxNodes = 2048 nodes.  Lanes at or beyond W = ceil(n_nodes / 32) hold zeros and load no mask word.
//   * everything else is wave-uniform and formed through P::uni (readfirstlane) or a ballot, so that the compiler knows it: the current
//     node, the item position and end, the stack pointer, the byte, its class, the lowest node still to do.  The branches do not diverge.
//   * nxt |= mask[run][class] & ~vis is one coalesced row load and two vector operations, whatever the width.
//   * the stack is per WAVE: 4 bytes a slot, its capacity the image's longest epsilon chain (at most n_nodes).  One lane writes a slot
//     with an ordinary store and the same wave reads it back in program order.
//   * input: up to 64 aligned 16-byte blocks per round, lane l block l of the round (1 KiB, coalesced), consumed a byte at a time through
//     P::word.  Only blocks that hold a byte of the string are loaded, forward and reversed; a lane whose block holds none loads nothing.
//
// The tables are those of nfa_set_core.h (same header, same sections; image_host.cpp: nfa_set_wave_build) with three differences: a mask
// row and `accept` are W words for any W from 1 to 64; a node number takes 11 bits in an item and in a stack word; a stack word is
// node << kWavePosBits | next item, which holds an image to 2^21 items.
//
// Strings in pieces (mfa_match_batch_resume_set_wide, the last section of this header): a record of 68 words per string, mfa_set_state_wide,
// carries the set from call to call -- a tag quarter and 64 node words, lane l word l; its decode and check, the walk of one piece
// from the set it holds, its encode.  The host harness of that section is tests/emul/nfa_set_wave_resume_emul.cpp, with the primitives
// of tests/emul/wave_lanes_resume.h.  (The 48-byte record of the lane kernel, mfa_set_state, has eight node words:
// mfa_match_batch_resume_set keeps refusing a wave image.)
//
// Deliberately not here: cutting a long string of a wave image across the GPU (one long string, or one long piece, holds one wave for
// its whole length; the records above are what the chunks of such a cut would hand on), and the wave kernel as the default for any image
// the lane kernel walks (MFA_SET_WAVE=1 forces it, for measurements and tests).
#ifndef MFA_NFA_SET_WAVE_CORE_H
#define MFA_NFA_SET_WAVE_CORE_H

#include "nfa_set_core.h"

namespace mfa {

static constexpr uint32_t kWaveLanes = 64;
static constexpr uint32_t kWaveMaxNodes = kWaveLanes * 32u;    // a mask word per lane
static constexpr uint32_t kWaveNodeMask = 0x7ffu;              // a node number: 11 bits, in an item and in a stack word
static constexpr uint32_t kWavePosBits = 21;                   // a stack word is node << kWavePosBits | next item: nfa_set_wave_build holds an image to 2^21 items
static_assert(kWaveMaxNodes <= kWaveNodeMask + 1u && kWavePosBits + 11u == 32u, "a node number and an item position share one 32-bit stack word");
static_assert((kWaveNodeMask & kSetItemEps) == 0u, "an epsilon item is the flag and a node number");
static constexpr uint32_t kWaveRoundBlocks = kWaveLanes;       // 16-byte blocks of input per fetch round: a block per lane

__host__ __device__ inline uint32_t wave_words_of(uint32_t n_nodes) { return (n_nodes + 31u) / 32u; }

#if defined(__HIPCC__)
// The primitives on the device.  Reg: this lane's word of a mask.  Every k, sp and address handed in is wave-uniform.
struct WaveDev {
    typedef uint32_t Reg;
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x & (kWaveLanes - 1u); }
    static __device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    static __device__ __forceinline__ Reg zero() { return 0u; }
    // "any lane not zero" and the lowest lane whose word is not zero (only asked when there is one): one ballot
    static __device__ __forceinline__ bool any(Reg r) { return __ballot(r != 0u) != 0ull; }
    static __device__ __forceinline__ uint32_t lowest(Reg r) { return (uint32_t)__builtin_ctzll(__ballot(r != 0u)); }
    // word k of a register
    static __device__ __forceinline__ uint32_t word(Reg r, uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)r, (int)uni(k)); }
    // or a bit into lane k
    static __device__ __forceinline__ void or_bit(Reg& r, uint32_t k, uint32_t bit) { r |= lane() == k ? bit : 0u; }
    // a row of W words: lane l its word l, zero at and beyond W
    static __device__ __forceinline__ Reg load_row(const uint32_t* row, uint32_t W) { return lane() < W ? row[lane()] : 0u; }
    // a value every lane reads from one place (an item, a class): made uniform for the compiler
    static __device__ __forceinline__ uint32_t load_uni(const uint32_t* p) { return uni(*p); }
    static __device__ __forceinline__ uint32_t load_uni8(const uint8_t* p) { return uni((uint32_t)*p); }
    // n_blocks (at most 64) aligned 16-byte blocks from bytes + first: lane l block l as d[0..3]; the other lanes load nothing
    static __device__ __forceinline__ void load_blocks(const uint8_t* bytes, uint64_t first, uint32_t n_blocks, Reg (&d)[4]) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (lane() < n_blocks) v = *reinterpret_cast<const uint4*>(bytes + first + (uint64_t)lane() * 16u);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    // the wave's stack (LDS): one lane stores the slot with an ordinary vector store, every lane reads it back -- the same wave, in
    // program order
    static __device__ __forceinline__ void push(uint32_t* stack, uint32_t sp, uint32_t v) {
        if (lane() == 0u) stack[sp] = v;
        __builtin_amdgcn_wave_barrier();
    }
    static __device__ __forceinline__ uint32_t pop(const uint32_t* stack, uint32_t sp) {
        __builtin_amdgcn_wave_barrier();
        return uni(stack[sp]);
    }
    // ---- the record of a string in pieces (the last section of this header); rec is 16-byte aligned ----
    // a row of 64 words: every lane stores its word, 256 bytes in one coalesced vector store
    static __device__ __forceinline__ void store_row(uint32_t* row, Reg r) { row[lane()] = r; }
    // the nodes this lane's word has, of an image of n_nodes: all ones up to n_nodes, a partial last word, zero beyond
    static __device__ __forceinline__ Reg have(uint32_t n_nodes) {
        const uint32_t first = lane() * 32u;
        return n_nodes >= first + 32u ? 0xffffffffu : n_nodes > first ? (1u << (n_nodes - first)) - 1u : 0u;
    }
    // the tag quarter (tag, reserved[3]): one 16-byte read that every lane makes of the same place, made uniform for the compiler; and
    // its store (tag, 0, 0, 0) by one lane, an ordinary 16-byte vector store
    static __device__ __forceinline__ void load_tag(const uint32_t* rec, uint32_t (&q)[4]) {
        const uint4 v = *reinterpret_cast<const uint4*>(rec);
        q[0] = uni(v.x); q[1] = uni(v.y); q[2] = uni(v.z); q[3] = uni(v.w);
    }
    static __device__ __forceinline__ void store_tag(uint32_t* rec, uint32_t tag) {
        if (lane() == 0u) *reinterpret_cast<uint4*>(rec) = make_uint4(tag, 0u, 0u, 0u);
    }
};
#endif

// eval(u) of the reference for a byte of class c.  stack: this wave's slots; a slot holds node << kWavePosBits | next item.  false: the
// stack would overflow -- the tables do not belong to this image (nfa_set_wave_build sizes it).
template <class P>
__device__ inline bool nfa_wave_eval(const NfaSetView& t, uint32_t W, uint32_t* stack, uint32_t u, uint32_t c, typename P::Reg& vis, typename P::Reg& nxt) {
    uint32_t sp = 0, node = u, pos = P::load_uni(t.item_begin + u), end = P::load_uni(t.item_begin + u + 1u);
    for (;;) {
        if (pos < end) {
            const uint32_t it = P::load_uni(t.items + pos);
            pos++;
            if (it & kSetItemEps) {
                const uint32_t to = it & kWaveNodeMask;
                if ((P::word(vis, to >> 5) >> (to & 31u)) & 1u) continue;
                if (sp >= t.depth) return false;
                P::push(stack, sp++, node << kWavePosBits | pos);
                node = to; pos = P::load_uni(t.item_begin + to); end = P::load_uni(t.item_begin + to + 1u);
            } else {
                const typename P::Reg m = P::load_row(t.masks + ((size_t)it * t.n_classes + c) * W, W);
                nxt = nxt | (m & ~vis);
            }
        } else {
            P::or_bit(vis, node >> 5, 1u << (node & 31u));
            if (sp == 0) return true;
            const uint32_t f = P::pop(stack, --sp);
            node = f >> kWavePosBits; pos = f & ((1u << kWavePosBits) - 1u); end = P::load_uni(t.item_begin + node + 1u);
        }
    }
}

// One byte of class c: cur becomes the reference's next set.  Returns 1 if that set is not empty, 0 if it is, 2 on a stack overflow.
// The nodes of cur in ascending number, those in vis left out: the lowest node of cur & ~vis, again and again -- vis only grows, and a
// node of cur below the one just evaluated is in it.
template <class P>
__device__ inline uint32_t nfa_wave_step(const NfaSetView& t, uint32_t W, uint32_t* stack, typename P::Reg& cur, uint32_t c) {
    typename P::Reg vis = P::zero(), nxt = P::zero();
    for (;;) {
        const typename P::Reg left = cur & ~vis;
        if (!P::any(left)) break;
        const uint32_t l = P::lowest(left);
        const uint32_t v = l * 32u + set_ctz(P::word(left, l));
        if (!nfa_wave_eval<P>(t, W, stack, v, c, vis, nxt)) return 2u;
    }
    cur = nxt;
    return P::any(nxt) ? 1u : 0u;
}

template <class P>
__device__ inline typename P::Reg nfa_wave_start(const NfaSetView& t) {
    typename P::Reg cur = P::zero();
    P::or_bit(cur, t.start >> 5, 1u << (t.start & 31u));
    return cur;
}
// the final pass with the empty letter: `finish` is evaluated iff cur meets the accept mask
template <class P>
__device__ inline uint8_t nfa_wave_accepts(const NfaSetView& t, uint32_t W, const typename P::Reg& cur) {
    return P::any(cur & P::load_row(t.accept, W)) ? (uint8_t)1 : (uint8_t)0;
}

// One wave, the bytes [b, e) of the batch (b < e or none), scanned upwards or (REV) downwards, from the set in cur: cur becomes the set
// reached.  Returns 1 if that set is not empty (also when there was no byte), 0 if it is -- an empty set ends the walk, the reference's
// `break` -- and 2 on a stack overflow.  A round is up to kWaveRoundBlocks aligned 16-byte blocks that all hold a byte of [b, e).
template <bool REV, class P>
__device__ inline uint32_t nfa_wave_walk_from(const NfaSetView& t, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e, typename P::Reg& cur) {
    uint64_t p = REV ? e : b;                                         // forward: next byte to consume; reverse: one past it
    while (REV ? p > b : p < e) {
        // the blocks of this round, in address order: forward from p's block towards the block of e - 1, reversed from the block of
        // p - 1 down towards b's
        const uint64_t near = (REV ? p - 1u : p) & ~(uint64_t)15, far = (REV ? b : e - 1u) & ~(uint64_t)15;
        const uint64_t span = (REV ? near - far : far - near) / 16u + 1u;
        const uint32_t n_blocks = span < kWaveRoundBlocks ? (uint32_t)span : kWaveRoundBlocks;
        const uint64_t first = REV ? near - (uint64_t)(n_blocks - 1u) * 16u : near;
        typename P::Reg d[4];
        P::load_blocks(bytes, first, n_blocks, d);
        // the round's bytes of the string: [lo, hi) relative to `first`
        const uint32_t lo = b > first ? (uint32_t)(b - first) : 0u;
        const uint32_t hi = (e - first) < (uint64_t)n_blocks * 16u ? (uint32_t)(e - first) : n_blocks * 16u;
        for (uint32_t jj = 0; jj < n_blocks; jj++) {
            const uint32_t j = REV ? n_blocks - 1u - jj : jj;
            // the block as two 64-bit halves that are shifted a byte per round: the next byte is always at a fixed place
            uint64_t lo64 = (uint64_t)P::word(d[0], j) | (uint64_t)P::word(d[1], j) << 32, hi64 = (uint64_t)P::word(d[2], j) | (uint64_t)P::word(d[3], j) << 32;
            for (uint32_t ii = 0; ii < 16u; ii++) {
                const uint32_t k = j * 16u + (REV ? 15u - ii : ii);
                const uint32_t byte = REV ? (uint32_t)(hi64 >> 56) : (uint32_t)(lo64 & 0xffu);
                if (REV) { hi64 = hi64 << 8 | lo64 >> 56; lo64 <<= 8; }
                else { lo64 = lo64 >> 8 | hi64 << 56; hi64 >>= 8; }
                if (k < lo || k >= hi) continue;
                const uint32_t alive = nfa_wave_step<P>(t, W, stack, cur, P::load_uni8(t.byte_class + byte));
                if (alive != 1u) return alive;
            }
        }
        p = REV ? first : first + (uint64_t)n_blocks * 16u;
    }
    return 1u;
}

// One wave, one string [b, e) of the batch, walked from {start}: its result byte.  A string beyond MFA_MAX_STRING_BYTES is not read and
// answers 2.
template <bool REV, class P>
__device__ inline uint8_t nfa_wave_walk(const NfaSetView& t, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e) {
    if (e - b > kSetMaxString) return 2;
    typename P::Reg cur = nfa_wave_start<P>(t);
    const uint32_t alive = nfa_wave_walk_from<REV, P>(t, W, stack, bytes, b, e, cur);
    if (alive != 1u) return alive == 0u ? (uint8_t)0 : (uint8_t)2;
    return nfa_wave_accepts<P>(t, W, cur);
}

// ---- strings in pieces (mfa_match_batch_resume_set_wide) ------------------------------------------------------------------------------
// As in nfa_set_core.h: the state of the set walk between two bytes is the set itself, so a string may be cut anywhere and a record per
// string carries the set from call to call.  The record (mfa_set_state_wide, include/mfa_hip.h) is 68 32-bit words, seventeen 16-byte
// quarters: tag, reserved[3], then nodes[64] -- lane l's word of the mask is nodes[l], whatever W the image has.  Node v is bit v & 31
// of nodes[v >> 5].  The tags and their meaning are nfa_set_core.h's (kSetStateStart, kSetStateLive, kSetStateInvalid).
static constexpr uint32_t kWaveStateWords = 4u + kWaveLanes;
static_assert(kWaveStateWords * 4u == 272u && kWaveStateWords % 4u == 0u, "a wide record is seventeen 16-byte quarters");

// The set a piece of `len` bytes is entered with: returns kSetStateLive, or kSetStateInvalid (and the empty set) for a record this image
// cannot have written -- a tag other than START or LIVE (INVALID among them, so an error stays one), a reserved word that is not zero,
// a bit for a node the image lacks (any word at or beyond its W among them) -- and for a piece beyond the limit.  START is {start}:
// `nodes` is loaded with the rest and not looked at.  n_nodes: the header's SET_H_NODES.
template <class P>
__device__ inline uint32_t nfa_wave_state_decode(const NfaSetView& t, uint32_t n_nodes, const uint32_t* rec, uint64_t len, typename P::Reg& cur) {
    uint32_t q[4];
    P::load_tag(rec, q);
    const typename P::Reg in = P::load_row(rec + 4, kWaveLanes);
    bool ok = (q[1] | q[2] | q[3]) == 0u && len <= kSetMaxString;
    if (q[0] == kSetStateStart) {
        cur = nfa_wave_start<P>(t);
    } else {
        ok = ok && q[0] == kSetStateLive && !P::any(in & ~P::have(n_nodes));
        cur = in;
    }
    if (ok) return kSetStateLive;
    cur = P::zero();
    return kSetStateInvalid;
}

// the record of a string that has reached cur (tag LIVE; lanes at and beyond W hold zero already), or of one in error (tag INVALID:
// `nodes` is zero whatever cur holds): all 64 lanes store their word, one lane the tag quarter
template <class P>
__device__ inline void nfa_wave_state_encode(uint32_t tag, const typename P::Reg& cur, uint32_t* rec) {
    P::store_row(rec + 4, tag == kSetStateLive ? cur : P::zero());
    P::store_tag(rec, tag);
}

// One wave, one piece [b, e) of the batch: the record at rec is replaced by the one behind the piece; returns the result byte -- what
// the plain call answers for the concatenation of the pieces so far (the empty set meets no mask: 0).  A string that enters dead (LIVE
// with the empty set) or in error leaves as it came and its bytes are not read.
template <bool REV, class P>
__device__ inline uint8_t nfa_wave_resume_piece(const NfaSetView& t, uint32_t n_nodes, uint32_t W, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e,
                                                uint32_t* rec) {
    typename P::Reg cur;
    uint32_t tag = nfa_wave_state_decode<P>(t, n_nodes, rec, e - b, cur);
    if (tag == kSetStateLive && P::any(cur) && nfa_wave_walk_from<REV, P>(t, W, stack, bytes, b, e, cur) == 2u) tag = kSetStateInvalid;
    nfa_wave_state_encode<P>(tag, cur, rec);
    return tag == kSetStateLive ? nfa_wave_accepts<P>(t, W, cur) : (uint8_t)2;
}

}  // namespace mfa

#endif
