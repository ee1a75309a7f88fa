// The set walk of a memory-less automaton (nfa_set.hip), the part that can be wrong without a GPU: the tables of one automaton, the
// reference's step (automata.cpp:98-128) on a bit mask of live nodes, the walk of one string, and the record that carries a string's set
// from call to call.  Included by the kernel and, with the
// one-lane shim of tests/emul/, by the host harnesses tests/emul/nfa_set_emul.cpp and nfa_set_resume_emul.cpp.
//
// The engine for automata whose determinisation passes the tabulation limit (image_host.cpp: tabulate_nfa): a lane's state is the SET of
// live nodes, W 32-bit words of mask (node v = bit v & 31 of word v >> 5), and every input byte runs the reference's own step on it.
// That step, exactly (image_host.cpp: Stepper is the norm):
//   vis = {}, nxt = {};  for every node v of cur in ascending number: if v is not in vis, eval(v)
//   eval(u): u's edges in list order -- an edge whose target is in vis is skipped, letter edges included; an epsilon edge recurses; a
//            letter edge whose label is the byte or '.' adds its target to nxt -- and AFTER the scan u joins vis.
// Between two epsilon edges of a node vis does not change, so a run of consecutive letter edges is one mask per byte class:
// nxt |= mask[run][class] & ~vis.  A node's edge list becomes a list of ITEMS: epsilon edges and letter runs, in list order.
// The recursion is an explicit stack of (node, next item), its capacity the longest epsilon chain of the image (nfa_set_build).
//
// Supported: up to kSetMaxNodes = 256 nodes (W = 1, 2, 4 or 8), up to 255 byte classes, no cycle of epsilon edges, a stack of at most
// kSetMaxDepth slots.
#ifndef MFA_NFA_SET_CORE_H
#define MFA_NFA_SET_CORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfa {

static constexpr uint32_t kSetMaxNodes = 256;
static constexpr uint32_t kSetMaxDepth = 48;               // stack slots per lane: 48 * 256 lanes * 4 bytes = 48 KiB of LDS
static constexpr uint32_t kSetItemEps = 0x80000000u;       // item: an epsilon edge to node (item & kSetNodeMask); else a letter run, its number
static constexpr uint32_t kSetNodeMask = 0xffu;            // a node number: 8 bits, in an item and in a stack word
static constexpr uint32_t kSetPosBits = 24;                // a stack word is node << kSetPosBits | next item: nfa_set_build holds an image to 2^24 items
static_assert(kSetMaxNodes <= kSetNodeMask + 1u && kSetPosBits + 8u == 32u, "a node number and an item position share one 32-bit stack word");
static constexpr uint64_t kSetMaxString = 0x00ffffffu;     // MFA_MAX_STRING_BYTES

// The tables, 32-bit words: a header, then the sections it names (offsets in words from the start of the tables).
enum : uint32_t {
    SET_H_NODES = 0, SET_H_WORDS, SET_H_CLASSES, SET_H_DEPTH, SET_H_START, SET_H_REVERSED, SET_H_TOTAL,
    SET_H_ITEM_BEGIN,      // [n_nodes + 1]: node u's items are items[item_begin[u] .. item_begin[u + 1])
    SET_H_ITEMS,           // [n_items]
    SET_H_MASKS,           // [n_runs][n_classes][W]: targets of the run's edges that take a byte of the class
    SET_H_ACCEPT,          // [W]: nodes whose epsilon closure holds `finish` (the final pass, automata.cpp:201-208)
    SET_H_BYTE_CLASS,      // [64]: 256 bytes, the class of every input byte (tabulate_nfa's classes)
    SET_H_SIZE = 16
};

struct NfaSetView {
    const uint32_t* item_begin;
    const uint32_t* items;
    const uint32_t* masks;
    const uint32_t* accept;
    const uint8_t*  byte_class;
    uint32_t n_classes, depth, start;
};

// hdr: the header (anywhere); base: where the sections are read from (LDS copy or global memory)
__host__ __device__ inline NfaSetView nfa_set_view(const uint32_t* hdr, const uint32_t* base) {
    NfaSetView t;
    t.item_begin = base + hdr[SET_H_ITEM_BEGIN];
    t.items = base + hdr[SET_H_ITEMS];
    t.masks = base + hdr[SET_H_MASKS];
    t.accept = base + hdr[SET_H_ACCEPT];
    t.byte_class = reinterpret_cast<const uint8_t*>(base + hdr[SET_H_BYTE_CLASS]);
    t.n_classes = hdr[SET_H_CLASSES]; t.depth = hdr[SET_H_DEPTH]; t.start = hdr[SET_H_START];
    return t;
}

// bit v of a mask; the word is chosen by compares, not by an index: the mask stays in registers
template <int W>
__host__ __device__ __forceinline__ bool set_has(const uint32_t (&m)[W], uint32_t v) {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < W; k++) w = (v >> 5) == (uint32_t)k ? m[k] : w;
    return (w >> (v & 31u)) & 1u;
}
template <int W>
__host__ __device__ __forceinline__ void set_put(uint32_t (&m)[W], uint32_t v) {
#pragma unroll
    for (int k = 0; k < W; k++) m[k] |= (v >> 5) == (uint32_t)k ? 1u << (v & 31u) : 0u;
}
__host__ __device__ __forceinline__ uint32_t set_ctz(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__ffs((int)x) - 1u;
#else
    return (uint32_t)__builtin_ctz(x);
#endif
}

// eval(u) of the reference for a byte of class c.  stack: this lane's slots, `stride` words apart ([slot][lane] in LDS); a slot holds
// node << kSetPosBits | next item.  false: the stack would overflow -- the tables do not belong to this image (nfa_set_build sizes it).
template <int W>
__host__ __device__ inline bool nfa_set_eval(const NfaSetView& t, uint32_t* stack, uint32_t stride, uint32_t u, uint32_t c, uint32_t (&vis)[W],
                                             uint32_t (&nxt)[W]) {
    uint32_t sp = 0, node = u, pos = t.item_begin[u], end = t.item_begin[u + 1u];
    for (;;) {
        if (pos < end) {
            const uint32_t it = t.items[pos++];
            if (it & kSetItemEps) {
                const uint32_t to = it & kSetNodeMask;
                if (set_has<W>(vis, to)) continue;
                if (sp >= t.depth) return false;
                stack[sp++ * stride] = node << kSetPosBits | pos;
                node = to; pos = t.item_begin[to]; end = t.item_begin[to + 1u];
            } else {
                const uint32_t* m = t.masks + ((size_t)it * t.n_classes + c) * (uint32_t)W;
#pragma unroll
                for (int k = 0; k < W; k++) nxt[k] |= m[k] & ~vis[k];
            }
        } else {
            set_put<W>(vis, node);
            if (sp == 0) return true;
            const uint32_t f = stack[--sp * stride];
            node = f >> kSetPosBits; pos = f & ((1u << kSetPosBits) - 1u); end = t.item_begin[node + 1u];
        }
    }
}

// One byte of class c: cur becomes the reference's next set.  Returns 1 if that set is not empty, 0 if it is, 2 on a stack overflow.
template <int W>
__host__ __device__ inline uint32_t nfa_set_step(const NfaSetView& t, uint32_t* stack, uint32_t stride, uint32_t (&cur)[W], uint32_t c) {
    uint32_t vis[W], nxt[W];
#pragma unroll
    for (int k = 0; k < W; k++) { vis[k] = 0; nxt[k] = 0; }
#pragma unroll
    for (int k = 0; k < W; k++) {
        uint32_t left = cur[k];
        while (left) {
            const uint32_t v = (uint32_t)k * 32u + set_ctz(left);
            left &= left - 1u;
            if (!set_has<W>(vis, v) && !nfa_set_eval<W>(t, stack, stride, v, c, vis, nxt)) return 2u;
        }
    }
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < W; k++) { cur[k] = nxt[k]; any |= nxt[k]; }
    return any ? 1u : 0u;
}

template <int W>
__host__ __device__ __forceinline__ void nfa_set_start(const NfaSetView& t, uint32_t (&cur)[W]) {
#pragma unroll
    for (int k = 0; k < W; k++) cur[k] = 0;
    set_put<W>(cur, t.start);
}
// the final pass with the empty letter: `finish` is evaluated iff cur meets the accept mask
template <int W>
__host__ __device__ __forceinline__ uint8_t nfa_set_accepts(const NfaSetView& t, const uint32_t (&cur)[W]) {
    uint32_t hit = 0;
#pragma unroll
    for (int k = 0; k < W; k++) hit |= cur[k] & t.accept[k];
    return hit ? (uint8_t)1 : (uint8_t)0;
}

// One lane, the bytes [b, e) of the batch, scanned upwards or (REV) downwards, from the set in cur: cur becomes the set reached.  Returns 1
// if that set is not empty (also when there was no byte), 0 if it is -- an empty set ends the walk, the reference's `break` -- and 2 on a
// stack overflow (cur is then not to be used).  The input is read in aligned 16-byte blocks, and only blocks that hold a byte of [b, e).
template <bool REV, int W>
__device__ inline uint32_t nfa_set_walk_from(const NfaSetView& t, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t b, uint64_t e,
                                             uint32_t (&cur)[W]) {
    uint64_t p = REV ? e : b;                                         // forward: next byte to consume; reverse: one past it
    while (REV ? p > b : p < e) {
        const uint64_t blk = (REV ? p - 1u : p) & ~(uint64_t)15;
        const uint4 d = *reinterpret_cast<const uint4*>(bytes + blk);
        // the block as two 64-bit halves that are shifted a byte per round: the next byte is always at a fixed place
        uint64_t lo64 = (uint64_t)d.x | (uint64_t)d.y << 32, hi64 = (uint64_t)d.z | (uint64_t)d.w << 32;
        const uint32_t lo = b > blk ? (uint32_t)(b - blk) : 0u, hi = (e - blk) < 16u ? (uint32_t)(e - blk) : 16u;
#pragma unroll 1
        for (uint32_t j = 0; j < 16u; j++) {
            const uint32_t k = REV ? 15u - j : j;
            const uint32_t byte = REV ? (uint32_t)(hi64 >> 56) : (uint32_t)(lo64 & 0xffu);
            if (REV) { hi64 = hi64 << 8 | lo64 >> 56; lo64 <<= 8; }
            else { lo64 = lo64 >> 8 | hi64 << 56; hi64 >>= 8; }
            if (k < lo || k >= hi) continue;
            const uint32_t alive = nfa_set_step<W>(t, stack, stride, cur, t.byte_class[byte]);
            if (alive != 1u) return alive;
        }
        p = REV ? blk : blk + 16u;
    }
    return 1u;
}

// One lane, one string [b, e) of the batch, walked from {start}: its result byte.  A string beyond MFA_MAX_STRING_BYTES is not walked and
// answers 2.
template <bool REV, int W>
__device__ inline uint8_t nfa_set_walk(const NfaSetView& t, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t b, uint64_t e) {
    if (e - b > kSetMaxString) return 2;
    uint32_t cur[W];
    nfa_set_start<W>(t, cur);
    const uint32_t alive = nfa_set_walk_from<REV, W>(t, stack, stride, bytes, b, e, cur);
    if (alive != 1u) return alive == 0u ? (uint8_t)0 : (uint8_t)2;
    return nfa_set_accepts<W>(t, cur);
}

// ---- strings in pieces (mfa_match_batch_resume_set) -----------------------------------------------------------------------------------
// The state of the set walk between two bytes is the set itself, so a string may be cut anywhere and its pieces walked one call after the
// other: a record per string carries the set from call to call.  The record (mfa_set_state, include/mfa_hip.h) is twelve 32-bit words,
// handled as three 16-byte quarters: q0 = tag, reserved[3]; q1 = nodes[0..3]; q2 = nodes[4..7].  Node v is bit v & 31 of nodes[v >> 5].
static constexpr uint32_t kSetStateStart = 0u;                 // MFA_SET_STATE_START: {start}, `nodes` is not looked at
static constexpr uint32_t kSetStateLive = 1u;                  // MFA_SET_STATE_LIVE: `nodes` is the set; the empty set is dead
static constexpr uint32_t kSetStateInvalid = 0xffffffffu;      // MFA_SET_STATE_INVALID: sticky, answered 2
static constexpr uint32_t kSetStateWords = 12u;
static constexpr int kSetStateNodeWords = 8;

// The set a piece of `len` bytes is entered with, unpacked into cur with compile-time indices only (the mask stays in registers): returns
// kSetStateLive, or kSetStateInvalid for a record this image cannot have written -- a tag other than START or LIVE (INVALID among them,
// so an error stays one), a reserved word that is not zero, a bit for a node the image lacks (any word beyond its W among them) -- and
// for a piece beyond the limit.  n_nodes: the header's SET_H_NODES.
template <int W>
__host__ __device__ inline uint32_t nfa_set_state_decode(const NfaSetView& t, uint32_t n_nodes, const uint4& q0, const uint4& q1, const uint4& q2, uint64_t len,
                                                         uint32_t (&cur)[W]) {
    const uint32_t in[kSetStateNodeWords] = {q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    bool ok = (q0.y | q0.z | q0.w) == 0u && len <= kSetMaxString;
    if (q0.x == kSetStateStart) {
        nfa_set_start<W>(t, cur);
    } else {
        ok = ok && q0.x == kSetStateLive;
#pragma unroll
        for (int k = 0; k < W; k++) {
            const uint32_t first = (uint32_t)k * 32u;                // the nodes word k has: first .. min(first + 32, n_nodes)
            const uint32_t have = n_nodes >= first + 32u ? 0xffffffffu : n_nodes > first ? (1u << (n_nodes - first)) - 1u : 0u;
            ok = ok && (in[k] & ~have) == 0u;
            cur[k] = in[k];
        }
#pragma unroll
        for (int k = W; k < kSetStateNodeWords; k++) ok = ok && in[k] == 0u;
    }
    if (ok) return kSetStateLive;
#pragma unroll
    for (int k = 0; k < W; k++) cur[k] = 0;
    return kSetStateInvalid;
}

// the record of a string that has reached cur (tag LIVE), or of one in error (tag INVALID: `nodes` is zero whatever cur holds)
template <int W>
__host__ __device__ inline void nfa_set_state_encode(uint32_t tag, const uint32_t (&cur)[W], uint4& q0, uint4& q1, uint4& q2) {
    uint32_t out[kSetStateNodeWords];
#pragma unroll
    for (int k = 0; k < W; k++) out[k] = tag == kSetStateLive ? cur[k] : 0u;
#pragma unroll
    for (int k = W; k < kSetStateNodeWords; k++) out[k] = 0u;
    q0 = make_uint4(tag, 0u, 0u, 0u);
    q1 = make_uint4(out[0], out[1], out[2], out[3]);
    q2 = make_uint4(out[4], out[5], out[6], out[7]);
}

// the result byte of a string whose record says (tag, cur): what mfa_match_batch answers for the concatenation of the pieces so far
template <int W>
__host__ __device__ __forceinline__ uint8_t nfa_set_state_result(const NfaSetView& t, uint32_t tag, const uint32_t (&cur)[W]) {
    return tag == kSetStateLive ? nfa_set_accepts<W>(t, cur) : (uint8_t)2;      // (the empty set meets no mask: 0)
}

// The piece [b, e) of a string that nfa_set_state_decode has entered with (tag, cur): the record behind the piece goes to q0, q1, q2;
// returns the result byte.  (Apart from nfa_set_resume_piece so that a kernel can look at what the string enters with -- a long piece
// with a live set is handed to nfa_set_split.hip -- without decoding twice.)
template <bool REV, int W>
__device__ inline uint8_t nfa_set_resume_entered(const NfaSetView& t, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t b, uint64_t e, uint32_t tag,
                                                 uint32_t (&cur)[W], uint4& q0, uint4& q1, uint4& q2) {
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < W; k++) any |= cur[k];
    if (tag == kSetStateLive && any != 0u && nfa_set_walk_from<REV, W>(t, stack, stride, bytes, b, e, cur) == 2u) tag = kSetStateInvalid;
    nfa_set_state_encode<W>(tag, cur, q0, q1, q2);
    return nfa_set_state_result<W>(t, tag, cur);
}

// One lane, one piece [b, e) of the batch: the record in q0, q1, q2 is replaced by the one behind the piece; returns the result byte.  A
// string that enters dead (LIVE with the empty set) or in error leaves as it came and its bytes are not read.
template <bool REV, int W>
__device__ inline uint8_t nfa_set_resume_piece(const NfaSetView& t, uint32_t n_nodes, uint32_t* stack, uint32_t stride, const uint8_t* bytes, uint64_t b, uint64_t e,
                                               uint4& q0, uint4& q1, uint4& q2) {
    uint32_t cur[W];
    const uint32_t tag = nfa_set_state_decode<W>(t, n_nodes, q0, q1, q2, e - b, cur);
    return nfa_set_resume_entered<REV, W>(t, stack, stride, bytes, b, e, tag, cur, q0, q1, q2);
}

}  // namespace mfa

#endif
