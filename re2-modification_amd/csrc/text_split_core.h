// The part of the text splitter (text_split.hip: text in device memory -> a batch, bytes back to back and offsets[0..n]) that can be wrong
// without a GPU: which bytes separate, the marks of a 16-byte block, a tile's totals, where a kept byte and a string's offset go, the
// stop-token comparison, the plan of the aligned stores.  Included by the kernels and, with the one-lane shim of tests/emul/, by the
// host harness tests/emul/text_split_emul.cpp.
//
// The rule (include/mfa_hip.h, "text to batch").  MFA_SPLIT_LINES restates std::getline: a string ends at byte 0x0a, which is dropped;
// every other byte is kept; bytes behind the last 0x0a are a last string if there is at least one.  MFA_SPLIT_TOKENS restates
// `cin >> text` in the C locale: separators are 0x09..0x0d and 0x20, a string is a maximal run of other bytes; an optional stop token
// ends the batch in front of the first token equal to it.
//
// Marks.  A byte is KEPT when it is inside the text and no separator.  An EVENT is what fixes one entry of offsets[]:
//   lines:  a 0x0a at p            -> offsets[e + 1] = kept bytes in front of p     (e: events in front of p; the string ENDS here)
//   tokens: a kept byte at p whose predecessor is not kept (or p == 0)
//                                  -> offsets[e]     = kept bytes in front of p     (the string STARTS here)
// What no event fixes is written once per call (split_edges_kernel): offsets[0] = 0 and offsets[n_strings] = n_bytes.
//
// Geometry.  A tile is kSplitTileBytes of text, one workgroup of four waves.  A wave owns 4 KiB of it and reads it as four rows of
// 1 KiB, lane l the 16-byte block l of each row, so that every load instruction of a wave covers 1 KiB of consecutive text; the order of
// the blocks in the text is (wave, row, lane): split_block_of.
#ifndef MFA_TEXT_SPLIT_CORE_H
#define MFA_TEXT_SPLIT_CORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfa {

static constexpr uint32_t kSplitLines = 0u, kSplitTokens = 1u;      // MFA_SPLIT_LINES, MFA_SPLIT_TOKENS
static constexpr uint32_t kSplitThreads = 256u;                     // a workgroup: four waves
static constexpr uint32_t kSplitRows = 4u;                          // 16-byte blocks per lane
static constexpr uint32_t kSplitTileBlocks = kSplitThreads * kSplitRows;
static constexpr uint32_t kSplitTileBytes = kSplitTileBlocks * 16u; // 16 KiB
static constexpr uint32_t kSplitStopMax = 15u;                      // bytes of a stop token
static constexpr uint32_t kSplitNone = 0xffffffffu;                 // SplitTotals: the tile holds no stop token

// what the count pass leaves per tile (16 bytes); stop_events/stop_kept: events and kept bytes of the tile in front of its first stop token
struct SplitTotals { uint32_t kept, events, stop_events, stop_kept; };
// what the scan pass leaves per tile (16 bytes): kept bytes and events of all tiles in front of it
struct SplitPrefix { uint64_t kept, events; };
// the stop token, bytes 0..7 in lo and 8..14 in hi, byte i in bits 8 * (i & 7); len == 0: none
struct SplitStop { uint64_t lo, hi; uint32_t len; };

__host__ __device__ inline uint64_t split_tiles(uint64_t n_text) { return (n_text + kSplitTileBytes - 1u) / kSplitTileBytes; }
// the workspace of a text of n_text bytes: the totals of all tiles, then their prefixes
__host__ __device__ inline uint64_t split_workspace_bytes(uint64_t n_text) {
    const uint64_t t = split_tiles(n_text);
    return (t ? t : 1u) * (sizeof(SplitTotals) + sizeof(SplitPrefix));
}

__host__ __device__ inline bool split_is_sep(uint32_t c, uint32_t mode) {
    return mode == kSplitLines ? c == 0x0au : ((c >= 0x09u && c <= 0x0du) || c == 0x20u);
}

// bit 7 of every byte of w that equals c
__host__ __device__ inline uint32_t split_word_eq(uint32_t w, uint32_t c) {
    const uint32_t t = w ^ (c * 0x01010101u);
    return ~((((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t)) & 0x80808080u;
}
// bit 7 of every byte of w that separates
__host__ __device__ inline uint32_t split_word_seps(uint32_t w, uint32_t mode) {
    if (mode == kSplitLines) return split_word_eq(w, 0x0au);
    const uint32_t low = w & 0x7f7f7f7fu;                                      // seven bits a byte: the sums below stay inside their byte
    const uint32_t ge9 = low + 0x77777777u, ge14 = low + 0x72727272u;          // bit 7: low >= 9, low >= 14
    return ((ge9 & ~ge14) | split_word_eq(low, 0x20u)) & ~w & 0x80808080u;     // (~w: a byte of 0x80 and more separates nothing)
}
// bits 7, 15, 23, 31 of m -> bits 0..3
__host__ __device__ inline uint32_t split_gather4(uint32_t m) { return (((m >> 7) * 0x01020408u) >> 24) & 0xfu; }

// bit i: byte i of the block separates
__host__ __device__ inline uint32_t split_block_seps(uint4 d, uint32_t mode) {
    return split_gather4(split_word_seps(d.x, mode)) | split_gather4(split_word_seps(d.y, mode)) << 4 |
           split_gather4(split_word_seps(d.z, mode)) << 8 | split_gather4(split_word_seps(d.w, mode)) << 12;
}
// bit i: byte i of the block equals c
__host__ __device__ inline uint32_t split_block_eq(uint4 d, uint32_t c) {
    return split_gather4(split_word_eq(d.x, c)) | split_gather4(split_word_eq(d.y, c)) << 4 | split_gather4(split_word_eq(d.z, c)) << 8 |
           split_gather4(split_word_eq(d.w, c)) << 12;
}
// bit i: byte base + i lies inside the text
__host__ __device__ inline uint32_t split_valid(uint64_t base, uint64_t n_text) {
    return base >= n_text ? 0u : (n_text - base >= 16u ? 0xffffu : (1u << (uint32_t)(n_text - base)) - 1u);
}
// the block of a tile that lane `lane` of wave `wave` reads as its row `row`
__host__ __device__ inline uint32_t split_block_of(uint32_t wave, uint32_t row, uint32_t lane) { return wave * 256u + row * 64u + lane; }

struct SplitMarks { uint32_t kept, events; };
// the marks of a block; prev_kept: the byte in front of the block is kept (tokens mode only; 0 at the start of the text)
__host__ __device__ inline SplitMarks split_marks(uint32_t seps, uint32_t valid, uint32_t prev_kept, uint32_t mode) {
    SplitMarks m;
    m.kept = valid & ~seps;
    m.events = mode == kSplitLines ? (valid & seps) : (m.kept & ~((m.kept << 1) | (prev_kept & 1u)));
    return m;
}
// the bits of mask below position i (i may be 16 and more)
__host__ __device__ inline uint32_t split_below(uint32_t mask, uint32_t i) { return i >= 16u ? mask : mask & ((1u << i) - 1u); }
// ... in front of the text position `p`, for a block that starts at `base`
__host__ __device__ inline uint32_t split_before(uint32_t mask, uint64_t base, uint64_t p) {
    return p <= base ? 0u : split_below(mask, p - base >= 16u ? 16u : (uint32_t)(p - base));
}
__host__ __device__ inline uint32_t split_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// which offsets[] entry event e of the text fixes
__host__ __device__ inline uint64_t split_event_index(uint64_t e, uint32_t mode) { return mode == kSplitLines ? e + 1u : e; }

__host__ __device__ inline uint32_t split_stop_byte(const SplitStop& s, uint32_t i) {
    return (uint32_t)((i < 8u ? s.lo >> (8u * i) : s.hi >> (8u * (i - 8u))) & 0xffu);
}
// the token that starts at p is the stop token: its bytes, and the end of the text or a separator behind them
__host__ __device__ inline bool split_stop_at(const uint8_t* text, uint64_t n_text, uint64_t p, const SplitStop& s) {
    if (s.len == 0u || n_text - p < s.len) return false;
    for (uint32_t i = 0; i < s.len; i++)
        if (text[p + i] != split_stop_byte(s, i)) return false;
    return p + s.len == n_text || split_is_sep(text[p + s.len], kSplitTokens);
}
// the stop token of a call: false for what the ABI refuses (empty, longer than kSplitStopMax, a separator inside); token == nullptr: none
inline bool split_stop_pack(const char* token, SplitStop* out) {
    *out = SplitStop{0, 0, 0};
    if (!token) return true;
    uint32_t len = 0;
    while (token[len]) {
        const uint32_t c = (uint8_t)token[len];
        if (len >= kSplitStopMax || split_is_sep(c, kSplitTokens)) return false;
        if (len < 8u) out->lo |= (uint64_t)c << (8u * len); else out->hi |= (uint64_t)c << (8u * (len - 8u));
        len++;
    }
    out->len = len;
    return len != 0u;
}

// What the scan pass makes of the totals: strings and kept bytes of the whole text.  events/kept: the sums over all tiles;
// last_byte_kept: the text's last byte is no separator (n_text > 0)
__host__ __device__ inline uint64_t split_string_count(uint64_t events, uint32_t mode, bool last_byte_kept) {
    return mode == kSplitLines ? events + (last_byte_kept ? 1u : 0u) : events;
}

// The stores of `count` staged bytes to the address `dst` (dst & 15 == skew): the staging area holds byte i at index skew + i, so an
// aligned 16-byte piece of the destination is an aligned piece of the staging area.  [skew, head_end) and [tail_begin, skew + count)
// go byte by byte, [head_end, tail_begin) in 16-byte vectors; all three may be empty.
struct SplitStorePlan { uint32_t head_end, tail_begin, end; };
__host__ __device__ inline SplitStorePlan split_store_plan(uint32_t skew, uint32_t count) {
    SplitStorePlan p;
    p.end = skew + count;
    const uint32_t up = (skew + 15u) & ~15u, down = p.end & ~15u;
    p.head_end = up < p.end ? up : p.end;
    p.tail_begin = down > p.head_end ? down : p.head_end;
    return p;
}

// how much of a tile's kept bytes (or events) a limit leaves: the tile's start is `prefix`, it holds `have`
__host__ __device__ inline uint32_t split_clip(uint64_t prefix, uint32_t have, uint64_t limit) {
    return prefix >= limit ? 0u : (limit - prefix < have ? (uint32_t)(limit - prefix) : have);
}

}  // namespace mfa

#endif
