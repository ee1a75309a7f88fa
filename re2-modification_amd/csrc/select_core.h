// The part of the selection (select.hip: a batch and its result bytes -> the kept strings, compacted, as a batch or as a text) that can be
// wrong without a GPU: which strings are kept, what a kept string adds to the output, the layout of the workspace, the geometry of an
// output tile, the searches in the blocks' prefixes and the output offsets, a run of output from aligned source blocks, a chunk's stores.
// Included by the kernels and, with the one-lane shim of tests/emul/, by the host harness tests/emul/select_emul.cpp.
//
// The rule (include/mfa_hip.h, "batch to text").  String k is KEPT when results[k] == 1, or == 0 under MFA_SELECT_INVERT; any other
// value is UNANSWERED and never kept.  A kept string of len bytes adds len bytes to the output, plus one 0x0a under MFA_SELECT_NEWLINE.
// The r-th kept string (its RANK) starts at out_offsets[r]; out_indices[r] is its index k.
//
// Geometry.  The strings go in BLOCKS of kSelectBlock: one workgroup, lane t the strings 4t .. 4t+3 of the block.  The output goes in
// TILES of kSelectTileBytes, cut along the 16-byte lines of the destination's memory: with skew = d_out_bytes & 15, tile t holds the
// output positions [16384 t - skew, 16384 (t + 1) - skew), so that every 16-byte CHUNK of a tile is one aligned line of memory and only
// the first chunk of tile 0 and the last chunk of the output can be partial.  The lanes of the workgroup FILL the staging area, by
// strings or by runs of four chunks (select_by_strings), and, behind a barrier, lane t STORES the chunks t, t + 256, ..., so that a store
// instruction of a wave covers 1 KiB of consecutive memory.
#ifndef MFA_SELECT_CORE_H
#define MFA_SELECT_CORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfa {

static constexpr uint32_t kSelectInvert = 1u, kSelectNewline = 2u;      // MFA_SELECT_INVERT, MFA_SELECT_NEWLINE
static constexpr uint32_t kSelectThreads = 256u;                        // a workgroup: four waves
static constexpr uint32_t kSelectPerLane = 4u;                          // strings per lane (count, place); chunks per lane (gather)
static constexpr uint32_t kSelectBlock = kSelectThreads * kSelectPerLane;      // 1024 strings
static constexpr uint32_t kSelectTileBytes = kSelectBlock * 16u;        // 16 KiB of output
static constexpr uint64_t kSelectMaxStrings = 1ull << 40;               // n of a call stays below it
static constexpr uint64_t kSelectMaxCapacity = 1ull << 44;              // the gather grid covers no more output than this (no device holds it)

// what the count pass leaves per block (16 bytes): output bytes of its kept strings, kept strings, unanswered strings
struct SelectTotals { uint64_t bytes; uint32_t kept, unanswered; };
// what the scan pass leaves per block and once behind the last (16 bytes): output bytes and kept strings of all blocks in front
struct SelectPrefix { uint64_t bytes, kept; };

__host__ __device__ inline uint64_t select_blocks(uint64_t n) { return (n + kSelectBlock - 1u) / kSelectBlock; }
// The workspace of n strings: totals[blocks], prefix[blocks + 1], then per block the list of its kept strings, list[j] the position
// inside the block of its j-th kept string (16 bits each; the count pass writes it, the gather pass maps a rank to a string with it).
__host__ __device__ inline uint64_t select_prefix_at(uint64_t blocks) { return blocks * sizeof(SelectTotals); }
__host__ __device__ inline uint64_t select_list_at(uint64_t blocks) { return select_prefix_at(blocks) + (blocks + 1u) * sizeof(SelectPrefix); }
__host__ __device__ inline uint64_t select_workspace_bytes(uint64_t n) {
    const uint64_t b = select_blocks(n);
    return select_list_at(b) + b * kSelectBlock * sizeof(uint16_t);
}

__host__ __device__ inline bool select_kept(uint32_t result, uint32_t flags) { return result == ((flags & kSelectInvert) ? 0u : 1u); }
__host__ __device__ inline bool select_unanswered(uint32_t result) { return result > 1u; }
__host__ __device__ inline uint64_t select_out_len(bool kept, uint64_t len, uint32_t flags) {
    return kept ? len + ((flags & kSelectNewline) ? 1u : 0u) : 0u;
}

// (what a call's limits leave is two of these: v = min(n_selected, max_selected) ranks, min(out_offsets[v], bytes_capacity) bytes)
__host__ __device__ inline uint64_t select_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// The largest i in [lo, hi] with a[i * stride] <= x; the caller knows a[lo * stride] <= x.  a ascends (equal neighbours allowed).
__host__ __device__ inline uint64_t select_last_le(const uint64_t* a, uint32_t stride, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1u) / 2u;
        if (a[mid * stride] <= x) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// ---- a tile of the output ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t select_tiles(uint64_t limit, uint32_t skew) { return (limit + skew + kSelectTileBytes - 1u) / kSelectTileBytes; }

// Tile `tile` in LINE SPACE: position x of it is the output byte x - skew, and byte x - line0 of the staging area.  [begin, end) is what
// of the tile lies inside the output [0, limit); empty when end <= begin.
struct SelectTile { uint64_t line0, begin, end; };
__host__ __device__ inline SelectTile select_tile(uint64_t tile, uint32_t skew, uint64_t limit) {
    SelectTile t;
    t.line0 = tile * kSelectTileBytes;
    t.begin = t.line0 > skew ? t.line0 : skew;
    t.end = select_min(t.line0 + kSelectTileBytes, limit + skew);
    return t;
}
// chunk c of the tile: [begin, end) in line space, clipped to the tile's part of the output
struct SelectChunk { uint64_t begin, end; };
__host__ __device__ inline SelectChunk select_chunk(const SelectTile& t, uint32_t c) {
    SelectChunk k;
    k.begin = t.line0 + 16u * c > t.begin ? t.line0 + 16u * c : t.begin;
    k.end = select_min(t.line0 + 16u * c + 16u, t.end);
    return k;
}

// the 32 bytes (a, b) from byte `sh` on (sh: 0..15): sixteen of them.  Selects only: no array is indexed by sh.
__host__ __device__ inline uint32_t select_align(uint32_t lo, uint32_t hi, uint32_t bits) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
}
__host__ __device__ inline uint4 select_shift(uint4 a, uint4 b, uint32_t sh) {
    uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
    if (sh & 4u) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6; w6 = w7; }
    if (sh & 8u) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; }
    const uint32_t bits = (sh & 3u) * 8u;
    return make_uint4(select_align(w0, w1, bits), select_align(w1, w2, bits), select_align(w2, w3, bits), select_align(w3, w4, bits));
}

// ---- a search by the whole workgroup ---------------------------------------------------------------------------------------------------
// select_last_le in rounds of kSelectThreads probes: in a round lane t looks at lo + (t + 1) * step, the lanes whose probe is <= x are
// counted (they are the first `count` lanes, since a ascends), and the range shrinks to the step behind the last of them.  The kernel
// does the probes with one load per lane and one barrier per round; the harness does them in a loop.
__host__ __device__ inline uint64_t select_search_step(uint64_t lo, uint64_t hi) { return (hi - lo) / kSelectThreads + 1u; }
__host__ __device__ inline bool select_search_probe(const uint64_t* a, uint32_t stride, uint64_t lo, uint64_t hi, uint64_t step, uint32_t t, uint64_t x) {
    const uint64_t p = lo + (uint64_t)(t + 1u) * step;
    return p <= hi && a[p * stride] <= x;
}
__host__ __device__ inline void select_search_narrow(uint64_t& lo, uint64_t& hi, uint64_t step, uint32_t count) {
    lo += (uint64_t)count * step;
    hi = select_min(hi, lo + step - 1u);
}

// The kept strings that reach into a tile: their ranks [r_lo, r_hi] and the blocks of strings [b_lo, b_hi] they come from.  The four
// searches, each given by its array, its bounds and its key, in the order the kernel makes them; search k needs the results of those
// in front of it.  prefix: [0 .. n_blocks]; v = min(n_selected, max_selected); [first, last]: the tile's output positions.
struct SelectReach { uint64_t b_lo, b_hi, r_lo, r_hi; };
struct SelectSearch { const uint64_t* a; uint32_t stride; uint64_t lo, hi, x; };
__host__ __device__ inline SelectSearch select_reach_search(uint32_t which, const SelectReach& got, const SelectPrefix* prefix, uint64_t n_blocks,
                                                            const uint64_t* out_offsets, uint64_t v, uint64_t first, uint64_t last) {
    switch (which) {
    case 0: return SelectSearch{&prefix[0].bytes, 2u, 0u, n_blocks, first};                 // the block that holds the tile's first byte
    case 1: return SelectSearch{&prefix[0].bytes, 2u, got.b_lo, n_blocks, last};            // ... its last byte
    case 2: return SelectSearch{out_offsets, 1u, prefix[got.b_lo].kept, select_min(prefix[got.b_lo + 1u].kept, v) - 1u, first};
    default: {
        const uint64_t from = prefix[got.b_hi].kept;
        return SelectSearch{out_offsets, 1u, from > got.r_lo ? from : got.r_lo, select_min(prefix[got.b_hi + 1u].kept, v) - 1u, last};
    }
    }
}
__host__ __device__ inline void select_reach_set(uint32_t which, SelectReach& got, uint64_t value) {
    if (which == 0) got.b_lo = value; else if (which == 1) got.b_hi = value; else if (which == 2) got.r_lo = value; else got.r_hi = value;
}

// what the gather pass reads besides the staging area
struct SelectSource {
    const uint8_t* bytes;             // d_bytes
    const uint64_t* offsets;          // d_offsets
    const uint64_t* out_offsets;      // d_out_offsets, written by the place pass: [0 .. v]
    const uint64_t* out_indices;      // d_out_indices, written by the place pass: [0 .. v), or nullptr
    const SelectPrefix* prefix;       // of the blocks of strings: [0 .. blocks]
    const uint16_t* list;             // the kept strings of every block
    uint32_t newline;                 // 1 under MFA_SELECT_NEWLINE
};

// the string of rank r: from the indices where the caller asked for them, else from the block's list; b: the block of the rank this lane
// looked up last (it only moves forward), b_hi: the last block of the tile
__host__ __device__ inline uint64_t select_string_of(const SelectSource& s, uint64_t& b, uint64_t b_hi, uint64_t r) {
    if (s.out_indices) return s.out_indices[r];
    if (s.prefix[b + 1u].kept <= r) b = select_last_le(&s.prefix[0].kept, 2u, b + 1u, b_hi, r);
    return b * kSelectBlock + s.list[b * kSelectBlock + (r - s.prefix[b].kept)];
}

// The source blocks a lane has loaded last: the second block of one piece is the first of the next
struct SelectHave { uintptr_t at; uint4 block; };

// Stages what of the string of rank r lies in the output positions [from, stop): into s_out (the tile from line0 on, 16-byte aligned).
// The output is taken in PIECES that end where the string ends or a 16-byte line of the destination does: a piece's source bytes come
// in one or two aligned 16-byte blocks, none of which lies outside the string's own bytes; a piece that is a whole line is staged as one
// vector, anything shorter byte by byte; the 0x0a behind the string is a byte store of its own.  Returns where the string ends.
__host__ __device__ inline uint64_t select_fill_string(const SelectSource& s, uint8_t* s_out, const SelectTile& t, uint32_t skew, uint64_t r, uint64_t from,
                                                       uint64_t stop, uint64_t& b, uint64_t b_hi, SelectHave& have) {
    const uint64_t begin_r = s.out_offsets[r], end_r = s.out_offsets[r + 1u], data_end = end_r - s.newline;
    const uint64_t stop_r = select_min(stop, end_r);
    uint64_t at = from > begin_r ? from : begin_r;
    uintptr_t src = 0;
    if (at < stop_r && at < data_end) src = reinterpret_cast<uintptr_t>(s.bytes) + s.offsets[select_string_of(s, b, b_hi, r)] + (at - begin_r);
    while (at < stop_r) {
        const uint64_t line_end = ((at + skew) | 15u) + 1u - skew;
        const uint32_t take = (uint32_t)(select_min(stop_r, line_end) - at);
        uint8_t* const to = s_out + (at + skew - t.line0);
        if (at < data_end) {
            const uint32_t n_data = (uint32_t)(select_min(at + take, data_end) - at);
            const uint32_t sh = (uint32_t)(src & 15u);
            const uintptr_t line = src - sh;
            const uint4 a = line == have.at ? have.block : *reinterpret_cast<const uint4*>(line);
            uint4 c = make_uint4(0, 0, 0, 0);
            have.block = a;
            have.at = line;
            if (sh + n_data > 16u) {
                c = *reinterpret_cast<const uint4*>(line + 16u);
                have.block = c;
                have.at = line + 16u;
            }
            const uint4 d = select_shift(a, c, sh);
            if (take == 16u) {
                *reinterpret_cast<uint4*>(to) = d;        // (a whole line of the staging area)
            } else {
                const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (uint32_t i = 0; i < 15u; i++)
                    if (i < n_data) to[i] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
            }
            src += take;
        }
        if (s.newline && at + take == end_r) to[take - 1u] = 0x0au;
        at += take;
    }
    return end_r;
}

// How a tile's work goes to the lanes.  A tile that more strings reach into than the workgroup has lanes is filled BY STRINGS: lane t
// stages the strings of rank r_lo + t, r_lo + t + 256, ... whole (as far as they lie in the tile), so that the lanes of a wave read
// neighbouring offsets, indices and source bytes.  Any other tile is filled BY RUNS: lane t stages the chunks 4t .. 4t + 3, one run of
// output, looking its first string up by binary search among the tile's and walking on from there; a long string is spread over the
// lanes it covers.
__host__ __device__ inline bool select_by_strings(const SelectReach& reach) { return reach.r_hi - reach.r_lo >= kSelectThreads; }

__host__ __device__ inline void select_fill_strings(const SelectSource& s, uint8_t* s_out, const SelectTile& t, uint32_t skew, const SelectReach& reach, uint32_t lane) {
    uint64_t b = reach.b_lo;
    SelectHave have{0, make_uint4(0, 0, 0, 0)};
    for (uint64_t r = reach.r_lo + lane; r <= reach.r_hi; r += kSelectThreads)
        (void)select_fill_string(s, s_out, t, skew, r, t.begin - skew, t.end - skew, b, reach.b_hi, have);
}

// [begin, end): the lane's run in line space
__host__ __device__ inline void select_fill_run(const SelectSource& s, uint8_t* s_out, const SelectTile& t, uint64_t begin, uint64_t end, uint32_t skew,
                                                const SelectReach& reach) {
    if (end <= begin) return;
    uint64_t at = begin - skew;                           // output positions from here on
    const uint64_t stop = end - skew;
    uint64_t r = select_last_le(s.out_offsets, 1u, reach.r_lo, reach.r_hi, at), b = reach.b_lo;
    SelectHave have{0, make_uint4(0, 0, 0, 0)};
    while (at < stop) {
        if (s.out_offsets[r + 1u] <= at) r = select_last_le(s.out_offsets, 1u, r + 1u, reach.r_hi, at);      // the string that holds `at`, behind any empty ones
        at = select_fill_string(s, s_out, t, skew, r, at, stop, b, reach.b_hi, have);
        r++;
    }
}

// The stores of a chunk: a whole one leaves as one aligned 16-byte vector, a partial one (the first of the output on a destination that
// is off its line, the last of the output) byte by byte.  dst_line: the 16-byte aligned address of the tile's position line0.
__host__ __device__ inline void select_store_chunk(const uint8_t* s_out, uint8_t* dst_line, const SelectTile& t, SelectChunk ch) {
    if (ch.end <= ch.begin) return;
    const uint64_t x = ch.begin - t.line0;
    if (ch.end - ch.begin == 16u) {
        *reinterpret_cast<uint4*>(dst_line + x) = *reinterpret_cast<const uint4*>(s_out + x);
    } else {
        for (uint64_t i = x; i < ch.end - t.line0; i++) dst_line[i] = s_out[i];
    }
}

}  // namespace mfa

#endif
