// TEST INFRASTRUCTURE ONLY: the host-compilable core of the text splitter (csrc/text_split_core.h: separator masks, marks, totals, write
// positions, the stop-token comparison, the store plan) run block by block in the order the kernels of csrc/text_split.hip give the
// blocks to their lanes: the count pass tile by tile, the scan over the tiles' totals, the write pass tile by tile through a staging
// area of the tile's size, then the longest string.
//   text_split_emul CASES.bin > OUT.bin
//       CASES.bin: u32 count, then per case  u32 mode, u32 stop_len, 16 bytes stop token, u64 max_strings, u64 bytes_capacity,
//                  u64 n_text, n_text bytes.
//       OUT.bin:   per case  the 32 bytes of mfa_split_info, u64 v = min(n_strings, max_strings), offsets[0..v] as u64, then
//                  min(offsets[v], bytes_capacity) bytes.
//       The text lies in exactly the room the read rule makes readable, d_bytes and d_offsets in exactly their capacities, so that a
//       host sanitizer sees every access beyond them.
#include <string>

#include "emul_common.h"
#include "mfa_hip.h"
#include "text_split_core.h"

using namespace mfa;

struct Case {
    uint32_t mode;
    SplitStop stop;
    uint64_t max_strings, capacity, n;
    uint8_t* text;      // emul::padded
};

static uint4 load16(const uint8_t* p) { uint4 d; memcpy(&d, p, 16); return d; }

// the marks of block `b` of tile `tile`, as lane_marks (text_split.hip) makes them
static SplitMarks block_marks(const Case& c, uint64_t tile, uint32_t b, uint4* d) {
    const uint64_t base = tile * kSplitTileBytes + (uint64_t)b * 16u;
    const uint32_t valid = split_valid(base, c.n);
    *d = valid ? load16(c.text + base) : make_uint4(0, 0, 0, 0);
    const uint32_t seps = split_block_seps(*d, c.mode);
    for (uint32_t i = 0; i < 16; i++)      // the word-wise classification against the byte-wise one
        if ((valid >> i & 1u) && (seps >> i & 1u) != (split_is_sep(c.text[base + i], c.mode) ? 1u : 0u)) { fprintf(stderr, "separator mask differs at %llu\n", (unsigned long long)(base + i)); exit(5); }
    const uint32_t prev = (c.mode == kSplitTokens && valid && base) ? (split_is_sep(c.text[base - 1], c.mode) ? 0u : 1u) : 0u;
    return split_marks(seps, valid, prev, c.mode);
}

template <class F>
static void for_blocks(F f) {
    uint32_t expect = 0;
    for (uint32_t wave = 0; wave < kSplitThreads / 64u; wave++)
        for (uint32_t row = 0; row < kSplitRows; row++)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const uint32_t b = split_block_of(wave, row, lane);
                if (b != expect++) { fprintf(stderr, "blocks out of order\n"); exit(5); }
                f(b);
            }
}

static void run_case(const Case& c, FILE* out) {
    const uint64_t tiles = split_tiles(c.n);
    std::vector<uint8_t> workspace(split_workspace_bytes(c.n));
    SplitTotals* totals = reinterpret_cast<SplitTotals*>(workspace.data());
    SplitPrefix* prefix = reinterpret_cast<SplitPrefix*>(totals + tiles);
    mfa_split_info info{};

    // count
    for (uint64_t tile = 0; tile < tiles; tile++) {
        SplitTotals t{0, 0, kSplitNone, 0};
        for_blocks([&](uint32_t b) {
            uint4 d;
            const SplitMarks m = block_marks(c, tile, b, &d);
            const uint64_t base = tile * kSplitTileBytes + (uint64_t)b * 16u;
            if (c.mode == kSplitTokens && c.stop.len && t.stop_events == kSplitNone) {
                uint32_t cand = m.events & split_block_eq(d, split_stop_byte(c.stop, 0));
                for (; cand; cand &= cand - 1u) {
                    const uint32_t i = (uint32_t)__builtin_ctz(cand);
                    if (split_stop_at(c.text, c.n, base + i, c.stop)) {
                        t.stop_events = t.events + split_popc(split_before(m.events, base, base + i));
                        t.stop_kept = t.kept + split_popc(split_before(m.kept, base, base + i));
                        break;
                    }
                }
            }
            t.kept += split_popc(m.kept);
            t.events += split_popc(m.events);
        });
        totals[tile] = t;
    }
    // scan
    if (tiles) {
        uint64_t kept = 0, events = 0;
        bool stopped = false;
        for (uint64_t tile = 0; tile < tiles; tile++) {
            prefix[tile] = SplitPrefix{kept, events};
            if (totals[tile].stop_events != kSplitNone && !stopped) {
                stopped = true;
                info.n_strings = events + totals[tile].stop_events;
                info.n_bytes = kept + totals[tile].stop_kept;
            }
            kept += totals[tile].kept;
            events += totals[tile].events;
        }
        if (!stopped) {
            info.n_strings = split_string_count(events, c.mode, c.n != 0 && !split_is_sep(c.text[c.n - 1], c.mode));
            info.n_bytes = kept;
        }
        info.stopped = stopped ? 1u : 0u;
    }
    // write: the edges, the tiles, the longest string
    uint8_t* d_bytes = (uint8_t*)malloc(c.capacity ? c.capacity : 1);
    uint64_t* d_offsets = (uint64_t*)malloc((c.max_strings + 1) * 8);
    memset(d_bytes, 0x5a, c.capacity ? c.capacity : 1);
    memset(d_offsets, 0x5a, (c.max_strings + 1) * 8);
    d_offsets[0] = 0;
    if (info.n_strings <= c.max_strings) d_offsets[info.n_strings] = info.n_bytes;
    info.overflow = (info.n_strings > c.max_strings || info.n_bytes > c.capacity) ? 1u : 0u;
    const uint64_t limit_bytes = info.n_bytes < c.capacity ? info.n_bytes : c.capacity;
    const uint64_t limit_index = info.n_strings < c.max_strings ? info.n_strings : c.max_strings;
    uint8_t* s_out = (uint8_t*)aligned_alloc(16, kSplitTileBytes + 16);
    for (uint64_t tile = 0; tile < tiles; tile++) {
        const SplitPrefix pre = prefix[tile];
        const uint32_t avail = split_clip(pre.kept, totals[tile].kept, limit_bytes);
        if (avail == 0u && split_event_index(pre.events, c.mode) > limit_index) continue;
        const uintptr_t dst = reinterpret_cast<uintptr_t>(d_bytes) + pre.kept;
        const uint32_t skew = (uint32_t)(dst & 15u);
        uint32_t kept_at = 0, events_at = 0;
        for_blocks([&](uint32_t b) {
            uint4 d;
            const SplitMarks m = block_marks(c, tile, b, &d);
            uint8_t raw[16];
            memcpy(raw, &d, 16);
            uint32_t to = skew + kept_at;
            for (uint32_t i = 0; i < 16; i++)
                if (m.kept >> i & 1u) s_out[to++] = raw[i];
            for (uint32_t ev = m.events; ev; ev &= ev - 1u) {
                const uint32_t i = (uint32_t)__builtin_ctz(ev);
                const uint64_t index = split_event_index(pre.events + events_at + split_popc(split_below(m.events, i)), c.mode);
                if (index <= limit_index) d_offsets[index] = pre.kept + kept_at + split_popc(split_below(m.kept, i));
            }
            kept_at += split_popc(m.kept);
            events_at += split_popc(m.events);
        });
        if (kept_at != totals[tile].kept || events_at != totals[tile].events) { fprintf(stderr, "the passes disagree on tile %llu\n", (unsigned long long)tile); exit(5); }
        const SplitStorePlan plan = split_store_plan(skew, avail);
        uint8_t* const dst_line = d_bytes + pre.kept - skew;      // (never touched below index skew)
        for (uint32_t x = skew; x < plan.head_end; x++) dst_line[x] = s_out[x];
        for (uint32_t x = plan.head_end; x < plan.tail_begin; x += 16) {
            if (((reinterpret_cast<uintptr_t>(dst_line) + x) & 15u) || x + 16 > plan.tail_begin) { fprintf(stderr, "a vector store off its line\n"); exit(5); }
            memcpy(dst_line + x, s_out + x, 16);
        }
        for (uint32_t x = plan.tail_begin; x < plan.end; x++) dst_line[x] = s_out[x];
        if (plan.head_end - skew > 15u || plan.end - plan.tail_begin > 15u) { fprintf(stderr, "head or tail of 16 bytes or more\n"); exit(5); }
    }
    free(s_out);
    for (uint64_t k = 0; k < limit_index; k++)
        if (d_offsets[k + 1] - d_offsets[k] > info.max_string_bytes) info.max_string_bytes = d_offsets[k + 1] - d_offsets[k];

    fwrite(&info, sizeof info, 1, out);
    fwrite(&limit_index, 8, 1, out);
    fwrite(d_offsets, 8, limit_index + 1, out);
    const uint64_t n_out = d_offsets[limit_index] < c.capacity ? d_offsets[limit_index] : c.capacity;
    fwrite(d_bytes, 1, n_out, out);
    free(d_bytes);
    free(d_offsets);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: text_split_emul CASES.bin > OUT.bin\n"); return 2; }
    const std::vector<uint8_t> file = emul::slurp(argv[1]);
    const uint8_t* p = file.data();
    uint32_t count;
    memcpy(&count, p, 4); p += 4;
    for (uint32_t k = 0; k < count; k++) {
        Case c;
        uint32_t stop_len;
        char token[17] = {0};
        memcpy(&c.mode, p, 4); memcpy(&stop_len, p + 4, 4); memcpy(token, p + 8, 16);
        memcpy(&c.max_strings, p + 24, 8); memcpy(&c.capacity, p + 32, 8); memcpy(&c.n, p + 40, 8);
        p += 48;
        token[stop_len < 16 ? stop_len : 16] = 0;
        if (!split_stop_pack(stop_len ? token : nullptr, &c.stop) || c.mode > kSplitTokens || (stop_len && c.mode != kSplitTokens)) { fprintf(stderr, "case %u: refused\n", k); return 3; }
        c.text = emul::padded(p, c.n);
        p += c.n;
        run_case(c, stdout);
        free(c.text);
    }
    return 0;
}
