// TEST INFRASTRUCTURE ONLY: the host-compilable core of the multi-table launch for the memory-less segments of a mixed call
// (csrc/dfa_mixed_core.h and, for the fused table, dfa_fill_table of csrc/dfa_split_core.h: the upload, the fused table, a lane's place in its
// string, the staged line, the walk of a line) run one lane
// at a time over an item list, in the order dfa_mixed_kernel (csrc/dfa_mixed.hip) uses it: slice by slice, the table filled only when
// the automaton changes.
//   dfa_mixed_emul BATCH.bin IMAGE0.blob IMAGE1.blob ...
//   dfa_mixed_emul --eligible STATES        prints "eligible table_bytes" for a memory-less automaton of STATES state sets
//   BATCH.bin: u64 n, u64 n_items, u64 offsets[n + 1], n_items x (u64 first, u64 count, u64 image), then offsets[n] bytes.
//   stdout: "fills F slices S", then one line per string: 0 / 1 / 2, or - for a string no item holds.
#include "emul_common.h"
#include "dfa_mixed_core.h"
#include "walk_plan.h"

using namespace mfa;

template <bool REV>
static uint8_t walk_string(const uint16_t* s_next, const uint8_t* accept_tab, const uint8_t* bytes, uint64_t total16, uint64_t b, uint64_t e) {
    alignas(16) uint8_t row[kMixTileRow];
    MixCursor<REV> c;
    c.start(true, b, e);
    if (c.active) {
        uint64_t line = c.line();
        for (;;) {
            for (uint32_t k = 0; k < kMixLineLanes; k++) {                // the eight lanes that stage this string's line
                const uint4 v = mix_stage16(bytes, line + 16u * k, total16, c.active);
                memcpy(row + 16u * k, &v, 16);
            }
            uint64_t next;
            (void)c.next_line(line, &next);
            uint32_t lo, hi;
            c.bounds(line, &lo, &hi);
            c.st = mix_walk_row<REV>(s_next, row, c.st, lo, hi, c.active && lo == 0u && hi == kMixLine);
            c.advance(line);
            if (!c.active) break;
            if (c.line() != next) { fprintf(stderr, "the line fetched ahead is not the line walked next\n"); exit(4); }
            line = c.line();
        }
    }
    return c.result(accept_tab);
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "--eligible") == 0) {               // dfa_mixed_eligible for a tabulated automaton of this many state sets
        HostImage img;
        img.h.kind = MFA_KIND_NFA;
        img.dfa_states = (uint32_t)strtoul(argv[2], nullptr, 10);
        printf("%d %u\n", dfa_mixed_eligible(img) ? 1 : 0, dfa_mixed_table_bytes(img));
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: dfa_mixed_emul BATCH.bin IMAGE.blob...\n"); return 2; }
    std::vector<HostImage> imgs(argc - 2);
    std::vector<const HostImage*> ptrs;
    std::vector<uint8_t> eligible;
    for (int k = 2; k < argc; k++) {
        HostImage& img = imgs[k - 2];
        emul::load_memoryless(argv[k], img);
        ptrs.push_back(&img);
        eligible.push_back(dfa_mixed_eligible(img) ? 1 : 0);
    }
    const std::vector<uint8_t> tables = dfa_mixed_pack(ptrs, eligible);
    const MixDfaDesc* descs = reinterpret_cast<const MixDfaDesc*>(tables.data());
    const std::vector<uint8_t> batch = emul::slurp(argv[1]);
    uint64_t n, n_items;
    memcpy(&n, batch.data(), 8);
    memcpy(&n_items, batch.data() + 8, 8);
    std::vector<uint64_t> off(n + 1), items(3 * n_items);
    memcpy(off.data(), batch.data() + 16, (n + 1) * 8);
    memcpy(items.data(), batch.data() + 16 + (n + 1) * 8, 3 * n_items * 8);
    const uint64_t total16 = (off[n] + 15u) & ~(uint64_t)15;
    uint8_t* bytes = emul::padded(batch.data() + 16 + (n + 1) * 8 + 3 * n_items * 8, (size_t)off[n]);      // exactly what the contract makes readable
    std::vector<char> out(n, '-');
    std::vector<uint16_t> s_next((kMixLdsMax - kMixTileBytes) / 2u, 0);
    uint64_t fills = 0, slices = 0, held = ~0ull;
    for (uint64_t i = 0; i < n_items; i++) {
        const uint64_t first = items[3 * i], count = items[3 * i + 1], image = items[3 * i + 2];
        if (image >= imgs.size() || !eligible[image] || first + count > n) { fprintf(stderr, "bad item %llu\n", (unsigned long long)i); return 3; }
        const MixDfaDesc d = descs[image];
        for (uint64_t s = 0; s < dfa_slices_of(count); s++, slices++) {
            if (image != held) {
                if ((size_t)d.n_states * kDfaRow > s_next.size()) { fprintf(stderr, "table beyond the LDS\n"); return 3; }
                dfa_fill_table(s_next.data(), reinterpret_cast<const uint16_t*>(tables.data() + d.trans_at), tables.data() + d.class_at, d.n_states, d.n_classes, 0u, 1u);
                held = image; fills++;
            }
            for (uint64_t t = 0; t < kDfaSliceStrings && s * kDfaSliceStrings + t < count; t++) {
                const uint64_t sid = first + s * kDfaSliceStrings + t;
                if (out[sid] != '-') { fprintf(stderr, "string %llu is in two items\n", (unsigned long long)sid); return 3; }
                const uint8_t r = d.reversed ? walk_string<true>(s_next.data(), tables.data() + d.accept_at, bytes, total16, off[sid], off[sid + 1])
                                             : walk_string<false>(s_next.data(), tables.data() + d.accept_at, bytes, total16, off[sid], off[sid + 1]);
                out[sid] = (char)('0' + r);
            }
        }
    }
    printf("fills %llu slices %llu\n", (unsigned long long)fills, (unsigned long long)slices);
    for (uint64_t k = 0; k < n; k++) printf("%c\n", out[k]);
    free(bytes);
    return 0;
}
