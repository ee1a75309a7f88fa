// TEST INFRASTRUCTURE ONLY: the host-compilable core of the split path for long strings of memory-less automata
// (csrc/dfa_split_core.h: chunk geometry, the chunk size, the map of a chunk, the composition of maps) run one lane at a time, in the
// order dfa_plan_kernel, dfa_chunk_kernel and dfa_fold_kernel use it.  Every non-empty string is cut.
//   dfa_split_emul IMAGE.blob BATCH.bin CHUNK_MIN ARENA_CHUNKS TILE_BYTES
//   BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  stdout: "chunk_bytes chunks", then one 0/1 line per string.
#include "emul_common.h"

using namespace mfa;

template <bool REV>
static void run(const HostImage& img, const std::vector<uint16_t>& next, const uint8_t* bytes, const std::vector<uint64_t>& off, uint64_t chunk_min,
                uint64_t arena, uint32_t tile_bytes) {
    const uint64_t n = off.size() - 1;
    uint64_t long_bytes = 0, queued = 0;
    for (uint64_t k = 0; k < n; k++) { long_bytes += off[k + 1] - off[k]; queued += off[k + 1] > off[k]; }
    uint64_t chunk = split_chunk_size(long_bytes, arena, chunk_min), total;
    for (;;) {                                                            // dfa_plan_kernel
        total = 0;
        for (uint64_t k = 0; k < n; k++) total += split_chunks_of(off[k], off[k + 1], chunk);
        if (total <= split_map_capacity(arena, queued)) break;
        fprintf(stderr, "the chosen chunk size overran the arena: %llu chunks of %llu bytes\n", (unsigned long long)total, (unsigned long long)chunk);
        exit(3);
    }
    printf("%llu %llu\n", (unsigned long long)chunk, (unsigned long long)total);
    const uint32_t S = img.dfa_states, ll2 = split_lanes_log2(S), lanes = 1u << ll2, runs = 256u >> ll2, tile_maps = tile_bytes >> ll2;
    std::vector<uint8_t> maps, tile_runs(256);
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = off[k], e = off[k + 1], nc = split_chunks_of(b, e, chunk);
        uint32_t st = 1;
        maps.assign(nc * lanes, 0);
        uint64_t covered = 0, expect = REV ? e : b;
        for (uint64_t c = 0; c < nc; c++) {                               // dfa_chunk_kernel: lane (c, j)
            uint64_t lo, hi;
            split_chunk_range<REV>(b, e, chunk, nc, c, &lo, &hi);
            // the chunks tile the string in scan order, and every border inside the string is 16-byte aligned
            if (lo >= hi || (REV ? hi != expect : lo != expect) || (lo != b && (lo & 15u)) || (hi != e && (hi & 15u))) { fprintf(stderr, "bad chunk %llu of string %llu\n", (unsigned long long)c, (unsigned long long)k); exit(4); }
            expect = REV ? lo : hi; covered += hi - lo;
            for (uint32_t j = 0; j < lanes; j++)
                maps[c * lanes + j] = j + 1u < S ? (uint8_t)(split_chunk_walk<REV>(next.data(), bytes, lo, hi, (j + 1u) * kDfaRow) / kDfaRow) : 0;
        }
        if (covered != e - b) { fprintf(stderr, "string %llu not covered\n", (unsigned long long)k); exit(4); }
        for (uint64_t t0 = 0; t0 < nc; t0 += tile_maps) {                 // dfa_fold_kernel: lane (r, j), then lane 0
            const uint32_t cnt = (uint32_t)(nc - t0 < tile_maps ? nc - t0 : tile_maps), per = split_fold_per(cnt, runs);
            for (uint32_t t = 0; t < 256; t++) {
                const uint32_t r = t >> ll2, j = t & (lanes - 1u);
                const uint32_t m0 = r * per < cnt ? r * per : cnt, m1 = m0 + per < cnt ? m0 + per : cnt;
                tile_runs[t] = (uint8_t)split_fold_run(maps.data() + t0 * lanes, lanes, m0, m1, j + 1u);
            }
            st = split_fold_run(tile_runs.data(), lanes, 0, runs, st);
        }
        printf("%d\n", (int)img.dfa_accept[st]);
    }
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: dfa_split_emul IMAGE.blob BATCH.bin CHUNK_MIN ARENA_CHUNKS TILE_BYTES\n"); return 2; }
    HostImage img;
    emul::load_memoryless(argv[1], img);
    const std::vector<uint16_t> next = emul::fused_table(img);
    const emul::Batch batch = emul::read_batch(emul::slurp(argv[2]));
    const uint64_t chunk_min = strtoull(argv[3], nullptr, 10), arena = strtoull(argv[4], nullptr, 10);
    const uint32_t tile_bytes = (uint32_t)strtoul(argv[5], nullptr, 10);
    if (img.h.is_reversed) run<true>(img, next, batch.bytes, batch.off, chunk_min, arena, tile_bytes);
    else run<false>(img, next, batch.bytes, batch.off, chunk_min, arena, tile_bytes);
    free(batch.bytes);
    return 0;
}
