// TEST INFRASTRUCTURE ONLY: the host-compilable core of the resume path for memory-less automata (csrc/dfa_resume_core.h: the state a
// piece is entered with, the error state, the walk of a piece from a given state, the answer of a state) run one lane at a time, as
// the resume instantiations of the kernels (kernels.hip, dfa_spec.hip) and of dfa_fold_kernel use it.
//   dfa_resume_emul pieces IMAGE.blob ROUNDS.bin lds|big
//       ROUNDS.bin: u64 n, u64 rounds, u32 state_in[n], rounds * n pairs (u64 b, u64 e) -- the piece of string k in round r, in place
//       in the buffer --, u64 total, then `total` bytes.  stdout: one line per round, "state:result" per string.
//   dfa_resume_emul fold IMAGE.blob BATCH.bin CHUNK TILE_BYTES
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  Every string is cut into chunks of CHUNK bytes, the chunks' maps
//       are composed as dfa_fold_kernel<RESUME> composes them FROM EVERY START STATE, and the state reached is compared with a plain walk of the
//       image's table from that state (and with resume_piece).  stdout: "ok STATES CHECKS"; a difference is exit code 5.
#include <string>

#include "emul_common.h"
#include "dfa_resume_core.h"

using namespace mfa;

// the walk nobody shares: the image's table, byte by byte
template <bool REV>
static uint32_t plain_walk(const HostImage& img, const uint8_t* bytes, uint64_t b, uint64_t e, uint32_t st) {
    for (uint64_t i = 0; i < e - b; i++) st = img.dfa_trans[(size_t)st * img.n_classes + img.byte_class[bytes[REV ? e - 1u - i : b + i]]];
    return st;
}

template <bool REV>
static int run_pieces(const HostImage& img, const std::vector<uint16_t>& next, const std::vector<uint8_t>& in, bool big) {
    uint64_t n, rounds;
    memcpy(&n, in.data(), 8); memcpy(&rounds, in.data() + 8, 8);
    std::vector<uint32_t> st(n);
    memcpy(st.data(), in.data() + 16, n * 4);
    const uint8_t* pairs = in.data() + 16 + n * 4;
    uint64_t total;
    memcpy(&total, pairs + rounds * n * 16, 8);
    uint8_t* bytes = emul::padded(pairs + rounds * n * 16 + 8, total);
    for (uint64_t r = 0; r < rounds; r++) {
        for (uint64_t k = 0; k < n; k++) {
            uint64_t b, e;
            memcpy(&b, pairs + (r * n + k) * 16, 8); memcpy(&e, pairs + (r * n + k) * 16 + 8, 8);
            uint32_t s = resume_enter(st[k], img.dfa_states, e - b);
            if (resume_walks(s))
                s = big ? resume_piece_big<REV, uint32_t>(img.dfa_trans.data(), img.byte_class, img.n_classes, bytes, b, e, s)
                        : resume_piece<REV>(next.data(), bytes, b, e, s);
            st[k] = s;
            printf("%u:%d%c", s, (int)resume_result(img.dfa_accept.data(), s), k + 1 == n ? '\n' : ' ');
        }
        if (n == 0) printf("\n");
    }
    free(bytes);
    return 0;
}

template <bool REV>
static int run_fold(const HostImage& img, const std::vector<uint16_t>& next, const std::vector<uint8_t>& file, uint64_t chunk, uint32_t tile_bytes) {
    const emul::Batch batch = emul::read_batch(file);
    const std::vector<uint64_t>& off = batch.off;
    const uint8_t* bytes = batch.bytes;
    const uint64_t n = off.size() - 1;
    const uint32_t S = img.dfa_states, ll2 = split_lanes_log2(S), lanes = 1u << ll2, runs = 256u >> ll2, tile_maps = tile_bytes >> ll2;
    std::vector<uint8_t> maps, tile_runs(256);
    uint64_t checks = 0;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = off[k], e = off[k + 1], nc = split_chunks_of(b, e, chunk);
        maps.assign(nc * lanes, 0);
        for (uint64_t c = 0; c < nc; c++) {                               // dfa_chunk_kernel: lane (c, j)
            uint64_t lo, hi;
            split_chunk_range<REV>(b, e, chunk, nc, c, &lo, &hi);
            for (uint32_t j = 0; j < lanes; j++)
                maps[c * lanes + j] = j + 1u < S ? (uint8_t)(split_chunk_walk<REV>(next.data(), bytes, lo, hi, (j + 1u) * kDfaRow) / kDfaRow) : 0;
        }
        for (uint32_t s_in = 0; s_in < S; s_in++) {                       // dfa_fold_kernel<RESUME>: lane (r, j), then lane 0, from s_in
            uint32_t st = s_in;
            for (uint64_t t0 = 0; t0 < nc; t0 += tile_maps) {
                const uint32_t cnt = (uint32_t)(nc - t0 < tile_maps ? nc - t0 : tile_maps), per = split_fold_per(cnt, runs);
                for (uint32_t t = 0; t < 256; t++) {
                    const uint32_t r = t >> ll2, j = t & (lanes - 1u);
                    const uint32_t m0 = r * per < cnt ? r * per : cnt, m1 = m0 + per < cnt ? m0 + per : cnt;
                    tile_runs[t] = (uint8_t)split_fold_run(maps.data() + t0 * lanes, lanes, m0, m1, j + 1u);
                }
                st = split_fold_run(tile_runs.data(), lanes, 0, runs, st);
            }
            const uint32_t want = plain_walk<REV>(img, bytes, b, e, s_in);
            const uint32_t piece = s_in ? resume_piece<REV>(next.data(), bytes, b, e, s_in) : 0u;
            if (st != want || piece != want) {
                fprintf(stderr, "string %llu from state %u: fold %u, piece %u, plain walk %u\n", (unsigned long long)k, s_in, st, piece, want);
                return 5;
            }
            checks++;
        }
    }
    printf("ok %u %llu\n", S, (unsigned long long)checks);
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: dfa_resume_emul pieces IMAGE.blob ROUNDS.bin lds|big  |  fold IMAGE.blob BATCH.bin CHUNK TILE_BYTES\n"); return 2; }
    const std::string mode = argv[1];
    HostImage img;
    emul::load_memoryless(argv[2], img);
    const std::vector<uint8_t> in = emul::slurp(argv[3]);
    const bool big = mode == "pieces" && std::string(argv[4]) == "big";
    const std::vector<uint16_t> next = big ? std::vector<uint16_t>() : emul::fused_table(img);
    if (mode == "pieces") return img.h.is_reversed ? run_pieces<true>(img, next, in, big) : run_pieces<false>(img, next, in, big);
    if (mode == "fold" && argc >= 6) {
        const uint64_t chunk = strtoull(argv[4], nullptr, 10);
        const uint32_t tile = (uint32_t)strtoul(argv[5], nullptr, 10);
        if (chunk < 16 || (chunk & 15u) || tile < 128) { fprintf(stderr, "bad chunk or tile\n"); return 2; }
        return img.h.is_reversed ? run_fold<true>(img, next, in, chunk, tile) : run_fold<false>(img, next, in, chunk, tile);
    }
    fprintf(stderr, "unknown mode\n");
    return 2;
}
