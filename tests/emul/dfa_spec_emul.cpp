// TEST INFRASTRUCTURE ONLY: the host-compilable core of the split path for large-table memory-less automata (csrc/dfa_spec_core.h: the
// lookback range, the guess from two seeds, when a chunk is walked again, the resolve loop over records, the home state) run one lane
// at a time in the order the kernels of dfa_spec.hip run it: round 0, ROUNDS repair rounds on alternating end arrays, resolve.
//   dfa_spec_emul IMAGE.blob BATCH.bin CHUNK LOOKBACK ROUNDS one|every
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  EVERY string is cut into chunks of CHUNK bytes, whatever its length.
//       one: every string from state 1; every: from every state set of the image but the dead one (the resume form).
//       The state reached is compared with a plain byte-by-byte walk of the image's table from the same state; a difference is exit code 5.
//       stdout: "ok STATES CHECKS REWALKED SERIAL_STRINGS SERIAL_BYTES HOME", then one line with the result byte of every string from state 1.
#include <string>

#include "emul_common.h"
#include "dfa_spec_core.h"

using namespace mfa;

// the walk nobody shares: the image's table, byte by byte
template <bool REV>
static uint32_t plain_walk(const HostImage& img, const uint8_t* bytes, uint64_t b, uint64_t e, uint32_t st) {
    for (uint64_t i = 0; i < e - b; i++) st = img.dfa_trans[(size_t)st * img.n_classes + img.byte_class[bytes[REV ? e - 1u - i : b + i]]];
    return st;
}

struct Counts { uint64_t rewalked = 0, serial_strings = 0, serial_bytes = 0; };

// one queued string [b, e) from the true state s0, as the kernels treat it
template <bool REV>
static uint32_t spec_string(const HostImage& img, const uint8_t* bytes, uint64_t b, uint64_t e, uint64_t chunk, uint32_t lookback, uint32_t rounds,
                            uint32_t home, uint32_t s0, Counts& cnt) {
    const uint32_t* trans = img.dfa_trans.data();
    const uint64_t nc = split_chunks_of(b, e, chunk);
    std::vector<uint32_t> su(nc), en[2] = {std::vector<uint32_t>(nc), std::vector<uint32_t>(nc)};
    for (uint64_t k = 0; k < nc; k++) {                                     // dfa_spec_walk_kernel: lane k
        uint64_t lo, hi, from, to;
        split_chunk_range<REV>(b, e, chunk, nc, k, &lo, &hi);
        uint32_t st = s0;
        if (k != 0) {
            spec_lookback_range<REV>(b, e, lo, hi, lookback, &from, &to);
            if (from < b || to > e || to - from > lookback || (REV ? from != hi : to != lo)) { fprintf(stderr, "lookback range outside the string\n"); exit(5); }
            st = spec_guess<REV, uint32_t>(trans, img.byte_class, img.n_classes, bytes, from, to, home);
            if (st == 0u) { fprintf(stderr, "a guess of 0\n"); exit(5); }
        }
        su[k] = st;
        en[0][k] = resume_piece_big<REV, uint32_t>(trans, img.byte_class, img.n_classes, bytes, lo, hi, st);
    }
    for (uint32_t r = 1; r <= rounds; r++) {                                // dfa_spec_repair_kernel, launch r; lanes in either order
        const std::vector<uint32_t>& prev = en[(r - 1u) & 1u];
        std::vector<uint32_t>& next = en[r & 1u];
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t k = (r & 1u) ? nc - 1u - i : i;
            const uint32_t p = k != 0 ? prev[k - 1u] : su[k];
            if (!spec_needs_rewalk((uint32_t)k, su[k], p)) { next[k] = prev[k]; continue; }
            uint64_t lo, hi;
            split_chunk_range<REV>(b, e, chunk, nc, k, &lo, &hi);
            su[k] = p;
            next[k] = resume_piece_big<REV, uint32_t>(trans, img.byte_class, img.n_classes, bytes, lo, hi, p);
            cnt.rewalked++;
        }
    }
    uint32_t cur = s0;                                                      // dfa_spec_resolve_kernel: the string's lane
    const uint32_t c = spec_resolve(su.data(), en[rounds & 1u].data(), (uint32_t)nc, &cur);
    if (c < nc) {
        uint64_t lo, hi, from, to;
        split_chunk_range<REV>(b, e, chunk, nc, c, &lo, &hi);
        spec_rest_range<REV>(b, e, lo, hi, &from, &to);
        cur = resume_piece_big<REV, uint32_t>(trans, img.byte_class, img.n_classes, bytes, from, to, cur);
        cnt.serial_strings++;
        cnt.serial_bytes += to - from;
    }
    return cur;
}

template <bool REV>
static int run(const HostImage& img, const std::vector<uint8_t>& file, uint64_t chunk, uint32_t lookback, uint32_t rounds, bool every) {
    const emul::Batch batch = emul::read_batch(file);                      // exactly what the kernels may read: whole 16-byte blocks
    const std::vector<uint64_t>& off = batch.off;
    const uint8_t* bytes = batch.bytes;
    const uint64_t n = off.size() - 1;
    const uint32_t home = spec_home_state(img.dfa_trans.data(), img.dfa_states, img.n_classes);
    if (home == 0u || home >= img.dfa_states) { fprintf(stderr, "home state %u\n", home); return 5; }
    Counts cnt;
    uint64_t checks = 0;
    std::string results;
    for (uint64_t k = 0; k < n; k++) {
        for (uint32_t s0 = 1; s0 < (every ? img.dfa_states : 2u); s0++) {
            const uint32_t got = spec_string<REV>(img, bytes, off[k], off[k + 1], chunk, lookback, rounds, home, s0, cnt);
            const uint32_t want = plain_walk<REV>(img, bytes, off[k], off[k + 1], s0);
            if (got != want) {
                fprintf(stderr, "string %llu [%llu, %llu) from state %u: %u, plain walk %u\n", (unsigned long long)k, (unsigned long long)off[k],
                        (unsigned long long)off[k + 1], s0, got, want);
                return 5;
            }
            if (s0 == 1u) results += img.dfa_accept[got] ? '1' : '0';
            checks++;
        }
    }
    printf("ok %u %llu %llu %llu %llu %u\n%s\n", img.dfa_states, (unsigned long long)checks, (unsigned long long)cnt.rewalked,
           (unsigned long long)cnt.serial_strings, (unsigned long long)cnt.serial_bytes, home, results.c_str());
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: dfa_spec_emul IMAGE.blob BATCH.bin CHUNK LOOKBACK ROUNDS one|every\n"); return 2; }
    HostImage img;
    emul::load_memoryless(argv[1], img);
    const std::vector<uint8_t> batch = emul::slurp(argv[2]);
    const uint64_t chunk = strtoull(argv[3], nullptr, 10);
    const uint32_t lookback = (uint32_t)strtoul(argv[4], nullptr, 10), rounds = (uint32_t)strtoul(argv[5], nullptr, 10);
    if (chunk < 16 || (chunk & 15u) || rounds > kSpecRoundsMax) { fprintf(stderr, "bad chunk or rounds\n"); return 2; }
    const bool every = std::string(argv[6]) == "every";
    return img.h.is_reversed ? run<true>(img, batch, chunk, lookback, rounds, every) : run<false>(img, batch, chunk, lookback, rounds, every);
}
