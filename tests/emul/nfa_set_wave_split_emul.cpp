// TEST INFRASTRUCTURE ONLY: the host-compilable core of the split path for long strings of wave images (csrc/nfa_set_wave_split_core.h:
// the wide chunk records, the guess from two seeds, the waves of round 0 and of a repair round, the resolve loop over records, the
// hand-over of the resume kernel) and the wide home set (csrc/image_host.cpp: nfa_set_home_wide), run with the host form of the
// lane-crossing primitives (wave_lanes_resume.h: a wave as an array of 64 words) one wave at a time in the order the kernels of
// nfa_set_wave_split.hip run it: round 0, ROUNDS repair rounds with the waves in alternating order on alternating end arrays, resolve.
// On the tables image_host.cpp builds with nfa_set_wave_build -- for every image, the narrow ones too.
//   nfa_set_wave_split_emul split IMAGE.blob BATCH.bin CHUNK LOOKBACK ROUNDS [DEPTH]
//       CHUNK, LOOKBACK and ROUNDS may each be a list ("16,32,64"): every combination is run, chunks outermost, one block of output each.
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  EVERY string is cut into chunks of CHUNK bytes, whatever its length,
//       and enters at {start}.  DEPTH: the stacks get this many slots instead of the tables' (an overflow is then a stack that is full).
//       The final record is compared, word for word, with nfa_wave_walk_from over the whole string; a difference is exit code 5, and so
//       are an empty guess, a lookback range outside the string, and a home set that is empty or names a node the image lacks.
//       stdout: "ok W CHECKS REWALKED SERIAL_STRINGS SERIAL_BYTES HOME_NODES HOME_GUESSES INVALID_ENDS" (HOME_GUESSES: chunks on whose
//       lookback bytes both seeds died or overflowed, so that the guess was the home set itself -- the seeds are walked once more, on
//       their own, for every guess that equals the home set; INVALID_ENDS: chunks whose end the resolve step found INVALID), then one
//       line with the result byte of every string.
//   nfa_set_wave_split_emul pieces IMAGE.blob STATES.bin|- CHUNK LOOKBACK ROUNDS SPLIT_MIN ROUND.bin [ROUND.bin ...]
//       the resume form as nfa_set_wave_resume_kernel and the kernels behind it treat a round: a piece of SPLIT_MIN bytes or more whose
//       record decodes to a live, non-empty set is queued and cut, every other is walked whole.  ROUND.bin and STATES.bin are those of
//       nfa_set_wave_resume_emul.  Behind every piece the record is compared with nfa_wave_resume_piece's on a copy (exit code 5).
//       stdout: "tables WORDS W DEPTH", one line "DIGITS QUEUED" per round, then one line per string: its final record, 68 words in hex.
//   Exit code 3: the image gets no wave tables.
#include <string>

#include "emul_wave.h"
#include "nfa_set_wave_split_core.h"
#include "wave_lanes_resume.h"

using namespace mfa;
typedef emul::WaveHostResume P;
typedef WaveRec<P> Rec;
using emul::fail;
using emul::list_of;

struct Counts { uint64_t rewalked = 0, serial_strings = 0, serial_bytes = 0, home_guesses = 0, invalid_ends = 0; };

// n records in exactly n * 272 bytes; a record that is read before it is written does not look like one
static uint32_t* new_records(uint64_t n) { return emul::new_records(n, kWaveStateWords, 0xa5); }

struct Ctx {
    NfaSetView t;
    uint32_t n_nodes, W;
    uint32_t* stack;
    const uint32_t* home;                                                 // 64 words, 16-byte aligned
};

// one queued string [b, e) from the caller's record `first` (nullptr: {start}), as the kernels treat it: its final record
template <bool REV>
static Rec split_string(const Ctx& x, const uint8_t* bytes, uint64_t b, uint64_t e, uint64_t chunk, uint32_t lookback, uint32_t rounds, const uint32_t* first, Counts& cnt) {
    const uint64_t nc = split_chunks_of(b, e, chunk);
    uint32_t* su = new_records(nc);
    uint32_t* en[2] = {new_records(nc), new_records(nc)};
    const Rec home_rec = wave_rec_of<P>(kSetStateLive, P::load_row(x.home, kWaveLanes));
    for (uint64_t k = 0; k < nc; k++) {                                    // nfa_set_wave_chunk_kernel: wave k
        uint64_t lo, hi;
        split_chunk_range<REV>(b, e, chunk, nc, k, &lo, &hi);
        if (lo < b || hi > e || lo >= hi) fail("a chunk outside its string");
        wave_spec_round0<REV, P>(x.t, x.n_nodes, x.W, x.stack, bytes, b, e, lo, hi, (uint32_t)k, first, x.home, lookback, su, en[0], k);
        if (k == 0) continue;
        uint64_t from, to;
        spec_lookback_range<REV>(b, e, lo, hi, lookback, &from, &to);
        if (from < b || to > e || to - from > lookback || (REV ? from != hi : to != lo)) fail("lookback range outside the string");
        const Rec g = wave_rec_load<P>(su, k);
        if (wave_rec_invalid<P>(g) || wave_rec_dead<P>(g)) fail("an empty guess");
        if (!wave_rec_equal<P>(g, home_rec)) continue;                      // (a guess that is the home set: did both seeds die, or did a walk end there?)
        P::Reg s1 = nfa_wave_start<P>(x.t), s2 = P::load_row(x.home, kWaveLanes);
        if (nfa_wave_walk_from<REV, P>(x.t, x.W, x.stack, bytes, from, to, s1) != 1u && nfa_wave_walk_from<REV, P>(x.t, x.W, x.stack, bytes, from, to, s2) != 1u)
            cnt.home_guesses++;
    }
    for (uint32_t r = 1; r <= rounds; r++) {                                // nfa_set_wave_repair_kernel, launch r; waves in either order
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t k = (r & 1u) ? nc - 1u - i : i;
            uint64_t lo, hi;
            split_chunk_range<REV>(b, e, chunk, nc, k, &lo, &hi);
            if (wave_spec_repair<REV, P>(x.t, x.W, x.stack, bytes, lo, hi, (uint32_t)k, su, en[(r - 1u) & 1u], en[r & 1u], k)) cnt.rewalked++;
        }
    }
    uint64_t serial = 0;                                                    // nfa_set_wave_resolve_kernel: the string's wave
    const Rec fin = wave_spec_resolve_string<REV, P>(x.t, x.n_nodes, x.W, x.stack, bytes, b, e, chunk, (uint32_t)nc, su, en[rounds & 1u], first, &serial);
    if (serial != 0u) { cnt.serial_strings++; cnt.serial_bytes += serial; }
    for (uint64_t k = 0; k < nc; k++)
        if (wave_rec_invalid<P>(wave_rec_load<P>(en[rounds & 1u], k))) cnt.invalid_ends++;
    free(su); free(en[0]); free(en[1]);
    return fin;
}

static bool same_record(const Rec& a, const uint32_t* rec) {
    uint32_t* mine = new_records(1);
    wave_rec_store<P>(mine, 0, a);
    const bool same = memcmp(mine, rec, kWaveStateWords * 4u) == 0;
    free(mine);
    return same;
}

template <bool REV>
static int run_split(const Ctx& x, const std::vector<uint8_t>& file, uint64_t chunk, uint32_t lookback, uint32_t rounds) {
    const emul::Batch batch = emul::read_batch(file);                      // exactly what the kernels may read: whole 16-byte blocks
    const uint64_t n = batch.off.size() - 1;
    uint32_t home_nodes = 0;
    for (uint32_t l = 0; l < kWaveLanes; l++) home_nodes += (uint32_t)__builtin_popcount(x.home[l]);
    if (P::any(P::load_row(x.home, kWaveLanes) & ~P::have(x.n_nodes))) fail("the home set names a node the image lacks");
    if (home_nodes == 0u) fail("an empty home set");
    Counts cnt;
    uint64_t checks = 0;
    std::string results;
    uint32_t* want = new_records(1);
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = batch.off[k], e = batch.off[k + 1];
        if (e - b > kSetMaxString) continue;
        const Rec got = split_string<REV>(x, batch.bytes, b, e, chunk, lookback, rounds, nullptr, cnt);
        memset(want, 0, kWaveStateWords * 4u);                              // a zeroed record: START
        (void)nfa_wave_resume_piece<REV, P>(x.t, x.n_nodes, x.W, x.stack, batch.bytes, b, e, want);      // nfa_wave_walk_from over the whole string
        if (!same_record(got, want)) {
            fprintf(stderr, "string %llu [%llu, %llu): the record differs from the whole walk's\n", (unsigned long long)k, (unsigned long long)b, (unsigned long long)e);
            return 5;
        }
        results += (char)('0' + wave_rec_result<P>(x.t, x.W, got));
        checks++;
    }
    printf("ok %u %llu %llu %llu %llu %u %llu %llu\n%s\n", x.W, (unsigned long long)checks, (unsigned long long)cnt.rewalked, (unsigned long long)cnt.serial_strings,
           (unsigned long long)cnt.serial_bytes, home_nodes, (unsigned long long)cnt.home_guesses, (unsigned long long)cnt.invalid_ends, results.c_str());
    free(want);
    free(batch.bytes);
    return 0;
}

template <bool REV>
static int run_pieces(const Ctx& x, const std::vector<uint8_t>& states, uint64_t chunk, uint32_t lookback, uint32_t rounds, uint64_t split_min, int n_rounds,
                      char** round_files) {
    uint64_t n = 0;
    uint32_t* rec = nullptr;
    uint32_t* whole = new_records(1);
    Counts cnt;
    for (int r = 0; r < n_rounds; r++) {
        const emul::Round round = emul::read_round(round_files[r], r == 0, n);
        const std::vector<uint64_t>& off = round.off;
        const uint8_t* bytes = round.bytes;
        if (r == 0) {
            if (!states.empty() && states.size() != n * kWaveStateWords * 4u) { fprintf(stderr, "the states do not fit the batch\n"); return 2; }
            rec = emul::new_records(n, kWaveStateWords, 0);                // (the caller's records: every string at its start)
            if (!states.empty()) memcpy(rec, states.data(), states.size());
        }
        std::string out;
        uint64_t queued = 0;
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t b = off[k], e = off[k + 1];
            uint32_t* mine = rec + k * kWaveStateWords;
            memcpy(whole, mine, kWaveStateWords * 4u);
            // nfa_set_wave_resume_kernel: decode, hand over or walk
            P::Reg cur;
            const uint32_t tag = nfa_wave_state_decode<P>(x.t, x.n_nodes, mine, e - b, cur);
            uint8_t res;
            if (split_min != 0u && e - b >= split_min && tag == kSetStateLive && P::any(cur)) {
                queued++;
                const Rec fin = split_string<REV>(x, bytes, b, e, chunk, lookback, rounds, mine, cnt);
                nfa_wave_state_encode<P>(fin.tag, fin.nodes, mine);          // nfa_set_wave_resolve_kernel<RESUME>
                res = wave_rec_result<P>(x.t, x.W, fin);
            } else res = wave_resume_entered<REV, P>(x.t, x.W, x.stack, bytes, b, e, tag, cur, mine);
            const uint8_t want = nfa_wave_resume_piece<REV, P>(x.t, x.n_nodes, x.W, x.stack, bytes, b, e, whole);
            if (res != want || memcmp(whole, mine, kWaveStateWords * 4u) != 0) {
                fprintf(stderr, "round %d, string %llu: the record or the result differs from the whole piece's\n", r, (unsigned long long)k);
                return 5;
            }
            out.push_back((char)('0' + res));
        }
        printf("%s %llu\n", out.c_str(), (unsigned long long)queued);
        free(round.bytes);
    }
    for (uint64_t k = 0; k < n; k++)
        for (uint32_t j = 0; j < kWaveStateWords; j++) printf("%08x%c", rec[k * kWaveStateWords + j], j + 1u == kWaveStateWords ? '\n' : ' ');
    free(rec);
    free(whole);
    return 0;
}

int main(int argc, char** argv) {
    const char* usage = "usage: nfa_set_wave_split_emul split IMAGE.blob BATCH.bin CHUNK LOOKBACK ROUNDS [DEPTH] | pieces IMAGE.blob STATES.bin|- CHUNK LOOKBACK ROUNDS SPLIT_MIN ROUND.bin...\n";
    if (argc < 7) { fputs(usage, stderr); return 2; }
    const std::string mode = argv[1];
    const bool pieces = mode == "pieces";
    if ((!pieces && mode != "split") || (pieces && argc < 9)) { fputs(usage, stderr); return 2; }
    HostImage set;
    emul::load_wave(argv[2], set);
    const std::vector<uint64_t> chunks = list_of(argv[4]), lookbacks = list_of(argv[5]), round_counts = list_of(argv[6]);
    for (uint64_t chunk : chunks)
        if (chunk < 16 || (chunk & 15u)) { fprintf(stderr, "bad chunk\n"); return 2; }
    for (uint64_t rounds : round_counts)
        if (rounds > kSpecRoundsMax) { fprintf(stderr, "bad rounds\n"); return 2; }
    Ctx x;
    x.t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    if (!pieces && argc >= 8) x.t.depth = (uint32_t)strtoul(argv[7], nullptr, 10);
    x.n_nodes = set.set_tables[SET_H_NODES]; x.W = set.set_tables[SET_H_WORDS];
    std::vector<uint32_t> stack(x.t.depth);                                 // exactly the slots the kernel has: a sanitizer sees one more
    x.stack = stack.data();
    uint32_t* home = new_records(1);                                         // (16-byte aligned room for 64 words)
    memcpy(home, set.set_home_wide, sizeof set.set_home_wide);
    x.home = home;
    const bool rev = set.h.is_reversed != 0;
    if (pieces) {
        if (chunks.size() != 1 || lookbacks.size() != 1 || round_counts.size() != 1) { fprintf(stderr, "pieces: one chunk, one lookback, one round count\n"); return 2; }
        const std::vector<uint8_t> states = std::string(argv[3]) == "-" ? std::vector<uint8_t>() : emul::slurp(argv[3]);
        const uint64_t split_min = strtoull(argv[7], nullptr, 10);
        emul::print_tables(set);
        const int r = rev ? run_pieces<true>(x, states, chunks[0], (uint32_t)lookbacks[0], (uint32_t)round_counts[0], split_min, argc - 8, argv + 8)
                          : run_pieces<false>(x, states, chunks[0], (uint32_t)lookbacks[0], (uint32_t)round_counts[0], split_min, argc - 8, argv + 8);
        free(home);
        return r;
    }
    const std::vector<uint8_t> batch = emul::slurp(argv[3]);
    for (uint64_t chunk : chunks)
        for (uint64_t lookback : lookbacks)
            for (uint64_t rounds : round_counts) {
                const int r = rev ? run_split<true>(x, batch, chunk, (uint32_t)lookback, (uint32_t)rounds) : run_split<false>(x, batch, chunk, (uint32_t)lookback, (uint32_t)rounds);
                if (r != 0) { fprintf(stderr, "(chunk %llu, lookback %llu, rounds %llu)\n", (unsigned long long)chunk, (unsigned long long)lookback, (unsigned long long)rounds); return r; }
            }
    free(home);
    return 0;
}
