// TEST INFRASTRUCTURE ONLY: the host-compilable core of the split path for long strings of set-walk images (csrc/nfa_set_split_core.h: the
// chunk records, the guess from two seeds, the lanes of round 0 and of a repair round, the resolve loop over records) and the home set
// (csrc/image_host.cpp: nfa_set_home), run one lane at a time in the order the kernels of nfa_set_split.hip run it: round 0, ROUNDS repair
// rounds with the lanes in alternating order on alternating end arrays, resolve.
//   nfa_set_split_emul IMAGE.blob BATCH.bin CHUNK LOOKBACK ROUNDS one|every
//       CHUNK, LOOKBACK and ROUNDS may each be a list ("16,32,64"): every combination is run, chunks outermost, one block of output each.
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  EVERY string is cut into chunks of CHUNK bytes, whatever its length.
//       one: every string from a zeroed record (tag START: {start}); every: also from every node set tabulate_nfa hands out for the image,
//       and from the empty set (the resume form).
//       The final record is compared, word for word, with nfa_set_walk_from over the whole string from the same set; a difference is exit
//       code 5, and so are an empty guess, a lookback range outside the string, and a home set that is empty or names a node the image lacks.
//       stdout: "ok W CHECKS REWALKED SERIAL_STRINGS SERIAL_BYTES HOME_NODES HOME_GUESSES" (HOME_GUESSES: chunks on whose lookback bytes both
//       seeds died, so that the guess was the home set itself), then one line with the result byte of every string from {start}.
#include <string>

#include "emul_common.h"
#include "nfa_set_split_core.h"

using namespace mfa;
using emul::fail;
using emul::list_of;

struct Counts { uint64_t rewalked = 0, serial_strings = 0, serial_bytes = 0, home_guesses = 0; };

static const SetRec kStartRec = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};

// one queued string [b, e) from the record `first`, as the kernels treat it: its final record
template <bool REV, int W>
static SetRec split_string(const NfaSetView& t, uint32_t n_nodes, uint32_t* stack, const uint8_t* bytes, uint64_t b, uint64_t e, uint64_t chunk, uint32_t lookback,
                           uint32_t rounds, const SetHome& home, const SetRec& first, Counts& cnt) {
    const uint64_t nc = split_chunks_of(b, e, chunk);
    std::vector<uint4> su(nc * kSetRecQuarters), en[2] = {std::vector<uint4>(nc * kSetRecQuarters), std::vector<uint4>(nc * kSetRecQuarters)};
    uint32_t home_set[W];
    for (int k = 0; k < W; k++) home_set[k] = home.w[k];
    const SetRec home_rec = set_rec_of<W>(kSetStateLive, home_set);
    for (uint64_t k = 0; k < nc; k++) {                                     // nfa_set_chunk_kernel: lane k
        uint64_t lo, hi;
        split_chunk_range<REV>(b, e, chunk, nc, k, &lo, &hi);
        if (lo < b || hi > e || lo >= hi) fail("a chunk outside its string");
        set_spec_round0<REV, W>(t, n_nodes, stack, 1u, bytes, b, e, lo, hi, (uint32_t)k, first, home, lookback, su.data(), en[0].data(), k);
        if (k == 0) continue;
        uint64_t from, to;
        spec_lookback_range<REV>(b, e, lo, hi, lookback, &from, &to);
        if (from < b || to > e || to - from > lookback || (REV ? from != hi : to != lo)) fail("lookback range outside the string");
        const SetRec g = set_rec_load(su.data(), k);
        if (set_rec_invalid(g) || set_rec_dead(g)) fail("an empty guess");
        uint32_t s1[W], s2[W];                                              // both seeds on their own: did they die?
        nfa_set_start<W>(t, s1);
        for (int j = 0; j < W; j++) s2[j] = home.w[j];
        if (nfa_set_walk_from<REV, W>(t, stack, 1u, bytes, from, to, s1) != 1u && nfa_set_walk_from<REV, W>(t, stack, 1u, bytes, from, to, s2) != 1u) {
            if (!set_rec_equal(g, home_rec)) fail("both seeds died and the guess is not the home set");
            cnt.home_guesses++;
        }
    }
    for (uint32_t r = 1; r <= rounds; r++) {                                // nfa_set_repair_kernel, launch r; lanes in either order
        const std::vector<uint4>& prev = en[(r - 1u) & 1u];
        std::vector<uint4>& next = en[r & 1u];
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t k = (r & 1u) ? nc - 1u - i : i;
            uint64_t lo, hi;
            split_chunk_range<REV>(b, e, chunk, nc, k, &lo, &hi);
            if (set_spec_repair<REV, W>(t, n_nodes, stack, 1u, bytes, lo, hi, (uint32_t)k, su.data(), prev.data(), next.data(), k)) cnt.rewalked++;
        }
    }
    uint64_t serial = 0;                                                    // nfa_set_resolve_kernel: the string's lane
    const SetRec fin = set_spec_resolve_string<REV, W>(t, n_nodes, stack, 1u, bytes, b, e, chunk, (uint32_t)nc, su.data(), en[rounds & 1u].data(), first, &serial);
    if (serial != 0u) { cnt.serial_strings++; cnt.serial_bytes += serial; }
    return fin;
}

template <bool REV, int W>
static int run(const HostImage& set, const std::vector<SetRec>& starts, const std::vector<uint8_t>& file, uint64_t chunk, uint32_t lookback, uint32_t rounds) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t n_nodes = set.set_tables[SET_H_NODES];
    std::vector<uint32_t> stack(t.depth + 1u);
    const emul::Batch batch = emul::read_batch(file);                      // exactly what the kernels may read: whole 16-byte blocks
    const uint64_t n = batch.off.size() - 1;
    SetHome home;
    uint32_t home_nodes = 0;
    for (int k = 0; k < kSetStateNodeWords; k++) { home.w[k] = set.set_home[k]; home_nodes += (uint32_t)__builtin_popcount(home.w[k]); }
    for (uint32_t v = 0; v < 256u; v++)
        if (((home.w[v >> 5] >> (v & 31u)) & 1u) && v >= n_nodes) fail("the home set names a node the image lacks");
    if (home_nodes == 0u) fail("an empty home set");
    Counts cnt;
    uint64_t checks = 0;
    std::string results;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = batch.off[k], e = batch.off[k + 1];
        if (e - b > kSetMaxString) continue;
        for (size_t s = 0; s < starts.size(); s++) {
            const SetRec got = split_string<REV, W>(t, n_nodes, stack.data(), batch.bytes, b, e, chunk, lookback, rounds, home, starts[s], cnt);
            uint32_t cur[W];
            const uint32_t tag = set_rec_set<W>(t, n_nodes, starts[s], cur);
            if (tag != kSetStateLive) fail("a start record that is not live");
            const SetRec want = set_chunk_walk<REV, W>(t, stack.data(), 1u, batch.bytes, b, e, cur);      // nfa_set_walk_from over the whole string
            if (memcmp(&got, &want, sizeof got) != 0) {
                fprintf(stderr, "string %llu [%llu, %llu) from start %zu: the record differs from the whole walk's\n", (unsigned long long)k, (unsigned long long)b,
                        (unsigned long long)e, s);
                return 5;
            }
            if (s == 0) results += (char)('0' + set_rec_result<W>(t, n_nodes, got));
            checks++;
        }
    }
    printf("ok %d %llu %llu %llu %llu %u %llu\n%s\n", W, (unsigned long long)checks, (unsigned long long)cnt.rewalked, (unsigned long long)cnt.serial_strings,
           (unsigned long long)cnt.serial_bytes, home_nodes, (unsigned long long)cnt.home_guesses, results.c_str());
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: nfa_set_split_emul IMAGE.blob BATCH.bin CHUNK LOOKBACK ROUNDS one|every\n"); return 2; }
    const std::vector<uint8_t> blob = emul::slurp(argv[1]);
    HostImage tab, set;
    if (parse_blob(blob.data(), blob.size(), tab) != MFA_OK || tab.h.kind != MFA_KIND_NFA) { fprintf(stderr, "not a memory-less image\n"); return 2; }
    set = tab;
    const int rc = nfa_set_build(set);
    if (rc != MFA_OK) { fprintf(stderr, "no set-walk tables: %d\n", rc); return 3; }
    const std::vector<uint8_t> batch = emul::slurp(argv[2]);
    const std::vector<uint64_t> chunks = list_of(argv[3]), lookbacks = list_of(argv[4]), round_counts = list_of(argv[5]);
    for (uint64_t chunk : chunks)
        if (chunk < 16 || (chunk & 15u)) { fprintf(stderr, "bad chunk\n"); return 2; }
    for (uint64_t rounds : round_counts)
        if (rounds > kSpecRoundsMax) { fprintf(stderr, "bad rounds\n"); return 2; }
    std::vector<SetRec> starts{kStartRec};
    if (std::string(argv[6]) == "every") {
        std::vector<std::string> sets;
        if (tabulate_nfa(tab, MFA_MAX_DFA_STATES, &sets) != MFA_OK) { fprintf(stderr, "not tabulated\n"); return 2; }
        for (const std::string& s : sets) {                                // (sets[0] is the empty set)
            uint32_t w[kSetStateNodeWords] = {0};
            for (uint32_t v = 0; v < tab.h.n_nodes; v++)
                if ((s[v >> 3] >> (v & 7)) & 1) w[v >> 5] |= 1u << (v & 31u);
            starts.push_back(SetRec{make_uint4(kSetStateLive, 0, 0, 0), make_uint4(w[0], w[1], w[2], w[3]), make_uint4(w[4], w[5], w[6], w[7])});
        }
    }
    const uint32_t W = set.set_tables[SET_H_WORDS];
    const bool rev = set.h.is_reversed != 0;
#define GO(R, WW) run<R, WW>(set, starts, batch, chunk, (uint32_t)lookback, (uint32_t)rounds)
    for (uint64_t chunk : chunks)
        for (uint64_t lookback : lookbacks)
            for (uint64_t rounds : round_counts) {
                const int r = rev ? (W == 1 ? GO(true, 1) : W == 2 ? GO(true, 2) : W == 4 ? GO(true, 4) : GO(true, 8))
                                  : (W == 1 ? GO(false, 1) : W == 2 ? GO(false, 2) : W == 4 ? GO(false, 4) : GO(false, 8));
                if (r != 0) { fprintf(stderr, "(chunk %llu, lookback %llu, rounds %llu)\n", (unsigned long long)chunk, (unsigned long long)lookback, (unsigned long long)rounds); return r; }
            }
#undef GO
    return 0;
}
