// TEST INFRASTRUCTURE ONLY: the host-compilable core of the wave-cooperative set walk on strings in pieces (csrc/nfa_set_wave_core.h: the
// record of 68 words that carries a string's node set from call to call, its decode and check, the walk of one piece from the set it
// holds, its encode) run with the host form of the lane-crossing primitives (wave_lanes.h and wave_lanes_resume.h: a wave as an array of
// 64 words), as nfa_set_wave_resume_kernel uses it, on the tables image_host.cpp builds (nfa_set_wave_build) -- for every image, the
// narrow ones too.
//   nfa_set_wave_resume_emul pieces IMAGE.blob STATES.bin ROUND.bin [ROUND.bin ...]
//       ROUND.bin: one round of pieces as one call gets it -- u64 n, u64 total, u64 offsets[n + 1], then `total` bytes.  The bytes get
//       exactly the room the library's read rule makes readable (emul::padded); piece k is [offsets[k], offsets[k + 1]) of them and may
//       lie outside them (a piece beyond MFA_MAX_STRING_BYTES, or of a record that is dead or in error: it is not walked).  STATES.bin:
//       n records of 68 u32 the strings enter the first round with, or "-": all zero, every string at its start.  The records live in
//       exactly n * 272 bytes.
//       stdout: "tables WORDS W DEPTH", then one line of result digits per round, then one line per string: its final record, 68 words
//       in hex.
//   nfa_set_wave_resume_emul table IMAGE.blob BATCH.bin
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  The image is tabulated as well (tabulate_nfa hands out the node
//       set behind every state number).  Every whole string is walked through the table, byte by byte, and through the core from a
//       zeroed record: the record's set must be, bit for bit, the node set of the state the table reached, and the result byte what the
//       table's state answers.  stdout: "tables WORDS W DEPTH", then "ok STRINGS STATES"; a difference is exit code 5.
//   Exit code 3: the image gets no wave tables (an epsilon cycle, more than 2048 nodes).
#include <string>

#include "emul_wave.h"
#include "wave_lanes_resume.h"

using namespace mfa;
typedef emul::WaveHostResume P;

// n zeroed records in exactly n * 272 bytes
static uint32_t* new_records(uint64_t n) { return emul::new_records(n, kWaveStateWords, 0); }

template <bool REV>
static int run_pieces(const HostImage& set, const std::vector<uint8_t>& states, int n_rounds, char** round_files) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t W = set.set_tables[SET_H_WORDS], n_nodes = set.set_tables[SET_H_NODES];
    std::vector<uint32_t> stack(t.depth);                           // exactly the slots the kernel has: a sanitizer sees one more
    uint64_t n = 0;
    uint32_t* rec = nullptr;
    for (int r = 0; r < n_rounds; r++) {
        const emul::Round round = emul::read_round(round_files[r], r == 0, n);      // exactly the library's read rule: ASan sees a byte beyond it
        const std::vector<uint64_t>& off = round.off;
        if (r == 0) {
            if (!states.empty() && states.size() != n * kWaveStateWords * 4u) { fprintf(stderr, "the states do not fit the batch\n"); return 2; }
            rec = new_records(n);
            if (!states.empty()) memcpy(rec, states.data(), states.size());
        }
        std::string out;
        for (uint64_t k = 0; k < n; k++)
            out.push_back((char)('0' + nfa_wave_resume_piece<REV, P>(t, n_nodes, W, stack.data(), round.bytes, off[k], off[k + 1], rec + k * kWaveStateWords)));
        puts(out.c_str());
        free(round.bytes);
    }
    for (uint64_t k = 0; k < n; k++)
        for (uint32_t j = 0; j < kWaveStateWords; j++) printf("%08x%c", rec[k * kWaveStateWords + j], j + 1u == kWaveStateWords ? '\n' : ' ');
    free(rec);
    return 0;
}

template <bool REV>
static int run_table(const HostImage& tab, const HostImage& set, const std::vector<std::string>& sets, const std::vector<uint8_t>& file) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t W = set.set_tables[SET_H_WORDS], n_nodes = set.set_tables[SET_H_NODES];
    std::vector<uint32_t> stack(t.depth);
    const emul::Batch batch = emul::read_batch(file);
    const uint64_t n = batch.off.size() - 1;
    if (sets.size() != tab.dfa_states) { fprintf(stderr, "%zu sets for %u states\n", sets.size(), tab.dfa_states); return 5; }
    uint32_t* rec = new_records(1);
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = batch.off[k], e = batch.off[k + 1];
        if (e - b > kSetMaxString) continue;
        uint32_t st = 1;                                                          // the walk nobody shares: the image's table, byte by byte
        for (uint64_t i = 0; i < e - b; i++) st = tab.dfa_trans[(size_t)st * tab.n_classes + tab.byte_class[batch.bytes[REV ? e - 1u - i : b + i]]];
        uint32_t want[kWaveStateWords] = {kSetStateLive};
        for (uint32_t v = 0; v < tab.h.n_nodes; v++)
            if ((sets[st][v >> 3] >> (v & 7)) & 1) want[4u + (v >> 5)] |= 1u << (v & 31u);
        memset(rec, 0, sizeof want);
        const uint8_t res = nfa_wave_resume_piece<REV, P>(t, n_nodes, W, stack.data(), batch.bytes, b, e, rec);
        if (memcmp(rec, want, sizeof want) != 0 || res != (tab.dfa_accept[st] ? 1 : 0)) {
            fprintf(stderr, "string %llu (%llu bytes): the record is not the node set of the table's state %u, or answers %d where the table says %d\n",
                    (unsigned long long)k, (unsigned long long)(e - b), st, (int)res, (int)tab.dfa_accept[st]);
            return 5;
        }
    }
    printf("ok %llu %u\n", (unsigned long long)n, tab.dfa_states);
    free(rec);
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: nfa_set_wave_resume_emul pieces IMAGE.blob STATES.bin|- ROUND.bin... | table IMAGE.blob BATCH.bin\n"); return 2; }
    const std::string mode = argv[1];
    HostImage tab, set;
    emul::load_wave(argv[2], set, &tab);
    const bool rev = set.h.is_reversed != 0;
    emul::print_tables(set);
    if (mode == "pieces" && argc >= 5) {
        const std::vector<uint8_t> states = std::string(argv[3]) == "-" ? std::vector<uint8_t>() : emul::slurp(argv[3]);
        return rev ? run_pieces<true>(set, states, argc - 4, argv + 4) : run_pieces<false>(set, states, argc - 4, argv + 4);
    }
    if (mode == "table") {
        std::vector<std::string> sets;
        if (tabulate_nfa(tab, MFA_MAX_DFA_STATES, &sets) != MFA_OK) { fprintf(stderr, "not tabulated\n"); return 2; }
        const std::vector<uint8_t> batch = emul::slurp(argv[3]);
        return rev ? run_table<true>(tab, set, sets, batch) : run_table<false>(tab, set, sets, batch);
    }
    fprintf(stderr, "unknown mode\n");
    return 2;
}
