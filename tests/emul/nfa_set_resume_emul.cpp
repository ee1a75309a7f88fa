// TEST INFRASTRUCTURE ONLY: the host-compilable core of the set walk on strings in pieces (csrc/nfa_set_core.h: the record that carries a
// string's set of live nodes from call to call, its decode and check, the walk of one piece from a given set, its encode) run one lane at
// a time, as nfa_set_resume_kernel uses it, on the tables image_host.cpp builds (nfa_set_build).
//   nfa_set_resume_emul pieces IMAGE.blob BATCH.bin CUTS.bin [STATES.bin]
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  CUTS.bin: u64 rounds, then rounds * n pairs (u64 b, u64 e) -- the
//       piece of string k in round r, relative to the start of the string, walked in place in the batch's buffer; a piece beyond
//       MFA_MAX_STRING_BYTES may lie outside the buffer (it is not walked).  STATES.bin: n records of twelve u32 the strings enter the
//       first round with (default: all zero, every string at its start).
//       stdout: one line of result digits per round, then one line per string: its final record, twelve words in hex.
//   nfa_set_resume_emul table IMAGE.blob BATCH.bin
//       The image is tabulated as well (tabulate_nfa hands out the node set behind every state number).  Every whole string is walked
//       through the table, byte by byte, and through the core from a zeroed record: the record's set must be, bit for bit, the node set
//       of the state the table reached, and the result byte what the table's state answers.  The proof of nfa_set_emul step, for whole
//       walks.  stdout: "ok STRINGS STATES W"; a difference is exit code 5.
#include <string>

#include "emul_common.h"
#include "nfa_set_core.h"

using namespace mfa;

struct Record { uint4 q0, q1, q2; };
static_assert(sizeof(Record) == kSetStateWords * 4u, "a record is twelve words");

template <bool REV, int W>
static int run_pieces(const HostImage& set, const std::vector<uint8_t>& file, const std::vector<uint8_t>& cuts, const std::vector<uint8_t>& states) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t n_nodes = set.set_tables[SET_H_NODES];
    std::vector<uint32_t> stack(t.depth + 1u);
    const emul::Batch batch = emul::read_batch(file);                            // exactly the library's read rule: ASan sees a byte beyond it
    const uint64_t n = batch.off.size() - 1;
    uint64_t rounds;
    memcpy(&rounds, cuts.data(), 8);
    if (cuts.size() != 8 + rounds * n * 16 || (!states.empty() && states.size() != n * sizeof(Record))) { fprintf(stderr, "cuts or states do not fit the batch\n"); return 2; }
    std::vector<Record> rec(n, Record{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)});
    if (!states.empty()) memcpy(rec.data(), states.data(), states.size());
    for (uint64_t r = 0; r < rounds; r++) {
        std::string out;
        for (uint64_t k = 0; k < n; k++) {
            uint64_t b, e;
            memcpy(&b, cuts.data() + 8 + (r * n + k) * 16, 8); memcpy(&e, cuts.data() + 8 + (r * n + k) * 16 + 8, 8);
            if (e < b || (e - b <= kSetMaxString && batch.off[k] + e > batch.off[k + 1])) { fprintf(stderr, "round %llu, string %llu: a piece outside its string\n", (unsigned long long)r, (unsigned long long)k); return 2; }
            out.push_back((char)('0' + nfa_set_resume_piece<REV, W>(t, n_nodes, stack.data(), 1u, batch.bytes, batch.off[k] + b, batch.off[k] + e, rec[k].q0, rec[k].q1, rec[k].q2)));
        }
        puts(out.c_str());
    }
    for (uint64_t k = 0; k < n; k++) {
        uint32_t w[kSetStateWords];
        memcpy(w, &rec[k], sizeof w);
        for (uint32_t j = 0; j < kSetStateWords; j++) printf("%08x%c", w[j], j + 1u == kSetStateWords ? '\n' : ' ');
    }
    free(batch.bytes);
    return 0;
}

template <bool REV, int W>
static int run_table(const HostImage& tab, const HostImage& set, const std::vector<std::string>& sets, const std::vector<uint8_t>& file) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t n_nodes = set.set_tables[SET_H_NODES];
    std::vector<uint32_t> stack(t.depth + 1u);
    const emul::Batch batch = emul::read_batch(file);
    const uint64_t n = batch.off.size() - 1;
    if (sets.size() != tab.dfa_states) { fprintf(stderr, "%zu sets for %u states\n", sets.size(), tab.dfa_states); return 5; }
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = batch.off[k], e = batch.off[k + 1];
        if (e - b > kSetMaxString) continue;
        uint32_t st = 1;                                                          // the walk nobody shares: the image's table, byte by byte
        for (uint64_t i = 0; i < e - b; i++) st = tab.dfa_trans[(size_t)st * tab.n_classes + tab.byte_class[batch.bytes[REV ? e - 1u - i : b + i]]];
        uint32_t want[kSetStateWords] = {kSetStateLive};
        for (uint32_t v = 0; v < tab.h.n_nodes; v++)
            if ((sets[st][v >> 3] >> (v & 7)) & 1) want[4u + (v >> 5)] |= 1u << (v & 31u);
        Record rec{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        const uint8_t res = nfa_set_resume_piece<REV, W>(t, n_nodes, stack.data(), 1u, batch.bytes, b, e, rec.q0, rec.q1, rec.q2);
        if (memcmp(&rec, want, sizeof rec) != 0 || res != (tab.dfa_accept[st] ? 1 : 0)) {
            fprintf(stderr, "string %llu (%llu bytes): the record is not the node set of the table's state %u, or answers %d where the table says %d\n",
                    (unsigned long long)k, (unsigned long long)(e - b), st, (int)res, (int)tab.dfa_accept[st]);
            return 5;
        }
    }
    printf("ok %llu %u %d\n", (unsigned long long)n, tab.dfa_states, W);
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: nfa_set_resume_emul pieces IMAGE.blob BATCH.bin CUTS.bin [STATES.bin] | table IMAGE.blob BATCH.bin\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> blob = emul::slurp(argv[2]);
    HostImage tab, set;
    if (parse_blob(blob.data(), blob.size(), tab) != MFA_OK || tab.h.kind != MFA_KIND_NFA) { fprintf(stderr, "not a memory-less image\n"); return 2; }
    set = tab;
    const int rc = nfa_set_build(set);
    if (rc != MFA_OK) { fprintf(stderr, "no set-walk tables: %d\n", rc); return 3; }
    const uint32_t W = set.set_tables[SET_H_WORDS];
    const bool rev = set.h.is_reversed != 0;
    const std::vector<uint8_t> batch = emul::slurp(argv[3]);
#define BY_W(CALL1, CALL2, CALL4, CALL8) (W == 1 ? CALL1 : W == 2 ? CALL2 : W == 4 ? CALL4 : CALL8)
    if (mode == "pieces" && argc >= 5) {
        const std::vector<uint8_t> cuts = emul::slurp(argv[4]);
        const std::vector<uint8_t> states = argc >= 6 ? emul::slurp(argv[5]) : std::vector<uint8_t>();
        if (rev) return BY_W((run_pieces<true, 1>(set, batch, cuts, states)), (run_pieces<true, 2>(set, batch, cuts, states)), (run_pieces<true, 4>(set, batch, cuts, states)), (run_pieces<true, 8>(set, batch, cuts, states)));
        return BY_W((run_pieces<false, 1>(set, batch, cuts, states)), (run_pieces<false, 2>(set, batch, cuts, states)), (run_pieces<false, 4>(set, batch, cuts, states)), (run_pieces<false, 8>(set, batch, cuts, states)));
    }
    if (mode == "table") {
        std::vector<std::string> sets;
        if (tabulate_nfa(tab, MFA_MAX_DFA_STATES, &sets) != MFA_OK) { fprintf(stderr, "not tabulated\n"); return 2; }
        if (rev) return BY_W((run_table<true, 1>(tab, set, sets, batch)), (run_table<true, 2>(tab, set, sets, batch)), (run_table<true, 4>(tab, set, sets, batch)), (run_table<true, 8>(tab, set, sets, batch)));
        return BY_W((run_table<false, 1>(tab, set, sets, batch)), (run_table<false, 2>(tab, set, sets, batch)), (run_table<false, 4>(tab, set, sets, batch)), (run_table<false, 8>(tab, set, sets, batch)));
    }
    fprintf(stderr, "unknown mode\n");
    return 2;
}
