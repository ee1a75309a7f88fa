// TEST INFRASTRUCTURE ONLY: the host-compilable core of the set walk of memory-less automata (csrc/nfa_set_core.h: the reference's step
// on a bit mask of live nodes, the walk of one string) run one lane at a time, as nfa_set_kernel uses it, on the tables image_host.cpp
// builds (nfa_set_build).
//   nfa_set_emul step IMAGE.blob
//       The image is tabulated (tabulate_nfa, which hands out the node set behind every state number) AND given set-walk tables.  Every
//       tabulated state set, as a mask, is stepped over every byte class with the core's step: the mask reached must be, bit for bit, the
//       node set of the state the table's row names, and must accept exactly when the table says so.
//       stdout: "ok STATES CLASSES W DEPTH"; a difference is exit code 5.
//   nfa_set_emul match IMAGE.blob BATCH.bin
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  stdout: one result digit per string, then a newline.
//   nfa_set_emul table IMAGE.blob
//       stdout: "tables WORDS W DEPTH CLASSES" -- the words of the lane tables, their mask width, their stack depth and byte classes: what
//       set_lds_of (csrc/nfa_set.h) places them by, (DEPTH * 256 + WORDS) * 4 against 65536.
//   Exit code 3: the image gets no set-walk tables.
#include <string>

#include "emul_common.h"
#include "nfa_set_core.h"

using namespace mfa;

template <int W>
static int run_step(const HostImage& tab, const HostImage& set, const std::vector<std::string>& sets) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    std::vector<uint32_t> stack(t.depth + 1u);
    // state number -> mask: the table's own node set (bit v & 7 of byte v >> 3), widened to W words
    auto mask_of = [&](uint32_t s, uint32_t (&m)[W]) {
        for (int k = 0; k < W; k++) m[k] = 0;
        for (uint32_t v = 0; v < tab.h.n_nodes; v++)
            if ((sets[s][v >> 3] >> (v & 7)) & 1) m[v >> 5] |= 1u << (v & 31u);
    };
    if (sets.size() != tab.dfa_states) { fprintf(stderr, "%zu sets for %u states\n", sets.size(), tab.dfa_states); return 5; }
    uint32_t one[W], begin[W];
    nfa_set_start<W>(t, begin);
    if (tab.dfa_states > 1) { mask_of(1, one); if (memcmp(one, begin, sizeof one) != 0) { fprintf(stderr, "state 1 is not {start}\n"); return 5; } }
    for (uint32_t s = 1; s < tab.dfa_states; s++) {
        uint32_t from[W], want[W];
        mask_of(s, from);
        if (nfa_set_accepts<W>(t, from) != (tab.dfa_accept[s] ? 1 : 0)) { fprintf(stderr, "state %u: accept differs\n", s); return 5; }
        for (uint32_t c = 0; c < tab.n_classes; c++) {
            uint32_t cur[W];
            memcpy(cur, from, sizeof cur);
            const uint32_t alive = nfa_set_step<W>(t, stack.data(), 1u, cur, c);
            const uint32_t to = tab.dfa_trans[(size_t)s * tab.n_classes + c];
            mask_of(to, want);
            if (alive > 1u || (alive == 0u) != (to == 0u) || memcmp(cur, want, sizeof cur) != 0) {
                fprintf(stderr, "state %u class %u: the step's set is not the set of the table's state %u\n", s, c, to);
                return 5;
            }
        }
    }
    printf("ok %u %u %d %u\n", tab.dfa_states, tab.n_classes, W, t.depth);
    return 0;
}

template <bool REV, int W>
static int run_match(const HostImage& set, const std::vector<uint8_t>& file) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    std::vector<uint32_t> stack(t.depth + 1u);
    const emul::Batch batch = emul::read_batch(file);                            // exactly the library's read rule: ASan sees a byte beyond it
    std::string out;
    for (size_t k = 0; k + 1 < batch.off.size(); k++) out.push_back((char)('0' + nfa_set_walk<REV, W>(t, stack.data(), 1u, batch.bytes, batch.off[k], batch.off[k + 1])));
    puts(out.c_str());
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: nfa_set_emul step IMAGE.blob | match IMAGE.blob BATCH.bin | table IMAGE.blob\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> blob = emul::slurp(argv[2]);
    HostImage tab, set;
    if (parse_blob(blob.data(), blob.size(), tab) != MFA_OK || tab.h.kind != MFA_KIND_NFA) { fprintf(stderr, "not a memory-less image\n"); return 2; }
    set = tab;
    const int rc = nfa_set_build(set);
    if (rc != MFA_OK) { fprintf(stderr, "no set-walk tables: %d\n", rc); return 3; }
    const uint32_t W = set.set_tables[SET_H_WORDS];
    const bool rev = set.h.is_reversed != 0;
    if (mode == "table") {
        printf("tables %zu %u %u %u\n", set.set_tables.size(), W, set.set_tables[SET_H_DEPTH], set.set_tables[SET_H_CLASSES]);
        return 0;
    }
#define BY_W(CALL1, CALL2, CALL4, CALL8) (W == 1 ? CALL1 : W == 2 ? CALL2 : W == 4 ? CALL4 : CALL8)
    if (mode == "step") {
        std::vector<std::string> sets;
        if (tabulate_nfa(tab, MFA_MAX_DFA_STATES, &sets) != MFA_OK) { fprintf(stderr, "not tabulated\n"); return 2; }
        return BY_W(run_step<1>(tab, set, sets), run_step<2>(tab, set, sets), run_step<4>(tab, set, sets), run_step<8>(tab, set, sets));
    }
    if (mode == "match" && argc >= 4) {
        const std::vector<uint8_t> batch = emul::slurp(argv[3]);
        if (rev) return BY_W((run_match<true, 1>(set, batch)), (run_match<true, 2>(set, batch)), (run_match<true, 4>(set, batch)), (run_match<true, 8>(set, batch)));
        return BY_W((run_match<false, 1>(set, batch)), (run_match<false, 2>(set, batch)), (run_match<false, 4>(set, batch)), (run_match<false, 8>(set, batch)));
    }
    fprintf(stderr, "unknown mode\n");
    return 2;
}
