// TEST INFRASTRUCTURE ONLY: the host-compilable core of the wave-cooperative set walk (csrc/nfa_set_wave_core.h: the reference's step on a
// node set that lies across the 64 lanes of a wave, the walk of one string) run with the host form of its lane-crossing primitives
// (wave_lanes.h: a wave as an array of 64 words), as nfa_set_wave_kernel uses it, on the tables image_host.cpp builds
// (nfa_set_wave_build) -- for every image, the narrow ones too.
//   nfa_set_wave_emul step IMAGE.blob
//       The image is tabulated (tabulate_nfa, which hands out the node set behind every state number) AND given wave tables.  Every
//       tabulated state set, as a mask across the lanes, is stepped over every byte class with the core's step: the mask reached must
//       be, bit for bit, the node set of the state the table's row names, and must accept exactly when the table says so.
//       stdout: "ok STATES CLASSES W DEPTH"; a difference is exit code 5.
//   nfa_set_wave_emul match IMAGE.blob BATCH.bin
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  stdout: one result digit per string, then a newline.
//   Exit code 3: the image gets no wave tables (an epsilon cycle, more than 2048 nodes).
#include <string>

#include "emul_wave.h"
#include "wave_lanes.h"

using namespace mfa;
typedef emul::WaveHost P;

static int run_step(const HostImage& tab, const HostImage& set, const std::vector<std::string>& sets) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t W = set.set_tables[SET_H_WORDS];
    std::vector<uint32_t> stack(t.depth);                           // exactly the slots the kernel has: a sanitizer sees one more
    // state number -> mask: the table's own node set (bit v & 7 of byte v >> 3), lane v >> 5 bit v & 31
    auto mask_of = [&](uint32_t s) {
        P::Reg m = P::zero();
        for (uint32_t v = 0; v < tab.h.n_nodes; v++)
            if ((sets[s][v >> 3] >> (v & 7)) & 1) m.w[v >> 5] |= 1u << (v & 31u);
        return m;
    };
    if (sets.size() != tab.dfa_states) { fprintf(stderr, "%zu sets for %u states\n", sets.size(), tab.dfa_states); return 5; }
    const P::Reg begin = nfa_wave_start<P>(t);
    if (tab.dfa_states > 1) { const P::Reg one = mask_of(1); if (memcmp(&one, &begin, sizeof one) != 0) { fprintf(stderr, "state 1 is not {start}\n"); return 5; } }
    for (uint32_t s = 1; s < tab.dfa_states; s++) {
        const P::Reg from = mask_of(s);
        if (nfa_wave_accepts<P>(t, W, from) != (tab.dfa_accept[s] ? 1 : 0)) { fprintf(stderr, "state %u: accept differs\n", s); return 5; }
        for (uint32_t c = 0; c < tab.n_classes; c++) {
            P::Reg cur = from;
            const uint32_t alive = nfa_wave_step<P>(t, W, stack.data(), cur, c);
            const uint32_t to = tab.dfa_trans[(size_t)s * tab.n_classes + c];
            const P::Reg want = mask_of(to);
            if (alive > 1u || (alive == 0u) != (to == 0u) || memcmp(&cur, &want, sizeof cur) != 0) {
                fprintf(stderr, "state %u class %u: the step's set is not the set of the table's state %u\n", s, c, to);
                return 5;
            }
        }
    }
    printf("ok %u %u %u %u\n", tab.dfa_states, tab.n_classes, W, t.depth);
    return 0;
}

template <bool REV>
static int run_match(const HostImage& set, const std::vector<uint8_t>& file) {
    const NfaSetView t = nfa_set_view(set.set_tables.data(), set.set_tables.data());
    const uint32_t W = set.set_tables[SET_H_WORDS];
    std::vector<uint32_t> stack(t.depth);
    const emul::Batch batch = emul::read_batch(file);                            // exactly the library's read rule: ASan sees a byte beyond it
    std::string out;
    for (size_t k = 0; k + 1 < batch.off.size(); k++) out.push_back((char)('0' + nfa_wave_walk<REV, P>(t, W, stack.data(), batch.bytes, batch.off[k], batch.off[k + 1])));
    puts(out.c_str());
    free(batch.bytes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: nfa_set_wave_emul step IMAGE.blob | match IMAGE.blob BATCH.bin\n"); return 2; }
    const std::string mode = argv[1];
    HostImage tab, set;
    emul::load_wave(argv[2], set, &tab);
    if (mode == "step") {
        std::vector<std::string> sets;
        if (tabulate_nfa(tab, MFA_MAX_DFA_STATES, &sets) != MFA_OK) { fprintf(stderr, "not tabulated\n"); return 2; }
        return run_step(tab, set, sets);
    }
    if (mode == "match" && argc >= 4) {
        const std::vector<uint8_t> batch = emul::slurp(argv[3]);
        return set.h.is_reversed ? run_match<true>(set, batch) : run_match<false>(set, batch);
    }
    fprintf(stderr, "unknown mode\n");
    return 2;
}
