// TEST INFRASTRUCTURE ONLY: the search inside lines (csrc/search_core.h) run one lane at a time on the tables csrc/search_tables.cpp
// derives, in the order search.hip's two passes use them.
//   search_emul run IMAGE.blob BATCH.bin [check]
//       BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes.  stdout, binary: results[n], u64 spans[2n + 1], span_results[2n] --
//       what mfa_search_batch leaves.  check: every line also against a brute force that walks the image's own table D from every
//       begin (a reversed image: down from every end) until dead, and shares no code with the subset construction; a difference is exit 5.
//   search_emul info IMAGE.blob
//       stdout, one line per pass: states accept_from start_accepts enters_start row0_dead
//       (enters_start: some transition leads to set 1; row0_dead: every transition of set 0 leads to set 0).  exit 3: the image is refused.
//   search_emul plan STATES1 STATES2 N CUS
//       stdout: form1 lds1 lds2 grid1 grid2 per_cu1 per_cu2 tile_bytes
#include "emul_common.h"
#include "search_core.h"
#include "search_tables.h"

using namespace mfa;

static std::vector<uint16_t> fused(const HostImage& img, const SearchTable& t) {
    std::vector<uint16_t> next((size_t)t.states * kDfaRow, 0);
    dfa_fill_table(next.data(), t.trans.data(), img.byte_class, t.states, img.n_classes, 0u, 1u);
    return next;
}

struct Span { bool found; uint64_t i, j; };

// the definition, on D: the smallest i with a match [i, j), and for it the largest j
static Span brute(const HostImage& img, const uint8_t* bytes, uint64_t b, uint64_t e) {
    const uint32_t nc = img.n_classes;
    auto D = [&](uint32_t q, uint8_t c) { return img.dfa_trans[(size_t)q * nc + img.byte_class[c]]; };
    Span best{false, 0, 0};
    auto offer = [&](uint64_t i, uint64_t j) {
        if (!best.found || i < best.i || (i == best.i && j > best.j)) best = Span{true, i, j};
    };
    if (!img.h.is_reversed) {
        for (uint64_t i = b; i <= e && !best.found; i++) {
            uint32_t q = 1;
            if (img.dfa_accept[q]) offer(i, i);
            for (uint64_t p = i; p < e && q != 0; p++) {
                q = D(q, bytes[p]);
                if (img.dfa_accept[q]) offer(i, p + 1);
            }
        }
    } else {
        for (uint64_t j = b; j <= e; j++) {
            uint32_t q = 1;
            if (img.dfa_accept[q]) offer(j, j);
            for (uint64_t p = j; p > b && q != 0; p--) {
                q = D(q, bytes[p - 1]);
                if (img.dfa_accept[q]) offer(p - 1, j);
            }
        }
    }
    return best;
}

static int run(const char* image, const char* batch_path, bool check) {
    HostImage img;
    emul::load_memoryless(image, img);
    SearchTables tb;
    if (search_tables_build(img, tb) != MFA_OK) { fprintf(stderr, "%s: the search refuses this image\n", image); return 3; }
    const std::vector<uint16_t> next1 = fused(img, tb.pass1), next2 = fused(img, tb.pass2);
    const emul::Batch batch = emul::read_batch(emul::slurp(batch_path));
    const uint64_t n = batch.off.size() - 1;
    std::vector<uint8_t> results(n ? n : 1, 7), span_results(n ? 2 * n : 1, 7);
    std::vector<uint64_t> spans(2 * n + 1, ~0ull);
    spans[2 * n] = batch.off[n];
    // pass 1: search_pass1_*_kernel, one lane
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t b = batch.off[k];
        uint64_t e = batch.off[k + 1];
        const bool too_long = e - b > kSearchMaxLine;
        if (too_long || tb.pass1.states == 0) e = b;
        uint32_t last = (!too_long && tb.pass1.states != 0) ? search_first<true>(tb.pass1.start_accepts, b, e) : kSearchNone;
        (void)search_walk<true>(next1.data(), tb.pass1.accept_from * kDfaRow, batch.bytes, b, e, kDfaRow, &last);
        search_put_pass1(results.data(), spans.data(), k, b, too_long, last);
    }
    // pass 2: search_pass2_kernel, one lane
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t result = results[k];
        uint64_t i = 0;
        uint32_t last = 0;
        if (result == 1u) {
            i = spans[2 * k];
            (void)search_walk<false>(next2.data(), tb.pass2.accept_from * kDfaRow, batch.bytes, i, batch.off[k + 1], kDfaRow, &last);
        }
        search_put_pass2(spans.data(), span_results.data(), k, result, i, last);
    }
    if (check)
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t b = batch.off[k], e = batch.off[k + 1];
            if (e - b > kSearchMaxLine) continue;
            const Span w = brute(img, batch.bytes, b, e);
            const uint64_t wi = w.found ? w.i : b, wj = w.found ? w.j : b;
            if (results[k] != (w.found ? 1 : 0) || spans[2 * k] != wi || spans[2 * k + 1] != wj) {
                fprintf(stderr, "line %llu [%llu, %llu): brute force %d [%llu, %llu), the walks %d [%llu, %llu)\n", (unsigned long long)k, (unsigned long long)b,
                        (unsigned long long)e, (int)w.found, (unsigned long long)wi, (unsigned long long)wj, (int)results[k],
                        (unsigned long long)spans[2 * k], (unsigned long long)spans[2 * k + 1]);
                emul::fail("the walks differ from the definition");
            }
        }
    fwrite(results.data(), 1, n, stdout);
    fwrite(spans.data(), 8, 2 * n + 1, stdout);
    fwrite(span_results.data(), 1, 2 * n, stdout);
    free(batch.bytes);
    return 0;
}

static int info(const char* image) {
    HostImage img;
    emul::load_memoryless(image, img);
    SearchTables tb;
    if (search_tables_build(img, tb) != MFA_OK) return 3;
    for (const SearchTable* t : {&tb.pass1, &tb.pass2}) {
        bool enters = false, row0 = true, in_range = true;
        for (size_t x = 0; x < t->trans.size(); x++) {
            enters = enters || t->trans[x] == 1u;
            in_range = in_range && t->trans[x] < t->states;
            if (x < img.n_classes) row0 = row0 && t->trans[x] == 0u;
        }
        if (!in_range || t->trans.size() != (size_t)t->states * img.n_classes) emul::fail("a transition leaves the table");
        printf("%u %u %u %d %d\n", t->states, t->accept_from, t->start_accepts, (int)enters, (int)row0);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3], argc >= 5 && !strcmp(argv[4], "check"));
    if (argc >= 3 && !strcmp(argv[1], "info")) return info(argv[2]);
    if (argc >= 6 && !strcmp(argv[1], "plan")) {
        const uint32_t s1 = (uint32_t)strtoul(argv[2], nullptr, 10), s2 = (uint32_t)strtoul(argv[3], nullptr, 10);
        const uint64_t n = strtoull(argv[4], nullptr, 10), cus = strtoull(argv[5], nullptr, 10);
        const SearchPlan p = plan_search(s1, s2, n, cus);
        printf("%s %zu %zu %u %u %llu %llu %zu\n", p.form1 == SEARCH_TILED ? "tiled" : "untiled", p.lds1, p.lds2, p.grid1, p.grid2,
               (unsigned long long)lds_blocks_per_cu(p.lds1), (unsigned long long)lds_blocks_per_cu(p.lds2), kMemlessTileBytes);
        return 0;
    }
    fprintf(stderr, "usage: search_emul run IMAGE.blob BATCH.bin [check] | info IMAGE.blob | plan STATES1 STATES2 N CUS\n");
    return 2;
}
