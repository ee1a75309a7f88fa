// TEST INFRASTRUCTURE ONLY.  The walk kernel's own source (csrc/walk_core.h, csrc/walk_tables.cpp) compiled for the host as a
// wave of one lane, so that the step function, the table builder and the jump logic can be checked against the oracle on a
// machine without a GPU.  Not a fallback: nothing in re2-modification_amd/ or include/ builds, links or calls this.
//
//   walk_emul <image.blob> <C> <accel 0|1> [<image2.blob> <first string of segment 2> ...]  < strings (one per line)  > 0/1 per line
// With accel = 1 every string gets a region table computed here from the definition in include/mfa_hip.h (brute force).
// EMUL_FIELDS set: one more line on stderr (before the counters), "fields: c-cm n1 .. n9 c-com .. c-rdm .. b-cm .. b-com .. b-rdm ..":
// per cell 1..9, the effective edges of the FIRST image's tables that hold the cell in cm, com, rdm -- the vnodes' waiting lists (c) and
// byte-class lists (b) counted apart, decoded from the table words as the launch has them (walk_tables.h).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <algorithm>

#define MFA_HOST_EMUL 1
#define WALK_WV 1u
#define WALK_DEV inline
#include "walk_core.h"
#include "walk_tables.h"
#include "emul_common.h"

using namespace mfa;
using namespace mfa_walk;

// region table of one string, from the definition: maximal q-periodic regions (q <= 8) of at least MFA_REGION_MIN_LEN bytes, those
// covered by a region of a proper divisor period dropped, the 15 longest kept, sorted by start
static void region_row(const uint8_t* s, uint32_t len, uint64_t* row) {
    struct R { uint32_t lo, hi, q; };
    std::vector<R> all;
    for (uint32_t q = 1; q <= 8; q++) {
        if (len <= q) continue;
        uint32_t a = 0;
        while (a + q < len) {
            if (s[a] != s[a + q]) { a++; continue; }
            uint32_t b = a;
            while (b + q < len && s[b] == s[b + q]) b++;
            if (b + q - a >= MFA_REGION_MIN_LEN) all.push_back(R{a, b + q, q});
            a = b + 1;
        }
    }
    std::vector<R> keep;
    for (const R& r : all) {
        bool covered = false;
        for (const R& d : all)
            if (d.q < r.q && r.q % d.q == 0 && d.lo <= r.lo && d.hi >= r.hi) covered = true;
        if (!covered) keep.push_back(r);
    }
    bool overflow = false;
    if (keep.size() > MFA_REGION_MAX) {
        std::sort(keep.begin(), keep.end(), [](const R& x, const R& y) { return x.hi - x.lo > y.hi - y.lo; });
        keep.resize(MFA_REGION_MAX);
        overflow = true;
    }
    std::sort(keep.begin(), keep.end(), [](const R& x, const R& y) { return x.lo < y.lo || (x.lo == y.lo && x.q < y.q); });
    for (uint32_t k = 0; k < MFA_REGION_WORDS; k++) row[k] = 0;
    row[0] = keep.size() | (overflow ? MFA_REGION_OVERFLOW : 0ull);
    for (size_t k = 0; k < keep.size(); k++) row[1 + k] = (uint64_t)keep[k].lo | ((uint64_t)keep[k].hi << 24) | ((uint64_t)keep[k].q << 48);
}

struct QueueSeqFeeder {                       // the lean walk's strings: the queue the first pass filled
    const uint32_t* queue; uint32_t count, next = 0;
    bool take(bool want, uint64_t& sid) {
        if (!want || next >= count) return false;
        sid = queue[next++];
        return true;
    }
};

struct SeqFeeder {
    uint64_t next = 0, n = 0;
    bool take(bool want, uint64_t& sid) {
        if (!want || next >= n) return false;
        sid = next++;
        return true;
    }
};

static void print_fields(const uint32_t* w) {
    const uint32_t n_vids = w[0], NC = w[2], off_vinfo = w[6], off_vc = w[7], off_vb = w[8], off_ee = w[9], eew = w[11];
    unsigned long long n[2][3][9] = {};
    auto count = [&](uint32_t list, int which) {
        for (uint32_t e = list >> 12; e < (list >> 12) + (list & 0xfffu); e++) {
            const uint32_t e1 = w[off_ee + e * eew + 1], e2 = eew == 3 ? w[off_ee + e * eew + 2] : 0u;
            const uint32_t f[3] = {eew == 2 ? (e1 >> 12) & 0x3fu : (e1 >> 18) & 0x1ffu, eew == 2 ? (e1 >> 18) & 0x3fu : e2 & 0x1ffu,
                                   eew == 2 ? (e1 >> 24) & 0x3fu : (e2 >> 9) & 0x1ffu};
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 9; c++) n[which][k][c] += (f[k] >> c) & 1u;
        }
    };
    for (uint32_t id = 0; id < n_vids; id++) {
        if (!(w[off_vinfo + id] & 1u)) continue;
        count(w[off_vc + id], 0);
        for (uint32_t c = 0; c < NC; c++) count(w[off_vb + id * NC + c], 1);
    }
    static const char* const names[2][3] = {{"c-cm", "c-com", "c-rdm"}, {"b-cm", "b-com", "b-rdm"}};
    fprintf(stderr, "fields:");
    for (int which = 0; which < 2; which++)
        for (int k = 0; k < 3; k++) {
            fprintf(stderr, " %s", names[which][k]);
            for (int c = 0; c < 9; c++) fprintf(stderr, " %llu", n[which][k][c]);
        }
    fprintf(stderr, "\n");
}

template <int K, bool REV>
static void run(const Batch& b, const std::vector<uint32_t>& T, uint32_t C, uint32_t CM, WaveStats* ws) {
    // one lane's blocks of LDS and of the spill area, laid out as the kernel's (walk.h); the node map (WALK_NODE_MAP builds) is the lane's
    const WalkLayout lay{(uint32_t)K, C, CM > C ? CM - C : 1u, false, false, (CM + 1u + 3u) / 4u, 1u};
    std::vector<uint32_t> lds(lay.lds_words() + 1u, 0xdeadbeefu), spill(lay.spill_words(), 0xdeadbeefu);
    Store st;
    st.C = lay.C; st.CX = lay.CX; st.CI = lay.CI();
    st.lv = &lds[lay.lv()]; st.ld = &lds[lay.ld()]; st.sb = &lds[lay.sb()]; st.sa = &lds[lay.sa()];
    st.nm = reinterpret_cast<uint8_t*>(&lds[lay.nm()]); st.nm_words = lay.nm_words;
    st.gv = &spill[lay.gv()]; st.gd = &spill[lay.gd()]; st.gsb = &spill[lay.gsb()]; st.gsa = &spill[lay.gsa()]; st.gq = &spill[lay.gq()];
    uint64_t rtc[MFA_RT_CACHED] = {0};
    SeqFeeder feed;
    feed.n = b.n;
    walk_wave<K, REV, SeqFeeder>(b, T.data(), st, rtc, feed, ws);
    if (b.lean_queue != nullptr && *b.lean_count != 0u) {      // the strings handed on: the plain step only (walk_core.h: walk_wave_lean)
        Store sl = st;
        sl.ld = nullptr; sl.sb = nullptr; sl.sa = nullptr; sl.gd = nullptr; sl.gsb = nullptr; sl.gsa = nullptr; sl.CI = 0;
        QueueSeqFeeder qf{b.lean_queue, *b.lean_count};
        Batch bl = b;
        bl.regions = nullptr; bl.accel = 0; bl.lean_queue = nullptr; bl.lean_count = nullptr;
        walk_wave_lean<K, REV, QueueSeqFeeder>(bl, T.data(), sl, qf);
    }
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: walk_emul image.blob C accel [image.blob first ...]\n"); return 2; }
    const uint32_t C = (uint32_t)atoi(argv[2]);
    const int accel = atoi(argv[3]);
    std::vector<uint32_t> T, seg_first, seg_table;
    uint32_t K = 1, CM = 1;
    bool rev = false;
    for (int a = 1; a < argc; a += (a == 1 ? 3 : 2)) {          // the launch's cell count: the largest of its automata's
        std::vector<uint8_t> blob = emul::slurp(argv[a]);
        HostImage img;
        if (parse_blob(blob.data(), blob.size(), img) != MFA_OK) { fprintf(stderr, "bad image %s\n", argv[a]); return 2; }
        K = std::max(K, (uint32_t)(img.h.n_cells ? img.h.n_cells : 1));
    }
    for (int a = 1; a < argc; a += (a == 1 ? 3 : 2)) {
        std::vector<uint8_t> blob = emul::slurp(argv[a]);
        HostImage img;
        if (parse_blob(blob.data(), blob.size(), img) != MFA_OK || check_mfa_invariants(img) != MFA_OK) { fprintf(stderr, "bad image %s\n", argv[a]); return 2; }
        WalkTables wt;
        if (build_walk_tables(img, wt, K > 6) != MFA_OK) { fprintf(stderr, "tables: unsupported %s\n", argv[a]); return 3; }
        seg_first.push_back(a == 1 ? 0u : (uint32_t)atoi(argv[a + 1]));
        seg_table.push_back((uint32_t)T.size());
        T.insert(T.end(), wt.words.begin(), wt.words.end());
        K = std::max(K, wt.K); CM = std::max(CM, wt.max_live);
        if (a == 1) rev = wt.reversed;
        else if (rev != wt.reversed) { fprintf(stderr, "segments of one launch must scan in the same direction\n"); return 2; }
    }
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off{0};
    {
        std::string line;
        int c;
        while ((c = getchar()) != EOF) {
            if (c == '\n') { bytes.insert(bytes.end(), line.begin(), line.end()); off.push_back(bytes.size()); line.clear(); }
            else line.push_back((char)c);
        }
    }
    const uint64_t n = off.size() - 1;
    seg_first.push_back((uint32_t)n);
    bytes.resize(bytes.size() + 64, 0);
    std::vector<uint8_t> res(n ? n : 1, 9);
    std::vector<uint64_t> table;
    if (accel) {
        table.resize(n * MFA_REGION_WORDS);
        for (uint64_t k = 0; k < n; k++) region_row(bytes.data() + off[k], (uint32_t)(off[k + 1] - off[k]), &table[k * MFA_REGION_WORDS]);
    }
    Batch b{bytes.data(), off.data(), n, res.data(), accel ? table.data() : nullptr, (uint32_t)(accel != 0), 1u, (uint32_t)seg_table.size(), seg_first.data(), seg_table.data(), 0u, nullptr, nullptr};
    std::vector<uint32_t> lean_queue(n ? n : 1);
    uint32_t lean_count = 0;
    if (accel && !getenv("EMUL_NO_LEAN")) { b.lean_queue = lean_queue.data(); b.lean_count = &lean_count; }
    WaveStats ws;
    if (n) {
#define GO(KK) do { if (rev) run<KK, true>(b, T, C, CM, &ws); else run<KK, false>(b, T, C, CM, &ws); } while (0)
        switch (K) { case 1: GO(1); break; case 2: GO(2); break; case 3: GO(3); break; case 4: GO(4); break; case 5: GO(5); break;
                     case 6: GO(6); break; case 7: GO(7); break; case 8: GO(8); break; default: GO(9); break; }
    }
    for (uint64_t k = 0; k < n; k++) { putchar('0' + res[k]); putchar('\n'); }
    fprintf(stderr, "emul: %u of the strings walked by the lean pass\n", lean_count);
    if (getenv("EMUL_FIELDS")) print_fields(T.data());
    fprintf(stderr, "emul: %llu strings, steps %llu, dual %llu, probes %llu, hits %llu, skipped %llu, spill-steps %llu\n", (unsigned long long)n, ws.steps, ws.dual,
            ws.probes, ws.hits, ws.skipped, ws.spills);
    if (getenv("EMUL_HIST")) { fprintf(stderr, "events: entries %llu edge-evals %llu inserts %llu search-iters %llu c-items %llu\n", g_ev[0], g_ev[1], g_ev[2], g_ev[3], g_ev[6]); for (int k = 0; k < 80; k++) if (ws.hist[k]) fprintf(stderr, " n=%d:%llu", k, ws.hist[k]); fprintf(stderr, "\n"); }
    return 0;
}
