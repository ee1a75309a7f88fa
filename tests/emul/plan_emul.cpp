// TEST INFRASTRUCTURE ONLY.  The launch planner (csrc/walk_plan.h, csrc/walk.h: pure functions, no HIP) on a machine without a GPU: reads
// cases from stdin, one per line, and prints what the library would launch as one JSON object per line (tests/test_walk_plan_cpu.py
// compares them with the plans recorded in tests/golden/plans/, and checks the layout's invariants).
//   walk  K max_live table_words reversed n n_cus regions n_seg seen quiet launches [ENV=value ...]
//   mixed K,max_live,words,words_wide[,memoryless,eligible,reversed,table_bytes];... seg_first,... n bytes sized calibrated ready,...|- cost,...|- [ENV=value ...]
// (`seen quiet launches`: the lean hint of the launch's slot; `sized` chooses an entry point of the library and is not used here: the
// caller resolves the bytes.  A mixed case is planned by plan_mixed, the function the library enqueues the result of.)
#include <cstdio>
#include <iostream>
#include <sstream>

#include "walk_plan.h"

using namespace mfa;

template <class T> static std::vector<T> list_of(const std::string& s) {
    std::vector<T> v;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, ',')) if (!t.empty() && t != "-") v.push_back((T)(sizeof(T) == sizeof(float) ? atof(t.c_str()) : strtoull(t.c_str(), nullptr, 10)));
    return v;
}
template <class V> static std::string arr(const V& v, size_t n) {
    std::ostringstream o;
    o << "[";
    for (size_t k = 0; k < n; k++) o << (k ? "," : "") << v[k];
    o << "]";
    return o.str();
}

// the pieces of a wave's block as [name, first word, words] triples, then the block's size
static void print_layout(const char* key, const WalkLayout& l) {
    printf(",\"%s\":{\"lds\":[[\"lv\",%u,%u],[\"ld\",%u,%u],[\"sb\",%u,%u],[\"sa\",%u,%u],[\"rtc\",%u,%u],[\"nm\",%u,%u]],\"lds_words\":%u,", key,
           l.lv(), 2u * l.C * l.W() * l.lanes, l.ld(), 2u * l.C * l.DW() * l.lanes, l.sb(), l.CI() * l.W() * l.lanes, l.sa(), l.CI() * l.DW() * l.lanes,
           l.rtc(), l.lean ? 0u : 2u * l.lanes * MFA_RT_CACHED, l.nm(), l.nm_words * l.lanes, l.lds_words());
    printf("\"spill\":[[\"gv\",%u,%u],[\"gd\",%u,%u],[\"gsb\",%u,%u],[\"gsa\",%u,%u],[\"gq\",%u,%u]],\"spill_used\":%u,\"spill_words\":%zu}",
           l.gv(), 2u * l.CX * l.W() * l.lanes, l.gd(), 2u * l.CX * l.DW() * l.lanes, l.gsb(), l.XI() * l.W() * l.lanes, l.gsa(), l.XI() * l.DW() * l.lanes,
           l.gq(), CMP_CACHE * 4u * l.lanes, l.spill_used(), l.spill_words());
}

static bool first_reversed(const std::vector<MixImage>& img) {
    for (const MixImage& i : img) if (!i.memoryless) return i.reversed;
    return false;
}

// "launches": the table engine's walk launches, "seg_walks": the per-segment engine's, [group, segment, a, b, stream, waits] each;
// "regions": [group, a, b, threads, signals] each
static void print_mixed(const MixPlan& P) {
    printf("{\"rc\":%d,\"table\":%d,\"cut\":%s,\"NW\":%d,\"where\":%s,\"launches\":[", P.rc, (int)P.table, arr(P.cut, P.cut.size()).c_str(), P.NW, arr(P.where, P.where.size()).c_str());
    for (size_t i = 0; i < P.walks.size() && P.table; i++) {
        const MixLaunch& L = P.walks[i];
        printf("%s{\"g\":%u,\"s0\":%u,\"s1\":%u,\"ml\":%u,\"Kc\":%u,\"w0\":%u,\"w1\":%u,\"a\":%llu,\"b\":%llu,\"k\":%d,\"sf\":%s,\"stb\":%s,\"slot\":%u,\"waits\":%d}", i ? "," : "", L.g, L.s0, L.s1, L.ml, L.Kc,
               L.w0, L.w1, (unsigned long long)L.a, (unsigned long long)L.b, L.k, arr(L.sf, L.s1 - L.s0 + 1).c_str(), arr(L.stb, L.s1 - L.s0).c_str(), L.slot, (int)L.waits);
    }
    printf("],\"direct\":%d,\"KD\":%d,\"NS\":%d,\"regions\":[", (int)P.direct, P.KD, P.NS);
    for (size_t i = 0; i < P.regions.size(); i++)
        printf("%s[%u,%llu,%llu,%u,%d]", i ? "," : "", P.regions[i].g, (unsigned long long)P.regions[i].a, (unsigned long long)P.regions[i].b, P.regions[i].threads, (int)P.regions[i].signals);
    printf("],\"own_event\":%s,\"seg_walks\":[", arr(P.own_event, P.direct || P.rc != MFA_OK ? 0 : P.n_groups).c_str());
    for (size_t i = 0; i < P.walks.size() && !P.table; i++) {
        const MixLaunch& L = P.walks[i];
        printf("%s[%u,%u,%llu,%llu,%d,%d]", i ? "," : "", L.g, L.s0, (unsigned long long)L.a, (unsigned long long)L.b, L.k, (int)L.waits);
    }
    printf("],\"dfa_items\":[");
    for (size_t i = 0; i < P.dfa.items.size(); i++) printf("%s[%u,%llu,%u]", i ? "," : "", P.dfa.items[i].image, (unsigned long long)P.dfa.items[i].first, P.dfa.items[i].count);
    printf("],\"dfa_own\":%s,\"dfa_chunks\":[", arr(P.dfa.own, P.dfa.own.size()).c_str());
    for (size_t i = 0; i < P.dfa_multi.size(); i++) printf("%s[%u,%u]", i ? "," : "", P.dfa_multi[i].first, P.dfa_multi[i].second);
    printf("],\"counts\":{\"region_launches\":%u,\"walk_launches\":%u,\"groups\":%u,\"dfa_multi\":%u,\"dfa_own\":%u,\"dfa_items\":%u,\"dfa_strings\":%llu,\"no_regions\":%d}}\n", P.n_regions, P.n_walks,
           P.n_groups, P.n_dfa_multi, P.n_dfa_own, P.n_dfa_items, (unsigned long long)P.dfa_strings, (int)P.no_regions);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream ss(line);
        std::string kind, e;
        ss >> kind;
        std::vector<std::string> envs;
        const auto set_env = [&]() { while (ss >> e) { envs.push_back(e.substr(0, e.find('='))); setenv(envs.back().c_str(), e.substr(e.find('=') + 1).c_str(), 1); } };
        if (kind == "walk") {
            uint32_t K, ml, tw, rev, n_seg, seen;
            uint64_t n;
            int n_cus, regions;
            LeanHint hint;
            ss >> K >> ml >> tw >> rev >> n >> n_cus >> regions >> n_seg >> seen >> hint.quiet >> hint.launches;
            set_env();
            // as launch_walk does: knobs, the lean decision, the plan; the hint moves on only when the launch could be planned
            const WalkKnobs kn = walk_knobs();
            Lean lean = regions && kn.accel && kn.lean != 0 ? Lean::on : Lean::off;
            LeanHint next = hint;
            const bool hinted = lean == Lean::on;
            if (hinted) lean = lean_decide(seen, next, kn);
            WalkLaunch L;
            int rc = plan_walk(WalkPlanInput{K, ml, rev != 0, tw}, kn, n, n_cus, n_seg, lean, L);
            if (rc == MFA_OK) { hint = next; if (!walk_has_kernel(L)) rc = MFA_ERR_UNSUPPORTED; }
            printf("{\"rc\":%d,\"quiet\":%u,\"launches\":%u", rc, hint.quiet, hint.launches);
            if (rc == MFA_OK) {
                const WalkArgs& a = L.args;
                const char* names[] = {"k", "long_k", "stats"};
                printf(",\"kernel\":\"%s%s\",\"C\":%u,\"CX\":%u,\"nm_words\":%u,\"table_words\":%u,\"shared_words\":%u,\"tables_global\":%d,\"images_global\":%u,\"accel\":%u,\"refill\":%u,"
                       "\"n_seg\":%u,\"reversed\":%d,\"grid\":%u,\"lds_bytes\":%zu", names[(int)L.kernel], L.kernel == WalkKernel::stats ? "" : std::to_string(L.K).c_str(), a.C, a.CX,
                       a.nm_words, a.table_words, a.shared_words, (int)L.tables_global, a.images_global, a.accel, a.refill, a.n_seg, (int)L.reversed, L.grid, L.lds_bytes);
                const bool lg = L.lean_grid != 0u;
                printf(",\"lean_grid\":%u,\"lean_C\":%u,\"lean_CX\":%u,\"lean_lds_bytes\":%zu,\"queue_at\":%lld,\"lean_seen\":%d,\"reserve_bytes\":%zu,\"counter_words\":%u",
                       L.lean_grid, lg ? L.lean_C : 0u, lg ? L.lean_CX : 0u, lg ? L.lean_lds_bytes : (size_t)0, lg ? (long long)L.queue_at : -1ll, hinted ? 1 : 0, L.spill_bytes, L.counter_words);
                print_layout("layout", WalkLayout{L.K, a.C, a.CX, a.images_global != 0u, false, a.nm_words});
                print_layout("lean_layout", WalkLayout{L.K, L.lean_C, L.lean_CX, false, true, a.nm_words});
            }
            printf("}\n");
        } else if (kind == "mixed") {
            std::string imgs, sfs, readys, costs;
            uint64_t n;
            double bytes;
            int sized, calibrated;
            ss >> imgs >> sfs >> n >> bytes >> sized >> calibrated >> readys >> costs;
            set_env();
            // the object's facts as mfa_mixed_create gathers them.  Tables: the memory automata's blocks back to back, in the wide format (3-word
            // edges) for automata of up to 6 cells when the object has one of more than 6; one scan direction, or no table engine
            std::vector<MixImage> img;
            std::vector<uint32_t> block_words[2];
            MixObject ob{1u, 0u, 0u, 0u, true};
            std::stringstream is(imgs);
            for (std::string t; std::getline(is, t, ';');) {
                auto v = list_of<uint64_t>(t);
                v.resize(8, 0);
                img.push_back(MixImage{(uint32_t)v[0], (uint32_t)v[1], 0u, v[4] != 0, v[4] != 0 && v[5] != 0, v[6] != 0, (uint32_t)v[7]});
                block_words[0].push_back((uint32_t)v[2]); block_words[1].push_back((uint32_t)v[3]);
                if (img.back().memoryless) { ob.n_dfa++; continue; }
                if (ob.n_mem++ != 0 && img.back().reversed != first_reversed(img)) ob.table_ok = false;
                ob.K = std::max(ob.K, img.back().K);
            }
            for (size_t k = 0; k < img.size() && ob.table_ok; k++) {
                img[k].block_at = ob.total_words;
                if (!img[k].memoryless) ob.total_words += block_words[ob.K > 6 && img[k].K <= 6 ? 1 : 0][k];
            }
            const std::vector<uint64_t> seg_first = list_of<uint64_t>(sfs);
            const std::vector<float> ready = list_of<float>(readys), cost = list_of<float>(costs);
            std::vector<float> r(MIX_MAX_GROUPS, 0.0f), c(img.size(), 0.0f);
            for (size_t k = 0; k < r.size() && k < ready.size(); k++) r[k] = ready[k];
            for (size_t k = 0; k < c.size() && k < cost.size(); k++) c[k] = cost[k];
            // calibrated = 1: the call after the calibrating one, on the same batch (2: after one with another number of groups)
            const MixKnobs kn = mixed_knobs();
            MixPlan P = plan_mixed(img, ob, seg_first.data(), n, (uint64_t)bytes, kn, MixCalib{false, 0u, r.data(), c.data()});
            if (calibrated) P = plan_mixed(img, ob, seg_first.data(), n, (uint64_t)bytes, kn, MixCalib{true, P.n_groups + (calibrated == 2 ? 1u : 0u), r.data(), c.data()});
            print_mixed(P);
        } else { fprintf(stderr, "plan_emul: unknown case '%s'\n", kind.c_str()); return 2; }
        for (const std::string& k : envs) unsetenv(k.c_str());
    }
    return 0;
}
