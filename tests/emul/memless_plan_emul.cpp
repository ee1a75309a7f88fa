// TEST INFRASTRUCTURE ONLY.  The planner of a call on one memory-less automaton (csrc/memless_plan.h: plan_memless_engine, plan_split,
// persistent_grid; pure, no HIP) on a machine without a GPU: reads cases from stdin, one per line, and prints one JSON object per line
// (tests/test_memless_plan_cpu.py checks them against the constants).
//   engine states classes set_walk set_wave set_words set_depth resume n n_cus [ENV=value ...]
//   split  scheme n seen,seen,... [ENV=value ...]      scheme: lds<lanes_log2> | none | l2 | set | wave; seen: the pinned word each call of
//                                                      ONE workspace reads, in order ("-": there is no pinned word)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "memless_plan.h"

using namespace mfa;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream ss(line);
        std::string what, e;
        ss >> what;
        if (what == "engine") {
            unsigned long long v[9];
            for (auto& x : v) ss >> x;
            std::vector<std::string> envs;
            while (ss >> e) { envs.push_back(e.substr(0, e.find('='))); setenv(envs.back().c_str(), e.substr(e.find('=') + 1).c_str(), 1); }
            const MemlessImage im{(uint32_t)v[0], (uint32_t)v[1], v[2] != 0, v[3] != 0, (uint32_t)v[4], (uint32_t)v[5]};
            const EnginePlan p = plan_memless_engine(im, v[6] != 0, memless_knobs(), v[7], v[8]);
            static const char* names[] = {"unsupported", "packed", "tiled", "untiled", "l2", "set_lane", "set_wave"};
            printf("{\"engine\":\"%s\",\"lds\":%zu,\"per_cu\":%llu,\"grid\":%u}\n", names[p.engine], p.lds, (unsigned long long)p.per_cu, p.grid);
            for (const std::string& k : envs) unsetenv(k.c_str());
        } else if (what == "split") {
            std::string scheme, seens;
            unsigned long long n;
            ss >> scheme >> n >> seens;
            std::vector<std::string> envs;
            while (ss >> e) { envs.push_back(e.substr(0, e.find('='))); setenv(envs.back().c_str(), e.substr(e.find('=') + 1).c_str(), 1); }
            const bool lds = scheme.compare(0, 3, "lds") == 0 && scheme.size() > 3;
            if (!lds && scheme != "none" && scheme != "l2" && scheme != "set" && scheme != "wave") { fprintf(stderr, "memless_plan_emul: no scheme '%s'\n", scheme.c_str()); return 2; }
            const SplitScheme sc = lds ? split_scheme_lds((uint32_t)atoi(scheme.c_str() + 3)) : scheme == "none" ? kSplitSchemeNone : scheme == "l2" ? kSplitSchemeL2
                                   : scheme == "set" ? kSplitSchemeSet : kSplitSchemeWave;
            SplitWorkspace ws{false, 0, false, 0};
            printf("{\"flags\":[%d,%d,%d],\"calls\":[", sc.tail != TAIL_SET, sc.tail == TAIL_SPEC, sc.tail == TAIL_SET);      // split_ran, spec_ran, set_split_ran
            std::stringstream sv(seens);
            bool first = true;
            for (std::string t; std::getline(sv, t, ',');) {
                ws.has_word = t != "-";
                ws.seen = ws.has_word ? (uint32_t)strtoul(t.c_str(), nullptr, 10) : 0u;
                const SplitPlan p = plan_split(sc, memless_knobs(), n, ws);      // (the knobs are read again for every call, as the library does)
                printf("%s{\"split_min\":%llu,\"tail\":%d,\"chunk_min\":%u,\"arena\":%u,\"map_cap\":%u,\"rounds\":%u,\"lookback\":%u,\"queue_at\":%zu,\"arena_at\":%zu,\"bytes\":%zu,"
                       "\"keep\":%d,\"quiet\":%u}", first ? "" : ",", (unsigned long long)p.split_min, (int)p.tail, p.chunk_min, p.arena_chunks, p.map_cap, p.rounds, p.lookback,
                       p.queue_at, p.arena_at, p.bytes, (int)p.keep, p.quiet);
                ws.keep = p.keep; ws.quiet = p.quiet;
                first = false;
            }
            printf("]}\n");
            for (const std::string& k : envs) unsetenv(k.c_str());
        } else { fprintf(stderr, "memless_plan_emul: no case '%s'\n", what.c_str()); return 2; }
    }
    return 0;
}
