// TEST INFRASTRUCTURE ONLY.  The planner of a mixed call's memory-less segments (csrc/walk_plan.h: plan_dfa_items, pure, no HIP) on a
// machine without a GPU: reads cases from stdin, one per line, and prints the plan as one JSON object per line
// (tests/test_mixed_dfa_plan_cpu.py checks its invariants).
//   seg_first,... memoryless,eligible,reversed,table_bytes;... table_schedule [ENV=value ...]
#include <cstdio>
#include <iostream>
#include <sstream>

#include "walk_plan.h"

using namespace mfa;

static std::vector<uint64_t> list_of(const std::string& s, char sep) {
    std::vector<uint64_t> v;
    std::stringstream ss(s);
    std::string t;
    while (std::getline(ss, t, sep)) if (!t.empty()) v.push_back(strtoull(t.c_str(), nullptr, 10));
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream ss(line);
        std::string sfs, imgs, e;
        int table_schedule;
        ss >> sfs >> imgs >> table_schedule;
        std::vector<std::string> envs;
        while (ss >> e) { envs.push_back(e.substr(0, e.find('='))); setenv(envs.back().c_str(), e.substr(e.find('=') + 1).c_str(), 1); }
        const std::vector<uint64_t> seg_first = list_of(sfs, ',');
        std::vector<DfaImage> img;
        std::stringstream is(imgs);
        for (std::string t; std::getline(is, t, ';');) {
            const std::vector<uint64_t> v = list_of(t, ',');
            img.push_back(DfaImage{v[0] != 0, v[1] != 0, v[2] != 0, (uint32_t)v[3]});
        }
        if (seg_first.size() != img.size() + 1) { fprintf(stderr, "dfa_plan_emul: %zu images need %zu segment borders\n", img.size(), img.size() + 1); return 2; }
        const DfaKnobs kn = dfa_knobs();
        const DfaPlan P = plan_dfa_items(seg_first.data(), img, table_schedule != 0, kn);
        printf("{\"multi\":%d,\"own_min\":%llu,\"items\":[", (int)kn.multi, (unsigned long long)kn.own_min);
        for (size_t i = 0; i < P.items.size(); i++) printf("%s[%u,%llu,%u]", i ? "," : "", P.items[i].image, (unsigned long long)P.items[i].first, P.items[i].count);
        printf("],\"own\":[");
        for (size_t i = 0; i < P.own.size(); i++) printf("%s%u", i ? "," : "", P.own[i]);
        printf("],\"table_bytes\":%u,\"strings\":%llu,\"slices\":%llu,\"launches\":%zu,\"wg\":[", P.table_bytes, (unsigned long long)P.strings, (unsigned long long)P.slices,
               (P.items.size() + kDfaMaxItems - 1) / kDfaMaxItems);
        // the slices of 7 workgroups: they tile [0, slices)
        for (uint32_t w = 0; w <= 7; w++) printf("%s%llu", w ? "," : "", (unsigned long long)dfa_slice_lo(P.slices, w, 7));
        printf("]}\n");
        for (const std::string& k : envs) unsetenv(k.c_str());
    }
    return 0;
}
