// search_tables.h: the subset construction over sets of the tabulated table's states.  Host only, pure: no HIP call, no lock (the C-ABI
// holds the image's lock around it), nothing of the reference's stepping restated -- every step is a look into HostImage::dfa_trans.
#include "search_tables.h"

#include <map>
#include <utility>

#include "mfa_internal.h"

namespace mfa {

namespace {

// a set of D's states: bit q of 128 (D has at most kSearchMaxSets states here)
struct Set128 {
    uint64_t w[2] = {0, 0};
    void add(uint32_t q) { w[q >> 6] |= 1ull << (q & 63u); }
    bool has(uint32_t q) const { return (w[q >> 6] >> (q & 63u)) & 1ull; }
    bool meets(const Set128& o) const { return ((w[0] & o.w[0]) | (w[1] & o.w[1])) != 0; }
    bool empty() const { return (w[0] | w[1]) == 0; }
    void join(const Set128& o) { w[0] |= o.w[0]; w[1] |= o.w[1]; }
    bool operator<(const Set128& o) const { return w[1] != o.w[1] ? w[1] < o.w[1] : w[0] < o.w[0]; }
};

}  // namespace

int search_table_build(const HostImage& img, bool pre, bool inject, SearchTable& out) {
    out = SearchTable{};
    const uint32_t n = img.dfa_states, nc = img.n_classes;
    if (n < 2 || n > kSearchMaxSets || nc == 0 || img.dfa_trans.size() != (size_t)n * nc) return MFA_ERR_UNSUPPORTED;
    Set128 F, one;
    one.add(1);
    for (uint32_t q = 1; q < n; q++)
        if (img.dfa_accept[q]) F.add(q);
    if (F.empty()) return MFA_OK;                                       // nothing is ever found: no table
    const Set128 first = pre ? F : one;
    auto step = [&](const Set128& S, uint32_t c) {
        Set128 T;
        for (uint32_t q = 1; q < n; q++) {
            const uint32_t t = img.dfa_trans[(size_t)q * nc + c];
            if (pre) { if (t != 0 && S.has(t)) T.add(q); }
            else if (S.has(q) && t != 0) T.add(t);
        }
        if (inject) T.join(first);
        return T;
    };
    auto accepts = [&](const Set128& S) { return pre ? S.has(1) : S.meets(F); };

    // in the order they are met: 0 the dead set, 1 the start set
    std::map<Set128, uint32_t> ids;
    std::vector<Set128> sets{Set128{}, first};
    ids[sets[0]] = 0; ids[first] = 1;
    std::vector<uint32_t> raw;                                          // [met order][class]
    for (size_t s = 0; s < sets.size(); s++)
        for (uint32_t c = 0; c < nc; c++) {
            const Set128 t = step(sets[s], c);
            auto it = ids.find(t);
            if (it == ids.end()) {
                if (sets.size() >= kSearchMaxSets) return MFA_ERR_UNSUPPORTED;
                it = ids.emplace(t, (uint32_t)sets.size()).first;
                sets.push_back(t);
            }
            raw.push_back(it->second);
        }

    // the numbering: 0, 1, the sets that do not accept, the sets that do
    uint32_t m = (uint32_t)sets.size();
    std::vector<uint8_t> acc(m, 0);
    for (uint32_t s = 1; s < m; s++) acc[s] = accepts(sets[s]) ? 1 : 0;
    out.start_accepts = acc[1];
    bool others_all_accept = true, start_entered = false;
    for (uint32_t s = 2; s < m; s++) others_all_accept = others_all_accept && acc[s];
    for (uint32_t t : raw) start_entered = start_entered || t == 1u;
    if (acc[1] && !others_all_accept) {
        // number 1 stays below accept_from; what leads back to the start set goes to a copy of it among the accepting sets
        if (start_entered) {
            if (m >= kSearchMaxSets) return MFA_ERR_UNSUPPORTED;
            for (uint32_t& t : raw)
                if (t == 1u) t = m;
            for (uint32_t c = 0; c < nc; c++) raw.push_back(raw[(size_t)nc + c]);
            acc.push_back(1);
            m++;
        }
        acc[1] = 0;
    }
    std::vector<uint32_t> number(m, 0);
    uint32_t next = 2;
    number[1] = 1;
    for (uint32_t s = 2; s < m; s++)
        if (!acc[s]) number[s] = next++;
    out.accept_from = acc[1] ? 1u : next;                               // (an accepting start set with nothing but accepting sets behind it: from 1 on)
    for (uint32_t s = 2; s < m; s++)
        if (acc[s]) number[s] = next++;
    out.states = m;
    out.trans.assign((size_t)m * nc, 0);
    for (uint32_t s = 0; s < m; s++)
        for (uint32_t c = 0; c < nc; c++) out.trans[(size_t)number[s] * nc + c] = (uint16_t)number[raw[(size_t)s * nc + c]];
    return MFA_OK;
}

int search_tables_build(const HostImage& img, SearchTables& out) {
    out.pass1 = SearchTable{}; out.pass2 = SearchTable{};
    const bool rev = img.h.is_reversed != 0;
    int rc = img.h.kind != MFA_KIND_NFA || img.set_walk ? MFA_ERR_UNSUPPORTED : search_table_build(img, !rev, true, out.pass1);
    if (rc == MFA_OK) rc = search_table_build(img, rev, false, out.pass2);
    out.rc = rc;
    return rc;
}

}  // namespace mfa
