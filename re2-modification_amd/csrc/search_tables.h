// The two tables of the search inside lines (mfa_search_batch; search_core.h has the walks, search.hip the kernels), derived from a
// tabulated image's own table D (HostImage::dfa_trans, dfa_accept; state 0 dead, state 1 = {start}, F its accepting states) by ONE
// subset construction over sets of D's states with two switches:
//   post   step S' = { D(q, c) : q in S } \ {0}, plus {1} under `inject`; start {1}; accepting when S meets F   (without inject: D itself)
//   pre    step S' = { q : D(q, c) in S },      plus F  under `inject`; start F;    accepting when 1 is in S
// Pass 1 walks a line from its end down to its begin on an injecting table and so sees, at every position, whether SOME match begins
// there; pass 2 walks up from the leftmost such position on a plain table and sees whether THE match may end there:
//   image scan    pass 1          pass 2
//   forward       pre, inject     post, plain
//   is_reversed   post, inject    pre, plain
// Every set stands for walks of D from state 1, so the answer is mfa_match_batch's on the substring, whatever quirks D carries.
//
// Numbering: 0 the dead set, 1 the start set, accepting sets highest -- the walks' accept test is ONE compare of the pre-multiplied state
// against accept_from * kDfaRow.  A start set that accepts is the one exception: it keeps number 1, below accept_from, and start_accepts
// says so (the walks look at their first position through that flag); where other sets do not accept, the transitions that lead BACK to
// the start set go to a copy of it among the accepting ones, so that number 1 is entered by no byte.
// The format is D's: [states][n_classes] 16-bit entries over the image's byte classes, fused by dfa_fill_table (kDfaRow).
#ifndef MFA_SEARCH_TABLES_H
#define MFA_SEARCH_TABLES_H

#include <cstdint>
#include <vector>

namespace mfa {

struct HostImage;

static constexpr uint32_t kSearchMaxSets = 127;      // sets per table, the dead one and a copy of the start set included: what an LDS table holds

struct SearchTable {
    uint32_t              states = 0;          // 0: the image has no accepting state -- no table, no walk, every answer 0
    uint32_t              accept_from = 0;     // sets numbered accept_from and up accept (== states: only the start set may)
    uint32_t              start_accepts = 0;   // the start set, number 1, accepts
    std::vector<uint16_t> trans;               // [states][n_classes]
};

struct SearchTables {
    int         rc = 1;                        // 1: not built yet; MFA_OK; MFA_ERR_UNSUPPORTED: a table passed kSearchMaxSets
    SearchTable pass1, pass2;
};

// one table; MFA_ERR_UNSUPPORTED beyond kSearchMaxSets sets (the routine gives up at 128), or when D itself has more
int search_table_build(const HostImage& img, bool pre, bool inject, SearchTable& out);
// both tables of a tabulated image, by the rule above; sets and returns out.rc
int search_tables_build(const HostImage& img, SearchTables& out);

}  // namespace mfa

#endif
