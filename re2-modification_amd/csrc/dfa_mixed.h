// The multi-table launch for the memory-less segments of a mixed call (dfa_mixed.hip); the plan is walk_plan.h's plan_dfa_items.
#ifndef MFA_DFA_MIXED_H
#define MFA_DFA_MIXED_H

#include <cstdint>
#include <vector>

#include "dfa_mixed_core.h"
#include "walk_plan.h"

namespace mfa {

// the plan's items [i0, i1) (at most kDfaMaxItems) in one launch, asynchronous on `stream`; n: strings of the whole batch
int launch_dfa_mixed(const DfaPlan& plan, size_t i0, size_t i1, const uint8_t* d_tables, int n_cus, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                     uint8_t* d_results, void* stream);

}  // namespace mfa

#endif
