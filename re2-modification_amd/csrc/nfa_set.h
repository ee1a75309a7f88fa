// What the set-walk kernels of nfa_set.hip and nfa_set_split.hip share: the LDS layout -- the stacks of the 256 lanes, [slot][lane], and
// behind them the automaton's tables when both fit 64 KiB -- its size on the host, and the one-time permission for that much dynamic LDS.
#ifndef MFA_NFA_SET_H
#define MFA_NFA_SET_H

#include <atomic>

#include "mfa_internal.h"
#include "nfa_set_core.h"

namespace mfa {

static_assert((size_t)kSetMaxDepth * 256u * 4u <= kSetLdsMax, "the stacks alone fit (nfa_set_build holds an image to kSetMaxDepth)");

// (memless_plan.h has the rule: set_lds, and kSetLdsMax)
inline SetLds set_lds_of(const HostImage& img) { return set_lds((uint32_t)img.set_tables.size(), img.set_tables[SET_H_DEPTH], img.set_wave); }
inline MemlessImage set_image(const HostImage& img) { return MemlessImage{0, 0, true, img.set_wave, (uint32_t)img.set_tables.size(), img.set_tables[SET_H_DEPTH]}; }

// the mask width W of a lane image (1, 2, 4, 8 words) and its direction, as template arguments of FN
#define MFA_SET_DISPATCH(FN, ...)                                                                                      \
    switch (img.set_tables[SET_H_WORDS]) {                                                                             \
        case 1: return img.h.is_reversed ? FN<true, 1>(__VA_ARGS__) : FN<false, 1>(__VA_ARGS__);                       \
        case 2: return img.h.is_reversed ? FN<true, 2>(__VA_ARGS__) : FN<false, 2>(__VA_ARGS__);                       \
        case 4: return img.h.is_reversed ? FN<true, 4>(__VA_ARGS__) : FN<false, 4>(__VA_ARGS__);                       \
        case 8: return img.h.is_reversed ? FN<true, 8>(__VA_ARGS__) : FN<false, 8>(__VA_ARGS__);                       \
    }                                                                                                                  \
    return MFA_ERR_UNSUPPORTED

// per kernel and device, once; images hold different locks, so the flags are atomic (two first launches at once both set it)
template <auto KERN>
inline int set_allow_lds(int device) {
    static std::atomic<bool> lds_allowed[64];
    const bool tracked = device >= 0 && device < 64;
    if (!tracked || !lds_allowed[device].load(std::memory_order_acquire)) {
        HIP_TRY(hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSetLdsMax));
        if (tracked) lds_allowed[device].store(true, std::memory_order_release);
    }
    return MFA_OK;
}

#ifdef __HIPCC__
// all 256 lanes of a block: where the tables' sections are read from -- their copy behind the stacks, made here, or global memory
__device__ __forceinline__ const uint32_t* set_tables_base(uint32_t* lds, const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t stack_words,
                                                           uint32_t tables_in_lds) {
    if (!tables_in_lds) return tables;
    uint32_t* copy = lds + stack_words;
    for (uint32_t k = threadIdx.x; k < table_words; k += 256u) copy[k] = tables[k];
    __syncthreads();
    return copy;
}
#endif

}  // namespace mfa

#endif
