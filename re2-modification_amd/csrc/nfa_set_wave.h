// What the wave kernels of nfa_set_wave.hip and nfa_set_wave_split.hip share: the LDS layout -- the stacks of the four waves of a block,
// `depth` slots of 4 bytes each, and behind them the automaton's tables when both fit 64 KiB -- its size on the host, and what a launch
// asks of the image before anything is enqueued.
#ifndef MFA_NFA_SET_WAVE_H
#define MFA_NFA_SET_WAVE_H

#include "nfa_set.h"
#include "nfa_set_wave_core.h"

namespace mfa {

// what a block takes of LDS: the four stacks and, when both fit kSetLdsMax, the tables behind them (set_lds_of; `stack_words` is 4 * depth)
static_assert((size_t)4u * kWaveMaxNodes * 4u <= kSetLdsMax, "the stacks alone fit (a chain is never longer than the image has nodes)");

// wave tables on the device, of a width and depth the kernels hold
inline bool wave_tables_ok(const HostImage& img, const DeviceState& ds) {
    if (!img.set_wave || !ds.d_set_tables || img.set_tables.size() < SET_H_SIZE) return false;
    const uint32_t W = img.set_tables[SET_H_WORDS];
    return W >= 1u && W <= kWaveLanes && W == wave_words_of(img.set_tables[SET_H_NODES]) && img.set_tables[SET_H_DEPTH] <= kWaveMaxNodes;
}

// direction and the tables' place as template arguments of FN
#define MFA_WAVE_DISPATCH(FN, in_lds, ...)                                                                                                  \
    (img.h.is_reversed ? ((in_lds) ? FN<true, true>(__VA_ARGS__) : FN<true, false>(__VA_ARGS__))                                            \
                       : ((in_lds) ? FN<false, true>(__VA_ARGS__) : FN<false, false>(__VA_ARGS__)))

#ifdef __HIPCC__
// all 256 lanes of a block: where the tables' sections are read from -- their copy behind the four stacks, made here, or global memory.
// IN_LDS is a template parameter of every kernel, so that the compiler knows the address space of every table read.
template <bool IN_LDS>
__device__ __forceinline__ const uint32_t* wave_tables_base(uint32_t* lds, const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t depth) {
    if (!IN_LDS) return tables;
    uint32_t* copy = lds + 4u * depth;
    for (uint32_t k = threadIdx.x; k < table_words; k += 256u) copy[k] = tables[k];
    __syncthreads();
    return copy;
}
#endif

}  // namespace mfa

#endif
