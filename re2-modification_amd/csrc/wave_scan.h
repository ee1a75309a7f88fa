// The inclusive prefix sum of a 64-bit value over the 64 lanes of a wave: what the scan passes of text_split.hip and select.hip share.
#ifndef MFA_WAVE_SCAN_H
#define MFA_WAVE_SCAN_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfa {

__device__ __forceinline__ uint64_t wave_scan_incl(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

}  // namespace mfa

#endif
