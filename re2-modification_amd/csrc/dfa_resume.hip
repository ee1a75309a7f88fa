// Memory-less automata on strings that arrive in pieces (mfa_match_batch_resume), for gfx950: the kernels of kernels.hip with the
// state of every string read from and written back to a word of device memory instead of starting at {start} and ending in a result
// byte alone.  One string per lane.  Which state a piece is entered with, the error state, the walk of a piece and the answer of a
// state are in dfa_resume_core.h (checked on the CPU: tests/emul).  Three table forms:
//   dfa_resume_tiled_kernel   fused table in LDS beside the input tile of dfa_tiled_kernel (table + tile <= 64 KiB: up to 55 state sets)
//   dfa_resume_walk_kernel    fused table in LDS, input read by the lane itself (up to 127 state sets; MFA_DFA_KERNEL=simple: always)
//   dfa_resume_big_kernel     table in global memory, resident in L2 (up to 2^20 state sets)
// The SGPR-packed form of dfa_tiled_kernel (MFA_DFA_KERNEL=packed) has no resume twin: such a call takes the LDS form.
// A piece of split_min bytes or more on an LDS table is queued for the split path exactly as in kernels.hip (split_take); the fold
// behind it (dfa_split.hip: dfa_fold_resume_kernel) starts from the string's word and writes word and result.  On an L2 table the launcher
// takes dfa_spec.hip's twin of dfa_resume_big_kernel, which queues such pieces for the kernels of that file.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "mfa_internal.h"
#include "dfa_resume_core.h"

namespace mfa {

// What a lane does with string sid of [b, e): the state it enters with (`st`), whether it walks the piece (`walks`), and whether the
// split path has taken it (`taken`: the lane then leaves word and result alone).
struct ResumeEntry { uint32_t st; bool walks, taken; };

__device__ __forceinline__ ResumeEntry resume_begin(const uint32_t* states, uint32_t n_states, uint64_t sid, uint64_t b, uint64_t e, const SplitArgs& sp) {
    ResumeEntry r;
    r.st = resume_enter(states[sid], n_states, e - b);
    r.walks = resume_walks(r.st);
    r.taken = r.walks && sp.split_min != 0u && e - b >= sp.split_min && split_take(sp, sid);
    return r;
}

__device__ __forceinline__ void resume_end(uint32_t* states, uint8_t* results, const uint8_t* accept_tab, uint64_t sid, uint32_t st) {
    states[sid] = st;
    if (results != nullptr) results[sid] = resume_result(accept_tab, st);
}

template <bool REV>
__global__ void __launch_bounds__(256)
dfa_resume_walk_kernel(const uint16_t* __restrict__ trans, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ byte_class,
                       uint32_t n_states, uint32_t n_classes, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                       uint32_t* __restrict__ states, uint8_t* __restrict__ results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    uint16_t* s_next = reinterpret_cast<uint16_t*>(lds);             // [n_states][kDfaRow], entry = next_state * kDfaRow
    for (uint32_t k = threadIdx.x; k < n_states * 256u; k += blockDim.x) {
        const uint32_t st = k >> 8, b = k & 255u;
        s_next[st * kDfaRow + b] = (uint16_t)(trans[st * n_classes + byte_class[b]] * kDfaRow);
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < n; sid += stride) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        const ResumeEntry r = resume_begin(states, n_states, sid, b, e, sp);
        if (r.taken) continue;
        resume_end(states, results, accept_tab, sid, r.walks ? resume_piece<REV>(s_next, bytes, b, e, r.st) : r.st);
    }
}

// dfa_tiled_kernel (kernels.hip has the layout of the tile and why it looks as it does), table in LDS, with the state carried
static constexpr uint32_t kLine = 128;                   // MFA_DFA_LINE
static constexpr uint32_t kTileRow = kLine + 16;
static constexpr uint32_t kLineLanes = kLine / 16;
static constexpr uint32_t kFetches = kLineLanes;

template <bool REV>
__global__ void __launch_bounds__(256)
dfa_resume_tiled_kernel(const uint16_t* __restrict__ trans, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ byte_class,
                        uint32_t n_states, uint32_t n_classes, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                        uint32_t* __restrict__ states, uint8_t* __restrict__ results, const SplitArgs sp) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint8_t* tile = reinterpret_cast<uint8_t*>(lds) + wave * (64u * kTileRow);
    uint16_t* s_next = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(lds) + 4u * 64u * kTileRow);
    for (uint32_t k = threadIdx.x; k < n_states * 256u; k += blockDim.x) {
        const uint32_t st = k >> 8, b = k & 255u;
        s_next[st * kDfaRow + b] = (uint16_t)(trans[st * n_classes + byte_class[b]] * kDfaRow);
    }
    __syncthreads();
    const uint64_t total16 = (offsets[n] + 15u) & ~(uint64_t)15;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t w0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u; w0 < n; w0 += n_waves * 64u) {
        const uint64_t sid = w0 + lane;
        const bool have = sid < n;
        const uint64_t b = have ? offsets[sid] : 0;
        uint64_t e = have ? offsets[sid + 1] : 0;
        ResumeEntry r{0u, false, false};
        if (have) r = resume_begin(states, n_states, sid, b, e, sp);
        if (!r.walks || r.taken) e = b;           // dead, in error or queued for the split path: empty here
        uint64_t p = REV ? e : b;                 // forward: next byte to consume; reverse: one past it
        uint32_t st = r.walks ? r.st * kDfaRow : 0u;
        bool active = have && (REV ? p > b : p < e);
        if (__any(active)) {
        uint64_t line = (REV ? p - 1u : p) & ~(uint64_t)(kLine - 1u);
        uint4 v[kFetches];
        auto fetch = [&](uint64_t ln, bool act) {
#pragma unroll
            for (int k = 0; k < (int)kFetches; k++) {
                const int src = k * (int)(64u / kLineLanes) + (int)(lane / kLineLanes);
                const uint32_t lo = __shfl((uint32_t)ln, src), hi = __shfl((uint32_t)(ln >> 32), src);
                const int a = __shfl((int)act, src);
                const uint64_t addr = (((uint64_t)hi << 32) | lo) + (lane % kLineLanes) * 16u;
                v[k] = (a && addr < total16) ? split_load16(bytes, addr) : make_uint4(0, 0, 0, 0);
            }
        };
        fetch(line, active);
        for (;;) {
#pragma unroll
            for (int k = 0; k < (int)kFetches; k++) {
                const uint32_t src = (uint32_t)k * (64u / kLineLanes) + lane / kLineLanes;
                *reinterpret_cast<uint4*>(tile + src * kTileRow + (lane % kLineLanes) * 16u) = v[k];
            }
            __builtin_amdgcn_wave_barrier();
            const uint64_t p_next = REV ? line : line + kLine;
            fetch((REV ? p_next - 1u : p_next) & ~(uint64_t)(kLine - 1u), active && (REV ? p_next > b : p_next < e));
            const uint32_t lo_b = active ? (uint32_t)((REV ? (b > line ? b - line : 0) : p - line)) : 0u;
            const uint32_t hi_b = active ? (uint32_t)((REV ? p - line : (e - line < kLine ? e - line : kLine))) : 0u;
            const bool full = __all(!active || (lo_b == 0u && hi_b == kLine));
            if (full && __all(active)) {
#pragma unroll 1
                for (int q = 0; q < (int)kLineLanes; q++) {
                    const int qq = REV ? (int)kLineLanes - 1 - q : q;
                    const uint4 d = *reinterpret_cast<const uint4*>(tile + lane * kTileRow + (uint32_t)qq * 16u);
                    st = split_step16<REV>(s_next, st, d, 0u, 16u);
                }
            } else
#pragma unroll 1
            for (int q = 0; q < (int)kLineLanes; q++) {
                const int qq = REV ? (int)kLineLanes - 1 - q : q;
                const uint4 d = *reinterpret_cast<const uint4*>(tile + lane * kTileRow + (uint32_t)qq * 16u);
                const uint32_t l = lo_b > (uint32_t)qq * 16u ? lo_b - (uint32_t)qq * 16u : 0u;
                const uint32_t h = hi_b > (uint32_t)qq * 16u ? hi_b - (uint32_t)qq * 16u : 0u;
                if (active) st = split_step16<REV>(s_next, st, d, l < 16u ? l : 16u, h < 16u ? h : 16u);
            }
            __builtin_amdgcn_wave_barrier();
            if (active) p = p_next;
            if (!REV && p > e) p = e;
            active = have && st != 0u && (REV ? p > b : p < e);
            if (!__any(active)) break;
            line = (REV ? p - 1u : p) & ~(uint64_t)(kLine - 1u);
        }
        }
        if (have && !r.taken) resume_end(states, results, accept_tab, sid, r.walks ? st / kDfaRow : r.st);
    }
}

template <bool REV, class T>
__global__ void __launch_bounds__(256)
dfa_resume_big_kernel(const T* __restrict__ trans, const uint8_t* __restrict__ accept_tab, const uint8_t* __restrict__ byte_class, uint32_t n_states,
                      uint32_t n_classes, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                      uint32_t* __restrict__ states, uint8_t* __restrict__ results) {
    __shared__ uint8_t s_class[256];
    s_class[threadIdx.x] = byte_class[threadIdx.x];
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < n; sid += stride) {
        const uint64_t b = offsets[sid], e = offsets[sid + 1];
        const uint32_t st = resume_enter(states[sid], n_states, e - b);
        resume_end(states, results, accept_tab, sid, resume_walks(st) ? resume_piece_big<REV, T>(trans, s_class, n_classes, bytes, b, e, st) : st);
    }
}

// ---- launcher -------------------------------------------------------------------------------------
template <bool REV>
static int launch_resume_dir(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                             uint32_t* d_states, uint8_t* d_results, hipStream_t s) {
    uint64_t blocks = (n + 255) / 256;
    if (blocks == 0) blocks = 1;
    if ((size_t)img.dfa_states * kDfaRow > 0xffffu) {                               // beyond 16-bit pre-multiplied states: table in L2
        if (blocks > (uint64_t)ds.n_cus * 8) blocks = (uint64_t)ds.n_cus * 8;
        SplitLaunch sl;                                                              // long pieces: dfa_spec.hip, as in kernels.hip
        int rc = spec_begin(img, cx, n, s, &sl);
        if (rc != MFA_OK) return rc;
        HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_start, s));
        if (sl.args.split_min != 0u) {
            rc = spec_main(img, ds, sl, d_bytes, d_offsets, n, d_results, s, d_states, (unsigned)blocks);
            if (rc == MFA_OK) rc = spec_tail(img, ds, sl, d_bytes, d_offsets, d_results, s, d_states);
            if (rc != MFA_OK) return rc;
            HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_stop, s));
            return MFA_OK;
        }
        if (img.dfa_states <= 0xffffu)
            hipLaunchKernelGGL((dfa_resume_big_kernel<REV, uint16_t>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint16_t*)ds.d_dfa_trans, ds.d_dfa_accept,
                               ds.d_byte_class, img.dfa_states, img.n_classes, d_bytes, d_offsets, n, d_states, d_results);
        else
            hipLaunchKernelGGL((dfa_resume_big_kernel<REV, uint32_t>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint32_t*)ds.d_dfa_trans, ds.d_dfa_accept,
                               ds.d_byte_class, img.dfa_states, img.n_classes, d_bytes, d_offsets, n, d_states, d_results);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_stop, s));
        return MFA_OK;
    }
    SplitLaunch sl;
    int rc = split_begin(img, cx, n, s, &sl);
    if (rc != MFA_OK) return rc;
    const size_t table = (size_t)img.dfa_states * kDfaRow * sizeof(uint16_t), tile = 4 * 64 * kTileRow;
    const char* mode = getenv("MFA_DFA_KERNEL");                                     // "simple" selects the untiled walk, as in kernels.hip
    const bool tiled = !(mode && mode[0] == 's') && table + tile <= 64 * 1024;
    const size_t lds = tiled ? table + tile : table;
    uint64_t per_cu = (160u * 1024u) / (lds ? lds : 1);      // resident blocks a CU's LDS allows (at most 8: 32 waves)
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    if (blocks > (uint64_t)ds.n_cus * per_cu) blocks = (uint64_t)ds.n_cus * per_cu;
    auto kern = tiled ? dfa_resume_tiled_kernel<REV> : dfa_resume_walk_kernel<REV>;
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_start, s));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, s, (const uint16_t*)ds.d_dfa_trans, ds.d_dfa_accept, ds.d_byte_class, img.dfa_states,
                       img.n_classes, d_bytes, d_offsets, n, d_states, d_results, sl.args);
    HIP_TRY(hipGetLastError());
    rc = split_tail(img, ds, sl, d_bytes, d_offsets, d_results, s, d_states);
    if (rc != MFA_OK) return rc;
    HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_stop, s));
    return MFA_OK;
}

int launch_dfa_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint32_t* d_states, uint8_t* d_results, void* stream) {
    return img.h.is_reversed ? launch_resume_dir<true>(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, (hipStream_t)stream)
                             : launch_resume_dir<false>(img, ds, cx, d_bytes, d_offsets, n, d_states, d_results, (hipStream_t)stream);
}

}  // namespace mfa
