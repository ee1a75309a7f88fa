// Long strings of WAVE images (257 to 2048 nodes, or any set-walk image under MFA_SET_WAVE=1), cut across the whole GPU (gfx950).  The
// kernels of nfa_set_wave.hip walk one string per wave at a few thousand bytes per second, so one string of 64 KiB holds a call for
// seconds while the other resident waves idle.  Here a string with len >= split_min is cut into chunks and every chunk is walked from
// ONE set -- a guess -- by a WAVE of its own; wrong guesses are repaired a bounded number of times, then resolved exactly
// (nfa_set_wave_split_core.h has the scheme and is checked on the CPU: tests/emul/nfa_set_wave_split_emul.cpp).  It is the scheme of
// nfa_set_split.hip with a wave where that one has a lane and the wide record (mfa_set_state_wide, 68 words) where that one has the
// 48-byte record.  Queue, plan, chunk geometry and the shared knobs are dfa_split.hip's:
//   memset(header) -> nfa_set_wave_kernel / nfa_set_wave_resume_kernel (queue long strings: split_take) -> dfa_plan_kernel
//     -> nfa_set_wave_chunk_kernel -> MFA_SET_SPLIT_ROUNDS x nfa_set_wave_repair_kernel -> nfa_set_wave_resolve_kernel
// all on the caller's stream, with no read-back; the number of launches is fixed when the call is enqueued.  Successive launches on one
// stream are the only ordering: no kernel here spins or waits for another workgroup, every loop is bounded by a chunk's or a string's bytes.
// Records: per chunk start_used and TWO ends, 3 x 272 = 816 bytes of arena, each moved as one coalesced row of 64 words and one 16-byte
// tag quarter (vector loads and stores).  Repair round r reads the ends round r - 1 left in end[(r - 1) & 1] and writes every chunk's
// end to end[r & 1] (walked again, or copied), so no wave reads a word another wave of the same launch writes; start_used[c] is read and
// written by the wave of chunk c alone.  Everything that crosses lanes goes through the primitives of WaveDev and stays wave-uniform;
// the header's counters are bumped by lane 0 with an ordinary atomic.
// LDS and grid: those of nfa_set_wave_kernel (nfa_set_wave.h) -- four waves a block, a chunk (a queued string) per wave, persistent,
// capped by lds_blocks_per_cu.  A block that finds no chunk leaves before it touches LDS.  The workspace is never quiet.
#include <hip/hip_runtime.h>

#include "nfa_set_split_core.h"      // kSetSplitLookback, kSetSplitRounds: shared with the lane images
#include "nfa_set_wave.h"
#include "nfa_set_wave_split_core.h"

namespace mfa {

// Round 0, one wave per chunk: chunk 0 of a string from its true set ({start}, or its record of `states`), every other from a guess.
template <bool REV, bool IN_LDS>
__global__ void __launch_bounds__(256)
nfa_set_wave_chunk_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t depth, const uint8_t* __restrict__ bytes,
                          const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue, uint32_t* __restrict__ start_used,
                          uint32_t* __restrict__ end0, const uint32_t* __restrict__ states, const uint32_t* __restrict__ home, uint32_t lookback) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if ((uint64_t)blockIdx.x * 4u >= n_chunks) return;             // (no long string: every block leaves here, before it touches LDS)
    extern __shared__ uint32_t lds[];
    const uint32_t wave = WaveDev::uni(threadIdx.x >> 6);
    uint32_t* stack = lds + wave * depth;
    const NfaSetView t = nfa_set_view(tables, wave_tables_base<IN_LDS>(lds, tables, table_words, depth));
    const uint32_t W = tables[SET_H_WORDS], n_nodes = tables[SET_H_NODES], chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + wave; c < n_chunks; c += n_waves) {
        const SpecChunk ch = spec_chunk<REV>(queue, n_q, offsets, chunk, (uint32_t)c);
        const uint32_t* first = ch.k == 0u && states != nullptr ? states + queue[ch.q].sid * kWaveStateWords : nullptr;
        wave_spec_round0<REV, WaveDev>(t, n_nodes, W, stack, bytes, ch.b, ch.e, ch.lo, ch.hi, ch.k, first, home, lookback, start_used, end0, c);
    }
}

// One repair round, one wave per chunk: walked again from what its predecessor ended in, if that is not what it was walked from.
template <bool REV, bool IN_LDS>
__global__ void __launch_bounds__(256)
nfa_set_wave_repair_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t depth, const uint8_t* __restrict__ bytes,
                           const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue, uint32_t* __restrict__ start_used,
                           const uint32_t* __restrict__ end_prev, uint32_t* __restrict__ end_next) {
    const uint32_t n_chunks = hdr[SPLIT_H_CHUNKS];
    if ((uint64_t)blockIdx.x * 4u >= n_chunks) return;
    extern __shared__ uint32_t lds[];
    const uint32_t wave = WaveDev::uni(threadIdx.x >> 6);
    uint32_t* stack = lds + wave * depth;
    const NfaSetView t = nfa_set_view(tables, wave_tables_base<IN_LDS>(lds, tables, table_words, depth));
    const uint32_t W = tables[SET_H_WORDS], chunk = hdr[SPLIT_H_CHUNK], n_q = hdr[SPLIT_H_STRINGS];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + wave; c < n_chunks; c += n_waves) {
        const SpecChunk ch = spec_chunk<REV>(queue, n_q, offsets, chunk, (uint32_t)c);
        const bool walked = wave_spec_repair<REV, WaveDev>(t, W, stack, bytes, ch.lo, ch.hi, ch.k, start_used, end_prev, end_next, c);
        if (walked && WaveDev::lane() == 0u) atomicAdd(&hdr[SPEC_H_REWALKED], 1u);
    }
}

// One wave per queued string: the set it reaches from its true set over its records, walking the rest serially where they do not join up.
// RESUME (mfa_match_batch_resume_set_wide): from the string's record (live and not empty: the main kernel queues no other), which gets
// the set reached; results may then be NULL.
template <bool REV, bool IN_LDS, bool RESUME>
__global__ void __launch_bounds__(256)
nfa_set_wave_resolve_kernel(const uint32_t* __restrict__ tables, uint32_t table_words, uint32_t depth, const uint8_t* __restrict__ bytes,
                            const uint64_t* __restrict__ offsets, uint32_t* __restrict__ hdr, const SplitEntry* __restrict__ queue,
                            const uint32_t* __restrict__ start_used, const uint32_t* __restrict__ end_fin, uint32_t* states, uint8_t* __restrict__ results) {
    const uint32_t n_q = hdr[SPLIT_H_STRINGS];
    if ((uint64_t)blockIdx.x * 4u >= n_q) return;
    extern __shared__ uint32_t lds[];
    const uint32_t wave = WaveDev::uni(threadIdx.x >> 6);
    uint32_t* stack = lds + wave * depth;
    const NfaSetView t = nfa_set_view(tables, wave_tables_base<IN_LDS>(lds, tables, table_words, depth));
    const uint32_t W = tables[SET_H_WORDS], n_nodes = tables[SET_H_NODES], chunk = hdr[SPLIT_H_CHUNK];
    for (uint32_t q = blockIdx.x * 4u + wave; q < n_q; q += gridDim.x * 4u) {
        const uint64_t sid = queue[q].sid, b = offsets[sid], e = offsets[sid + 1u];
        const uint32_t first_chunk = queue[q].first, nc = queue[q].nc;
        uint32_t* rec = RESUME ? states + sid * kWaveStateWords : nullptr;
        uint64_t serial;
        const WaveRec<WaveDev> fin = wave_spec_resolve_string<REV, WaveDev>(t, n_nodes, W, stack, bytes, b, e, chunk, nc, start_used + (uint64_t)first_chunk * kWaveStateWords,
                                                                            end_fin + (uint64_t)first_chunk * kWaveStateWords, rec, &serial);
        if (serial != 0u && WaveDev::lane() == 0u) {
            atomicAdd(&hdr[SPEC_H_SERIAL_STRINGS], 1u);
            atomicAdd(reinterpret_cast<unsigned long long*>(&hdr[SPEC_H_SERIAL_BYTES]), (unsigned long long)serial);
        }
        if (RESUME) nfa_wave_state_encode<WaveDev>(fin.tag, fin.nodes, rec);
        if (!RESUME || results != nullptr) {
            const uint8_t r = wave_rec_result<WaveDev>(t, W, fin);
            if (WaveDev::lane() == 0u) results[sid] = r;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------
static_assert(kSplitSchemeWave.per_chunk == 3u * kWaveStateWords * sizeof(uint32_t) && kSplitSchemeWave.chunk_min == kWaveSplitChunkMin &&
              kSplitSchemeWave.arena_cap == kWaveSplitArenaChunks && kSplitSchemeWave.rounds == kSetSplitRounds && kSplitSchemeWave.lookback == kSetSplitLookback,
              "memless_plan.h: the wave scheme, three wide records per chunk");

template <bool REV, bool IN_LDS>
static int wave_split_tail_go(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets, uint8_t* d_results,
                              hipStream_t s, uint32_t* d_states) {
    const SetLds l = set_lds_of(img);
    const uint32_t* tables = (const uint32_t*)ds.d_set_tables;
    const uint32_t depth = img.set_tables[SET_H_DEPTH];
    const SplitEntry* queue = sl.args.queue;
    // one wave per chunk, the chunk count is the plan's: a grid for every chunk the arena holds, capped by what the CUs keep resident;
    // blocks beyond the count leave at once
    const uint64_t per_cu = lds_blocks_per_cu(l.bytes);
    const unsigned blocks = persistent_grid(sl.map_cap, 4, (uint64_t)ds.n_cus, per_cu), q_blocks = persistent_grid(sl.args.qcap, 4, (uint64_t)ds.n_cus, per_cu);
    return guess_tail<uint32_t>(sl, kWaveStateWords, d_offsets, s,
        [&](uint32_t* start_used, uint32_t* end0) {
            int rc = set_allow_lds<nfa_set_wave_chunk_kernel<REV, IN_LDS>>(ds.device);
            if (rc == MFA_OK) rc = set_allow_lds<nfa_set_wave_repair_kernel<REV, IN_LDS>>(ds.device);
            if (rc != MFA_OK) return rc;
            hipLaunchKernelGGL((nfa_set_wave_chunk_kernel<REV, IN_LDS>), dim3(blocks), dim3(256), l.bytes, s, tables, l.words, depth, d_bytes, d_offsets,
                               (const uint32_t*)sl.args.hdr, queue, start_used, end0, (const uint32_t*)d_states, (const uint32_t*)ds.d_set_home, sl.spec_lookback);
            return MFA_OK;
        },
        [&](uint32_t* start_used, const uint32_t* end_prev, uint32_t* end_next) {
            hipLaunchKernelGGL((nfa_set_wave_repair_kernel<REV, IN_LDS>), dim3(blocks), dim3(256), l.bytes, s, tables, l.words, depth, d_bytes, d_offsets,
                               sl.args.hdr, queue, start_used, end_prev, end_next);
            return MFA_OK;
        },
        [&](const uint32_t* start_used, const uint32_t* end_fin) {
            const int rc = d_states != nullptr ? set_allow_lds<nfa_set_wave_resolve_kernel<REV, IN_LDS, true>>(ds.device)
                                               : set_allow_lds<nfa_set_wave_resolve_kernel<REV, IN_LDS, false>>(ds.device);
            if (rc != MFA_OK) return rc;
            hipLaunchKernelGGL((d_states != nullptr ? nfa_set_wave_resolve_kernel<REV, IN_LDS, true> : nfa_set_wave_resolve_kernel<REV, IN_LDS, false>), dim3(q_blocks),
                               dim3(256), l.bytes, s, tables, l.words, depth, d_bytes, d_offsets, sl.args.hdr, queue, start_used, end_fin, d_states, d_results);
            return MFA_OK;
        });
}

int set_wave_split_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets, uint8_t* d_results,
                        void* stream, uint32_t* d_states) {
    if (sl.args.hdr == nullptr) return MFA_OK;
    if (!wave_tables_ok(img, ds) || ds.d_set_home == nullptr) return MFA_ERR_UNSUPPORTED;
    return MFA_WAVE_DISPATCH(wave_split_tail_go, set_lds_of(img).in_lds != 0u, img, ds, sl, d_bytes, d_offsets, d_results, (hipStream_t)stream, d_states);
}

}  // namespace mfa
