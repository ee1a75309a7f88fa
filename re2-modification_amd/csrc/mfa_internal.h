// Internal declarations shared by the host-side image code, the kernels' launchers
// and the C-ABI glue of libmfa_hip.so.  Not installed.
#ifndef MFA_INTERNAL_H
#define MFA_INTERNAL_H

#include <hip/hip_runtime.h>
#include <cstdint>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mfa_hip.h"
#include "walk_tables.h"
#include "dfa_split.h"      // and memless_plan.h: MemlessKnobs, SplitScheme, plan_split, plan_memless_engine, persistent_grid
#include "walk_plan.h"      // LeanHint, WalkPlanInput, env_int, regions_enabled
#include "search_tables.h"  // SearchTables: the two tables of mfa_search_batch

#define HIP_TRY(expr)                                                   \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess) { set_last_hip_error((int)e_); return MFA_ERR_HIP; } \
    } while (0)

namespace mfa {

// ---- host image ---------------------------------------------------------------------------

struct HostImage {
    mfa_blob_header            h{};
    std::vector<uint32_t>      edge_begin;  // n_nodes + 1
    std::vector<mfa_blob_edge> edges;

    uint32_t              dfa_home = 1;        // MFA_KIND_NFA, tables in L2: second seed of dfa_spec.hip's guesses (dfa_spec_core.h: spec_home_state)
    // MFA_KIND_NFA only: the reference's step function (automata.cpp:98-128) tabulated
    // over its reachable state sets.  State 0 = the empty set (absorbing, rejects),
    // state 1 = {start}.
    uint32_t              dfa_states = 0;
    uint32_t              n_classes  = 0;
    uint8_t               byte_class[256] = {0};
    std::vector<uint32_t> dfa_trans;   // [dfa_states][n_classes]
    std::vector<uint8_t>  dfa_accept;  // [dfa_states]: finish is in the set after the final pass
    // MFA_KIND_NFA whose tabulation passed the limit: the tables of the set walk (nfa_set_core.h); dfa_states is then 0
    bool                  set_walk = false;
    std::vector<uint32_t> set_tables;
    bool                  set_wave = false;    //   ... in the form of the wave-cooperative walk (nfa_set_wave_core.h): one string per wave, up to 2048 nodes
    uint32_t              set_home[8] = {0};   //   ... and the second seed of nfa_set_split.hip's guesses, a node set (image_host.cpp: nfa_set_home)
    uint32_t              set_home_wide[64] = {0};   //   ... of a wave image: the second seed of nfa_set_wave_split.hip's guesses (nfa_set_home_wide), set_home stays zero
    mutable int           jit_source_ok = -1;      // MFA kind: the generated kernel's source is of a size a compiler finishes (jit.hip; -1 = not looked at)
};

int parse_blob(const void* blob, size_t n_bytes, HostImage& out);   // MFA_OK / MFA_ERR_*
int check_mfa_invariants(const HostImage& img);                      // MFA_OK / MFA_ERR_UNSUPPORTED
int tabulate_nfa(HostImage& img, uint32_t max_states = MFA_MAX_DFA_STATES, std::vector<std::string>* sets_out = nullptr);   // fills the dfa_* members; MFA_ERR_UNSUPPORTED beyond max_states state sets
int nfa_set_build(HostImage& img);                                   // fills set_tables instead (MFA_ERR_UNSUPPORTED: outside the set walk's limits)
int nfa_set_wave_build(HostImage& img);                              // ... in the wave form (sets set_wave beside set_walk; MFA_ERR_UNSUPPORTED beyond 2048 nodes)
void nfa_set_home(const HostImage& img, uint32_t (&home)[8]);        // a set-walk image's home set (nfa_set_build fills set_home with it)
void nfa_set_home_wide(const HostImage& img, uint32_t (&home)[64]);  // a wave image's home set, the same rule (nfa_set_wave_build fills set_home_wide with it)
int nfa_image_build(HostImage& img);                                 // MFA_KIND_NFA at image creation: one or the other

// ---- per-device state -----------------------------------------------------------------------

// Workspace of ONE launch: ticket counter, scratch, region table, events.  Every launch takes one from the
// pool of its (image, device); a context is reused by a later launch on the SAME stream (stream order makes
// that safe) or once its `done` event has completed, so launches of one image that overlap on different
// streams or from different host threads never share a counter, a scratch buffer or an event.
void lean_hint_free(LeanHint& h);

struct LaunchCtx {
    LeanHint lean;
    unsigned long long* d_counter = nullptr;   // next-string ticket (+ MFA_STATS words)
    uint32_t*           d_scratch = nullptr;   // slot arrays / probe images that do not fit LDS
    size_t              scratch_bytes = 0;
    uint64_t*           d_regions = nullptr;   // region table of the batch (regions.hip)
    size_t              region_bytes = 0;
    void*               ev_start = nullptr;    // hipEvent_t: around the match kernel
    void*               ev_stop  = nullptr;
    void*               ev_r0 = nullptr;       // around the region pass
    void*               ev_r1 = nullptr;
    void*               ev_done = nullptr;     // after the last kernel of the launch (no timing)
    void*               stream = nullptr;      // stream of the launch it was last used for
    bool                used = false;
    bool                ran_regions = false;
    // split path for long strings of memory-less automata (dfa_split.hip): plan header, queue and map arena of this launch
    uint8_t*            d_split = nullptr;
    size_t              split_bytes = 0;
    uint32_t*           split_seen = nullptr;  // pinned, device-visible; memless_plan.h: SplitWorkspace has the values
    uint32_t            split_quiet = 0;       // calls in a row that found "no long string" there
    bool                split_keep = false;    // a launch without the split kernels met a long string once: this workspace keeps them
    bool                split_ran = false;     // this launch has the split kernels behind its main kernel
    bool                spec_ran = false;      //   ... those of dfa_spec.hip (a table in L2): its header holds the words of mfa_last_dfa_spec
    bool                set_split_ran = false; // this launch has the kernels of nfa_set_split.hip behind its main kernel (mfa_last_set_split; the two above stay false)
};

struct DeviceState {
    int       device = -1;
    // NFA kind
    void*     d_dfa_trans  = nullptr;   // [dfa_states][n_classes], 16-bit entries up to 65535 state sets, 32-bit beyond
    uint8_t*  d_dfa_accept = nullptr;
    uint8_t*  d_byte_class = nullptr;
    uint32_t* d_set_tables = nullptr;   // a set-walk image: HostImage::set_tables
    uint32_t* d_set_home = nullptr;     // a wave image: HostImage::set_home_wide, 64 words of their own
    uint16_t* d_search[2] = {nullptr, nullptr};   // mfa_search_batch: the tables of pass 1 and pass 2 (mfa_image::search), uploaded by its first call
    // launch workspaces
    std::vector<LaunchCtx*> ctxs;
    LaunchCtx*              last = nullptr;    // context of the most recent launch (mfa_last_kernel_ms)
    int                 n_cus = 0;
    // specialised kernel (jit.hip), if one is loaded for this device
    bool                jit_tried = false;
    bool                jit_probed = false, jit_in_cache = false;      // automatic mode: looked whether the code object is cached
    void*               jit_mod = nullptr;     // hipModule_t
    void*               jit_fn  = nullptr;     // hipFunction_t
    int                 jit_waves_per_cu = 0;
    uint32_t            jit_words = 0;         // words per slot set of the specialised kernel
    uint32_t            jit_lanes = 64;        // string-carrying lanes per wave
    // live-list walk (walk.hip): the image's tables on this device
    uint32_t*           d_walk = nullptr;
};

}  // namespace mfa

struct mfa_image {
    mfa::HostImage                    host;
    std::mutex                        mu;
    std::map<int, mfa::DeviceState>   dev;
    uint32_t                          last_kernel = 0;   // MFA_KERNEL_*
    mfa::WalkTables                   walk;              // MFA kind: tables of the live-list walk (walk_tables.h)
    bool                              walk_ok = false;   //   ... built (false: the automaton exceeds the table format)
    mfa::SearchTables                 search;            // tabulated NFA kind: the tables of mfa_search_batch, built under `mu` by its first call (search_tables.h)
};

namespace mfa {

// launchers (kernels.hip); all asynchronous on `stream`
int launch_dfa_walk(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                    uint64_t n, uint8_t* d_results, void* stream);
// the same walk with every string's state read from and written to d_states (mfa_match_batch_resume); d_results may be NULL
int launch_dfa_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint32_t* d_states, uint8_t* d_results, void* stream);
// nfa_set.hip: the set walk of an image whose tabulation passed the limit (HostImage::set_walk)
int launch_nfa_set(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                   uint8_t* d_results, void* stream);
// the same walk with every string's set read from and written to its record of d_states (mfa_match_batch_resume_set: n records of twelve
// words, 16-byte aligned); d_results may be NULL
int launch_nfa_set_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                          uint32_t* d_states, uint8_t* d_results, void* stream);
// nfa_set_wave.hip: the same for an image with wave tables (HostImage::set_wave), one string per wave; a long string is cut by
// nfa_set_wave_split.hip behind the main kernel
int launch_nfa_set_wave(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                        uint8_t* d_results, void* stream);
// the same walk with every string's set read from and written to its record of d_states (mfa_match_batch_resume_set_wide: n records of
// 68 words, 16-byte aligned); d_results may be NULL
int launch_nfa_set_wave_resume(const HostImage& img, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                               uint32_t* d_states, uint8_t* d_results, void* stream);
// dfa_split.hip: split_begin in front of the main kernel (its `args` go to that kernel), the engine's tail behind it
struct SplitLaunch {
    SplitArgs args{};
    uint8_t*  maps = nullptr;
    uint32_t  chunk_min = 0, arena_chunks = 0, map_cap = 0;
    uint32_t  spec_rounds = 0, spec_lookback = 0;      // guess-repair-resolve tails: repair launches and lookback bytes of this call (`maps` holds its records)
};
// THE begin of every engine: makes and reads the pinned word, asks plan_split (memless_plan.h), reserves the workspace, zeroes the header
// and raises the scheme's flags of cx.  out->args.split_min == 0: the path is off; out->args.hdr == NULL: no tail follows this launch.
int  split_begin(const SplitScheme& sc, const MemlessKnobs& kn, LaunchCtx& cx, uint64_t n, void* stream, SplitLaunch* out);
int  split_plan(const SplitLaunch& sl, const uint64_t* d_offsets, void* stream);
// the tails: nothing when sl.args.hdr == NULL.  d_states != NULL (the resume calls): a queued string starts from its word or record of
// d_states, which gets what it reaches; d_results may then be NULL
int  split_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                uint8_t* d_results, void* stream, uint32_t* d_states = nullptr);
// dfa_spec.hip: tables in L2 (255 state sets and more).  spec_main launches the one main kernel of such tables -- d_states != NULL: its
// instantiation for mfa_match_batch_resume
bool spec_applies(const HostImage& img);
int  spec_main(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
               uint8_t* d_results, void* stream, uint32_t* d_states, unsigned blocks);
int  spec_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
               uint8_t* d_results, void* stream, uint32_t* d_states = nullptr);
// nfa_set_split.hip, nfa_set_wave_split.hip: a set-walk image, a lane or a wave per chunk
int  set_split_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                    uint8_t* d_results, void* stream, uint32_t* d_states);
int  set_wave_split_tail(const HostImage& img, DeviceState& ds, const SplitLaunch& sl, const uint8_t* d_bytes, const uint64_t* d_offsets,
                         uint8_t* d_results, void* stream, uint32_t* d_states);
// search.hip: mfa_search_batch.  search_upload puts the image's two tables on the device once (synchronous); launch_search brackets pass 1
// and, with d_spans, pass 2 in ev_start and ev_stop
int  search_upload(const SearchTables& tb, DeviceState& ds);
int  launch_search(const HostImage& img, const SearchTables& tb, DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                   uint64_t n, uint8_t* d_results, uint64_t* d_spans, uint8_t* d_span_results, void* stream);
// regions.hip
int launch_region_scan(int n_cus, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint64_t* d_table, void* stream, unsigned threads = 256, void* done_event = nullptr);
// launch contexts (capi.hip); the caller holds the image mutex
int  ctx_acquire(DeviceState& ds, void* stream, LaunchCtx** out);
int  ctx_reserve(void** buf, size_t* have, size_t need);
int device_prepare(mfa_image* img, int device, DeviceState** out);
// specialised kernels (jit_gen.cpp, jit.hip)
uint32_t    jit_slot_registers(const HostImage& img);
uint32_t    jit_lanes(const HostImage& img);
std::string jit_generate_source(const HostImage& img);
bool        jit_enabled(const HostImage& img);
bool        jit_cached(const HostImage& img);      // its code object is in the cache already
std::string jit_compile(const HostImage& img, std::string* err);
bool        jit_load(const HostImage& img, DeviceState& ds);
void        jit_unload(DeviceState& ds);
void        jit_print_stats(LaunchCtx& cx, const char* tag);
int         launch_mfa_jit(DeviceState& ds, LaunchCtx& cx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint8_t* d_results,
                           const uint64_t* d_regions, void* stream);
void device_release(DeviceState& ds);
// live-list walk (walk_launch.hip).  seg_first: n_seg + 1 string indices relative to the sub-batch; seg_table: word offsets into d_tables
int launch_walk(const WalkPlanInput& p, const uint32_t* d_tables, int n_cus, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                uint8_t* d_results, const uint64_t* d_regions, uint32_t n_seg, const uint32_t* seg_first, const uint32_t* seg_table,
                uint32_t** d_spill, size_t* spill_bytes, unsigned long long* d_counter, void* stream, LeanHint* lean = nullptr, void* wait_event = nullptr);
void set_last_hip_error(int e);
// capi.hip: `match` is given the device copies of the bytes, offsets, results, the batch's bytes, and the state records (nullptr without)
typedef std::function<int(const uint8_t* d_bytes, const uint64_t* d_offsets, uint8_t* d_results, uint64_t total_bytes, void* d_states)> HostMatch;
int  match_host_staged(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results, int device, const HostMatch& match,
                       void* states = nullptr, size_t state_bytes = 0, bool check_lengths = true);
int  check_device(int device);      // MFA_ERR_NO_DEVICE unless `device` exists; makes it the current one

// ---- one enqueue path of the memory-less engines -------------------------------------------------------------------------------------------
#ifdef __HIPCC__
// begin, ev_start, main kernel, tail, ev_stop: what every launch function of these engines does.  main(sl) launches the main kernel with
// sl.args, tail(sl) the kernels behind it; ev_stop is not recorded behind a tail that failed.
template <class Main, class Tail>
int memless_bracket(const SplitScheme& sc, const MemlessKnobs& kn, LaunchCtx& cx, uint64_t n, hipStream_t s, Main main, Tail tail) {
    SplitLaunch sl;
    int rc = split_begin(sc, kn, cx, n, s, &sl);
    if (rc != MFA_OK) return rc;
    HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_start, s));
    if ((rc = main(sl)) != MFA_OK) return rc;
    HIP_TRY(hipGetLastError());
    if ((rc = tail(sl)) != MFA_OK) return rc;
    HIP_TRY(hipEventRecord((hipEvent_t)cx.ev_stop, s));
    return MFA_OK;
}

// The guess-repair-resolve tail (dfa_spec.hip, nfa_set_split.hip, nfa_set_wave_split.hip) over an arena of records of `words` Rec each,
// start_used[map_cap], end[2][map_cap]: plan, round 0 into end[0], sl.spec_rounds repairs that read end[(r - 1) & 1] and write end[r & 1],
// resolve from the last one written.  The callables launch (and return MFA_OK or what kept them from it).
template <class Rec, class Round0, class Repair, class Resolve>
int guess_tail(const SplitLaunch& sl, size_t words, const uint64_t* d_offsets, hipStream_t s, Round0 round0, Repair repair, Resolve resolve) {
    int rc = split_plan(sl, d_offsets, s);
    if (rc != MFA_OK) return rc;
    Rec* start_used = reinterpret_cast<Rec*>(sl.maps);
    Rec* end[2] = {start_used + (size_t)sl.map_cap * words, start_used + 2u * (size_t)sl.map_cap * words};
    if ((rc = round0(start_used, end[0])) != MFA_OK) return rc;
    HIP_TRY(hipGetLastError());
    for (uint32_t r = 1; r <= sl.spec_rounds; r++) {
        if ((rc = repair(start_used, (const Rec*)end[(r - 1u) & 1u], end[r & 1u])) != MFA_OK) return rc;
        HIP_TRY(hipGetLastError());
    }
    if ((rc = resolve((const Rec*)start_used, (const Rec*)end[sl.spec_rounds & 1u])) != MFA_OK) return rc;
    HIP_TRY(hipGetLastError());
    return MFA_OK;
}
#endif

}  // namespace mfa

#endif
