// Host side of the live-list walk: launch planning, and the mixed-batch object of the C-ABI (mfa_mixed_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "dfa_mixed.h"
#include "mfa_internal.h"
#include "walk.h"

namespace mfa {

// One launch over the sub-batch [d_offsets[0], d_offsets[n]): what is launched is plan_walk's decision (walk_plan.h); here are the
// environment, the lean hint's pinned word, the spill buffer and the stream.
int launch_walk(const WalkPlanInput& p, const uint32_t* d_tables, int n_cus, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                uint8_t* d_results, const uint64_t* d_regions, uint32_t n_seg, const uint32_t* seg_first, const uint32_t* seg_table,
                uint32_t** d_spill, size_t* spill_bytes, unsigned long long* d_counter, void* stream, LeanHint* lean, void* wait_event) {
    if (n == 0) { if (wait_event) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)wait_event, 0)); return MFA_OK; }
    const WalkKnobs kn = walk_knobs();
    Lean decision = d_regions != nullptr && kn.accel && kn.lean != 0 ? Lean::on : Lean::off;
    LeanHint next;
    const bool hinted = decision == Lean::on && lean != nullptr;
    if (hinted && lean->h_seen == nullptr) {
        if (hipHostMalloc((void**)&lean->h_seen, sizeof(uint32_t), hipHostMallocMapped) == hipSuccess) *lean->h_seen = 0u; else (void)hipGetLastError();
    }
    const uint32_t seen = hinted && lean->h_seen ? *(volatile uint32_t*)lean->h_seen : 0u;
    if (hinted && lean->h_seen) { next = *lean; decision = lean_decide(seen, next, kn); }
    WalkLaunch L;
    int rc = plan_walk(p, kn, n, n_cus, n_seg, decision, L);
    if (rc != MFA_OK) return rc;
    WalkArgs& a = L.args;
    if (hinted && lean->h_seen) {                              // (a launch that cannot be planned leaves the hint as it was)
        if (getenv("MFA_VERBOSE")) fprintf(stderr, "mfa_hip: table walk of %llu strings: last lean queue seen %d, launch %u: lean kernel %s\n",
                                           (unsigned long long)n, (int)seen - 1, lean->launches, decision == Lean::off ? "left out" : decision == Lean::probe ? "on (a look)" : "on");
        *lean = next;
        a.lean_seen = lean->h_seen;
    }
    rc = ctx_reserve((void**)d_spill, spill_bytes, L.spill_bytes);
    if (rc != MFA_OK) return rc;
    a.bytes = d_bytes; a.offsets = d_offsets; a.results = d_results; a.regions = d_regions; a.tables = d_tables; a.counter = d_counter;
    for (uint32_t k = 0; k <= n_seg; k++) a.seg_first[k] = seg_first[k];
    for (uint32_t k = 0; k < n_seg; k++) a.seg_table[k] = seg_table[k];
    a.spill = *d_spill;
    a.lean_queue = L.lean_grid ? reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(*d_spill) + L.queue_at) : nullptr;
    HIP_TRY(hipMemsetAsync(d_counter, 0, sizeof(unsigned long long) * L.counter_words, (hipStream_t)stream));
    // (what the launch waits for -- its group's regions -- comes AFTER its own preparations on the stream: they are done when the event arrives)
    if (wait_event) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)wait_event, 0));
    typedef int (*Launcher)(const WalkLaunch&, void*);
    static const Launcher by_cells[WALK_MAX_K + 1] = {nullptr, launch_walk_k1, launch_walk_k2, launch_walk_k3, launch_walk_k4, launch_walk_k5,
                                                     launch_walk_k6, launch_walk_k7, launch_walk_k8, launch_walk_k9};
    if (!walk_has_kernel(L)) return MFA_ERR_UNSUPPORTED;
    rc = (L.kernel == WalkKernel::stats ? launch_walk_stats : L.kernel == WalkKernel::long_k1 ? launch_walk_long_k1 : by_cells[L.K])(L, stream);
    if (L.kernel == WalkKernel::stats && rc == MFA_OK) { (void)hipStreamSynchronize((hipStream_t)stream); walk_print_stats(d_counter, "walk"); }
    return rc;
}

void lean_hint_free(LeanHint& h) {
    if (h.h_seen) (void)hipHostFree(h.h_seen);
    h.h_seen = nullptr;
}

void walk_print_stats(unsigned long long* d_counter, const char* tag) {
    unsigned long long h[32] = {0};
    if (hipMemcpy(h, d_counter, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;
    const unsigned long long* o = h + 8;
    const double tot = (double)o[16] > 0 ? (double)o[16] : 1.0;
    fprintf(stderr, "%s stats: %llu waves, %llu strings, wave-iterations %llu (dual %llu), lane steps %llu, skipped %llu, probes %llu (hits %llu), spill steps %llu\n", tag,
            o[17], o[5], o[8], o[9], o[3], o[0], o[1], o[2], o[4]);
    fprintf(stderr, "%s stats: cycles per wave-iteration %.0f; share: string start %.1f%%, byte %.1f%%, region look-up %.1f%%, plain step %.1f%%, dual step %.1f%%, book-keeping %.1f%%\n", tag,
            tot / (double)(o[8] ? o[8] : 1), 100.0 * o[10] / tot, 100.0 * o[11] / tot, 100.0 * o[12] / tot, 100.0 * o[13] / tot, 100.0 * o[14] / tot, 100.0 * o[15] / tot);
}

}  // namespace mfa

using namespace mfa;

// ---- mixed batches ---------------------------------------------------------------------------------------------------------------------
// One batch, several automata.  What a call launches, on which stream and behind which event, is decided by walk_plan.h's plan_mixed (the
// schedule is described there; it runs on a machine without a GPU: tests/emul/plan_emul.cpp).  The table engine walks the memory automata
// unless MFA_WALK=jit asks for the generated kernels, one launch per segment, or the table format cannot hold the object's automata.
// Here are the object, its state on a device, and match_mixed_impl, which enqueues a plan.
constexpr uint32_t MIX_TIMINGS = 32;      // (MIX_MAX_GROUPS, MIX_MAX_STREAMS, MIX_MAX_LAUNCHES: walk_plan.h)

struct mfa_mixed {
    std::vector<mfa_image*> images;
    std::vector<MixImage>   img;            // what plan_mixed needs of each image
    std::vector<uint32_t>   words;          // the images' table blocks, back to back (table engine)
    uint32_t K = 1;                         // most cells of a memory automaton
    bool reversed = false, table_ok = true;
    std::vector<uint8_t>    dfa_tables;     // the memory-less automata's tables as the multi-table launch reads them
    uint32_t n_mem = 0, n_dfa = 0;
    std::mutex mu;
    std::map<uint64_t, uint64_t> bytes_of;                     // string count of a batch -> its bytes (read back once, see mfa_match_mixed)
    struct Dev {
        uint32_t* d_tables = nullptr;
        hipStream_t last_cs = nullptr;                         // the caller's stream of the last call
        hipStream_t ws[MIX_MAX_STREAMS] = {nullptr};           // walk streams
        hipEvent_t ev_g[MIX_MAX_GROUPS] = {nullptr};           // group g's regions are known (timed)
        hipEvent_t ev_w[MIX_MAX_STREAMS] = {nullptr};          // end of a walk stream's work
        hipEvent_t ev_in = nullptr;
        uint8_t* d_dfa = nullptr;                              // dfa_tables on this device (uploaded when a call first has items)
        MixPlan last;                                          // the plan of the last call: its counts are what mfa_mixed_last_* report
        bool no_regions[MIX_TIMINGS] = {false};                // a call of the ring that had nothing to scan
        // timing of the last MIX_TIMINGS calls (a ring): first region launch, end of the last region launch, end of the call
        hipEvent_t ev_r0[MIX_TIMINGS] = {nullptr}, ev_r1[MIX_TIMINGS] = {nullptr}, ev_end[MIX_TIMINGS] = {nullptr};
        uint64_t calls = 0;
        uint64_t* d_regions = nullptr; size_t region_bytes = 0;
        uint32_t* d_spill[MIX_MAX_LAUNCHES] = {nullptr}; size_t spill_bytes[MIX_MAX_LAUNCHES] = {0};
        LeanHint lean[MIX_MAX_LAUNCHES];
        unsigned long long* d_counters = nullptr;
        int n_cus = 0;
        bool timed = false, calibrated = false;
        std::vector<float> cost;                               // per segment: its walk alone, ms
        float ready[MIX_MAX_GROUPS] = {0};                     // per group: end of its region launch, ms from the start of the call
        uint32_t ng_last = 0;
    };
    std::map<int, Dev> dev;
};

extern "C" {

int mfa_mixed_create(mfa_image_t* const* images, uint32_t n_images, mfa_mixed_t** out) {
    if (!images || !out || n_images == 0) return MFA_ERR_INVALID_ARG;
    *out = nullptr;
    mfa_mixed* mx = new (std::nothrow) mfa_mixed();
    if (!mx) return MFA_ERR_NOMEM;
    for (uint32_t k = 0; k < n_images; k++) {
        mfa_image* img = images[k];
        if (!img) { delete mx; return MFA_ERR_INVALID_ARG; }
        mx->images.push_back(img);
        const bool dfa = img->host.h.kind != MFA_KIND_MFA;                                      // (tabulated: no regions, no live lists; any direction)
        mx->img.push_back(MixImage{img->walk.K, img->walk.max_live, 0u, dfa, dfa && dfa_mixed_eligible(img->host), img->host.h.is_reversed != 0,
                                   dfa ? dfa_mixed_table_bytes(img->host) : 0u});
        if (dfa) { mx->n_dfa++; continue; }
        if (!img->walk_ok) mx->table_ok = false;
        if (mx->n_mem++ == 0) mx->reversed = img->walk.reversed;
        else if (mx->reversed != img->walk.reversed) mx->table_ok = false;                      // one scan direction per table launch
        mx->K = std::max(mx->K, img->walk.K);
    }
    for (uint32_t k = 0; k < n_images && mx->table_ok; k++) {
        mfa_image* img = mx->images[k];
        mx->img[k].block_at = (uint32_t)mx->words.size();
        if (mx->img[k].memoryless) continue;                  // (no block)
        if (mx->K > 6 && img->walk.K <= 6) {                  // a kernel for more than 6 cells reads 3-word edges
            WalkTables wide;
            if (build_walk_tables(img->host, wide, true) != MFA_OK) { mx->table_ok = false; break; }
            mx->words.insert(mx->words.end(), wide.words.begin(), wide.words.end());
        } else mx->words.insert(mx->words.end(), img->walk.words.begin(), img->walk.words.end());
    }
    if (mx->n_dfa) {
        std::vector<const HostImage*> hosts;
        std::vector<uint8_t> eligible;
        for (uint32_t k = 0; k < n_images; k++) { hosts.push_back(&mx->images[k]->host); eligible.push_back(mx->img[k].eligible ? 1 : 0); }
        mx->dfa_tables = dfa_mixed_pack(hosts, eligible);
    }
    *out = mx;
    return MFA_OK;
}

// Everything a Dev owns goes through here, whether the object is destroyed or its first call on a device fails half way (the device is
// the current one).  As device_release for an image's state.
static void mixed_dev_release(mfa_mixed::Dev& d) {
    for (hipStream_t w : d.ws) if (w) (void)hipStreamSynchronize(w);
    if (d.calls > 0) (void)hipEventSynchronize(d.ev_end[(d.calls - 1) % MIX_TIMINGS]);      // (region launches on a caller's stream)
    for (void* p : {(void*)d.d_tables, (void*)d.d_dfa, (void*)d.d_regions, (void*)d.d_counters}) if (p) (void)hipFree(p);
    for (uint32_t* p : d.d_spill) if (p) (void)hipFree(p);
    for (LeanHint& h : d.lean) lean_hint_free(h);
    for (hipEvent_t e : d.ev_g) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d.ev_w) if (e) (void)hipEventDestroy(e);
    if (d.ev_in) (void)hipEventDestroy(d.ev_in);
    for (uint32_t k = 0; k < MIX_TIMINGS; k++) for (hipEvent_t e : {d.ev_r0[k], d.ev_r1[k], d.ev_end[k]}) if (e) (void)hipEventDestroy(e);
    for (hipStream_t w : d.ws) if (w) (void)hipStreamDestroy(w);
    d = mfa_mixed::Dev{};
}

static int mixed_dev_init(const mfa_mixed* mx, int device, mfa_mixed::Dev& d) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    d.n_cus = prop.multiProcessorCount;
    if (mx->table_ok && mx->n_mem) {
        HIP_TRY(hipMalloc((void**)&d.d_tables, mx->words.size() * 4));
        HIP_TRY(hipMemcpy(d.d_tables, mx->words.data(), mx->words.size() * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMalloc((void**)&d.d_counters, 64 * MIX_MAX_LAUNCHES * sizeof(unsigned long long)));
    // Streams are made when a call first needs them (the walk streams: match_mixed_impl): every stream beyond the hardware queues of the process (four
    // by default, the caller's included) shares a queue with another one, and work on streams that share a queue is serialised
    for (hipEvent_t& e : d.ev_g) HIP_TRY(hipEventCreate(&e));
    for (hipEvent_t& e : d.ev_w) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.ev_in, hipEventDisableTiming));
    for (uint32_t k = 0; k < MIX_TIMINGS; k++) { HIP_TRY(hipEventCreate(&d.ev_r0[k])); HIP_TRY(hipEventCreate(&d.ev_r1[k])); HIP_TRY(hipEventCreate(&d.ev_end[k])); }
    d.cost.assign(mx->images.size(), 0.0f);
    return MFA_OK;
}

// the object's state on `device`, built in place in the map by its first call there: a call that fails half way leaves no entry behind
static int mixed_device(mfa_mixed* mx, int device, mfa_mixed::Dev** out) {
    int rc = check_device(device);
    if (rc != MFA_OK) return rc;
    const auto ins = mx->dev.try_emplace(device);
    *out = &ins.first->second;
    if (!ins.second || (rc = mixed_dev_init(mx, device, **out)) == MFA_OK) return MFA_OK;
    mixed_dev_release(**out);
    mx->dev.erase(ins.first);
    return rc;
}

void mfa_mixed_destroy(mfa_mixed_t* mx) {
    if (!mx) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (auto& kv : mx->dev) { (void)hipSetDevice(kv.first); mixed_dev_release(kv.second); }
    if (cur >= 0) (void)hipSetDevice(cur);
    delete mx;
}

// The batch's bytes are device data (offsets[n] - offsets[0]): a caller that knows them says so (mfa_match_mixed_sized); otherwise they are
// read back ONCE per string count this object meets -- that call waits for the caller's stream -- and remembered (a later batch with the
// same count and other bytes gets the same grouping: a matter of speed only).
static int mixed_bytes(mfa_mixed* mx, const uint64_t* d_offsets, uint64_t n, hipStream_t cs, uint64_t* bytes) {
    auto known = mx->bytes_of.find(n);
    if (known != mx->bytes_of.end()) { *bytes = known->second; return MFA_OK; }
    if (n < 65536) return MFA_OK;      // (one group whatever its bytes: plan_cuts)
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], d_offsets, sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipMemcpyAsync(&ends[1], d_offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    *bytes = ends[1] - ends[0];
    if (mx->bytes_of.size() >= 64) mx->bytes_of.clear();
    mx->bytes_of[n] = *bytes;
    return MFA_OK;
}

// Once per device, after the first call on the per-segment engine: the walks' costs and the groups' region times.  That call runs a group's
// walks before the next group's region launch is reached by nothing: region launches follow each other on the caller's stream, so the
// elapsed time between two group events is the later group's region time.
static int mixed_calibrate(mfa_mixed* mx, mfa_mixed::Dev* d, const uint64_t* seg_first, int device, uint32_t slot_t) {
    HIP_TRY(hipEventSynchronize(d->ev_end[slot_t]));
    for (uint32_t s = 0; s < (uint32_t)mx->images.size(); s++) {
        float ms = 0.0f;
        if (seg_first[s + 1] > seg_first[s] && !mx->img[s].memoryless && mfa_last_kernel_ms(mx->images[s], device, &ms) == MFA_OK) d->cost[s] = ms;
    }
    for (uint32_t g = 0; g < d->ng_last; g++) HIP_TRY(hipEventElapsedTime(&d->ready[g], d->ev_r0[slot_t], d->ev_g[g]));
    d->calibrated = true;
    return MFA_OK;
}

// Once work has gone to the internal streams, the caller's stream is made to wait for all of it before match_mixed_impl returns, whatever
// happens: a caller that gets an error may free or reuse its buffers in stream order like one that gets MFA_OK.
struct MixJoin {
    mfa_mixed::Dev* d; hipStream_t cs; int NS; uint32_t slot_t; bool used[MIX_MAX_STREAMS] = {false}; bool started = false; int err = MFA_OK;
    void run() {
        if (!started) return;
        started = false;
        for (int k = 0; k < NS; k++)
            if (used[k] && (hipEventRecord(d->ev_w[k], d->ws[k]) != hipSuccess || hipStreamWaitEvent(cs, d->ev_w[k], 0) != hipSuccess)) { err = MFA_ERR_HIP; (void)hipStreamSynchronize(d->ws[k]); }
        if (hipEventRecord(d->ev_end[slot_t], cs) != hipSuccess) { err = MFA_ERR_HIP; (void)hipStreamSynchronize(cs); }
    }
    ~MixJoin() { run(); }
};

// seg_first: HOST array of n_images + 1 string indices, seg_first[0] = 0, seg_first[n_images] = n: strings seg_first[s] ..
// seg_first[s+1]-1 are matched against images[s] (the order of mfa_mixed_create).  `stream` sees the call as one operation.
// total_bytes: offsets[n] - offsets[0] if the caller knows it, else 0 (then it is read back once per string count: see the header).
static int match_mixed_impl(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* seg_first,
                            uint8_t* d_results, int device, void* stream, uint64_t total_bytes) {
    if (!mx || !d_offsets || !seg_first || (!d_results && n)) return MFA_ERR_INVALID_ARG;
    const uint32_t ns = (uint32_t)mx->images.size();
    if (seg_first[0] != 0 || seg_first[ns] != n) return MFA_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < ns; s++)
        if (seg_first[s] > seg_first[s + 1]) return MFA_ERR_INVALID_ARG;
    if (n == 0) return MFA_OK;
    std::lock_guard<std::mutex> lk(mx->mu);
    mfa_mixed::Dev* d = nullptr;
    int rc = mixed_device(mx, device, &d);
    if (rc != MFA_OK) return rc;
    hipStream_t cs = (hipStream_t)stream;
    const MixKnobs kn = mixed_knobs();
    if (mx->n_mem && !kn.cuts && total_bytes == 0 && (rc = mixed_bytes(mx, d_offsets, n, cs, &total_bytes)) != MFA_OK) return rc;
    // ---- what the call will launch, decided before anything is put on a stream (an error found here leaves the streams untouched)
    MixPlan plan = plan_mixed(mx->img, MixObject{mx->K, (uint32_t)mx->words.size(), mx->n_mem, mx->n_dfa, mx->table_ok}, seg_first, n, total_bytes, kn,
                              MixCalib{d->calibrated, d->ng_last, d->ready, d->cost.data()});
    if (plan.rc != MFA_OK) return plan.rc;
    if (!plan.dfa.items.empty() && !d->d_dfa) {
        HIP_TRY(hipMalloc((void**)&d->d_dfa, mx->dfa_tables.size()));
        HIP_TRY(hipMemcpy(d->d_dfa, mx->dfa_tables.data(), mx->dfa_tables.size(), hipMemcpyHostToDevice));
    }
    if (plan.with_regions && (rc = ctx_reserve((void**)&d->d_regions, &d->region_bytes, (size_t)n * MFA_REGION_WORDS * sizeof(uint64_t))) != MFA_OK) return rc;
    uint64_t* d_table = plan.with_regions ? d->d_regions : nullptr;
    for (int k = 0; k < plan.NS; k++)
        if (!d->ws[k]) HIP_TRY(hipStreamCreateWithFlags(&d->ws[k], hipStreamNonBlocking));
    const uint32_t slot_t = (uint32_t)(d->calls % MIX_TIMINGS);
    // ---- from here on work goes to the internal streams (plan.direct: none, NS is 0, and the only launch is mfa_match_batch's below).
    // The object's buffers -- table, counters, spill areas -- are shared by its calls: a call starts behind the end of the one before it,
    // whichever stream that one came on (the walk streams start behind ev_in)
    MixJoin join{d, cs, plan.NS, slot_t};
    if (d->calls > 0 && d->last_cs != cs) HIP_TRY(hipStreamWaitEvent(cs, d->ev_end[(d->calls - 1) % MIX_TIMINGS], 0));
    d->last_cs = cs;
    if (plan.NS) HIP_TRY(hipEventRecord(d->ev_in, cs));
    join.started = true;
    for (int k = 0; k < plan.NS; k++) HIP_TRY(hipStreamWaitEvent(d->ws[k], d->ev_in, 0));
    // the memory-less segments wait for nothing else: they run beside the region launches
    if (plan.KD >= 0) join.used[plan.KD] = true;
    for (const auto& items : plan.dfa_multi) {
        rc = launch_dfa_mixed(plan.dfa, items.first, items.second, d->d_dfa, d->n_cus, d_bytes, d_offsets, n, d_results, d->ws[plan.KD]);
        if (rc != MFA_OK) return rc;
    }
    for (uint32_t s : plan.dfa.own) {
        rc = mfa_match_batch(mx->images[s], d_bytes, d_offsets + seg_first[s], seg_first[s + 1] - seg_first[s], d_results + seg_first[s], device, d->ws[plan.KD]);
        if (rc != MFA_OK) return rc;
    }
    // The region launches go to the CALLER's stream: back-to-back calls pass from the last walk of one to the first region launch of the next
    // through ONE event (walk stream -> caller's stream) instead of three through a region stream of the object's own: 0.02 ms a call.
    HIP_TRY(hipEventRecord(d->ev_r0[slot_t], cs));
    if (plan.direct && (rc = mfa_match_batch(mx->images[0], d_bytes, d_offsets, n, d_results, device, stream)) != MFA_OK) return rc;
    size_t r = 0, w = 0;
    for (uint32_t g = 0; g < plan.n_groups; g++) {
        for (; r < plan.regions.size() && plan.regions[r].g == g; r++) {
            const MixRegion& R = plan.regions[r];
            rc = launch_region_scan(d->n_cus, d_bytes, d_offsets + R.a, R.b - R.a, d_table + R.a * MFA_REGION_WORDS, cs, R.threads, R.signals ? d->ev_g[g] : nullptr);
            if (rc != MFA_OK) return rc;
        }
        if (plan.own_event[g]) HIP_TRY(hipEventRecord(d->ev_g[g], cs));
        for (; w < plan.walks.size() && plan.walks[w].g == g; w++) {
            const MixLaunch& L = plan.walks[w];
            const uint64_t* regions = d_table ? d_table + L.a * MFA_REGION_WORDS : nullptr;
            join.used[L.k] = true;
            if (plan.table) {                                  // (the launch itself waits, behind its own preparations on the stream)
                const WalkPlanInput pk{L.Kc, L.ml, mx->reversed, L.w1 - L.w0};
                rc = launch_walk(pk, d->d_tables + L.w0, d->n_cus, d_bytes, d_offsets + L.a, L.b - L.a, d_results + L.a, regions, L.s1 - L.s0, L.sf, L.stb, &d->d_spill[L.slot],
                                 &d->spill_bytes[L.slot], d->d_counters + 64 * L.slot, d->ws[L.k], &d->lean[L.slot], L.waits ? d->ev_g[g] : nullptr);
            } else {
                if (L.waits) HIP_TRY(hipStreamWaitEvent(d->ws[L.k], d->ev_g[g], 0));
                rc = mfa_match_batch_regions(mx->images[L.s0], d_bytes, d_offsets + L.a, L.b - L.a, d_results + L.a, regions, device, d->ws[L.k]);
            }
            if (rc != MFA_OK) return rc;
        }
    }
    HIP_TRY(hipEventRecord(d->ev_r1[slot_t], cs));
    // the caller's stream (and with it the call's end event) waits for every stream that was given work
    join.run();
    if (join.err != MFA_OK) return join.err;
    d->no_regions[slot_t] = plan.no_regions;
    d->timed = true; d->calls++; d->ng_last = plan.n_groups;
    d->last = std::move(plan);                                // (its counts are what the mfa_mixed_last_* calls report)
    return d->last.calibrating ? mixed_calibrate(mx, d, seg_first, device, slot_t) : MFA_OK;
}

int mfa_match_mixed(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* seg_first,
                    uint8_t* d_results, int device, void* stream) {
    return match_mixed_impl(mx, d_bytes, d_offsets, n, seg_first, d_results, device, stream, 0);
}

int mfa_match_mixed_sized(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint64_t total_bytes, const uint64_t* seg_first,
                          uint8_t* d_results, int device, void* stream) {
    return match_mixed_impl(mx, d_bytes, d_offsets, n, seg_first, d_results, device, stream, total_bytes);
}

// the plan of the last call on `device` that went well, or nullptr; the caller holds mx->mu
static const MixPlan* mixed_last(mfa_mixed_t* mx, int device) {
    auto it = mx->dev.find(device);
    return it == mx->dev.end() || !it->second.timed ? nullptr : &it->second.last;
}

// what the last call on `device` launched (any pointer may be NULL): region launches, walk launches, groups of strings, and `gated`, always 0
// (kept for compatibility)
int mfa_mixed_last_launches(mfa_mixed_t* mx, int device, uint32_t* region_launches, uint32_t* walk_launches, uint32_t* groups, uint32_t* gated) {
    if (!mx) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(mx->mu);
    const MixPlan* p = mixed_last(mx, device);
    if (!p) return MFA_ERR_INVALID_ARG;
    if (region_launches) *region_launches = p->n_regions;
    if (walk_launches) *walk_launches = p->n_walks;
    if (groups) *groups = p->n_groups;
    if (gated) *gated = 0u;
    return MFA_OK;
}

// what the last call on `device` did with its memory-less segments (any pointer may be NULL): multi-table launches, launches of single
// segments, and the items and strings of the multi-table launches
int mfa_mixed_last_dfa(mfa_mixed_t* mx, int device, uint32_t* multi_launches, uint32_t* own_launches, uint32_t* items, uint64_t* strings) {
    if (!mx) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(mx->mu);
    const MixPlan* p = mixed_last(mx, device);
    if (!p) return MFA_ERR_INVALID_ARG;
    if (multi_launches) *multi_launches = p->n_dfa_multi;
    if (own_launches) *own_launches = p->n_dfa_own;
    if (items) *items = p->n_dfa_items;
    if (strings) *strings = p->dfa_strings;
    return MFA_OK;
}

// The same with HOST pointers: copies the batch to the device, matches, copies the results back, synchronises (the host mirror's
// match_mixed and the `diploma -match-mixed` command line; throughput is then bounded by the host link).
int mfa_match_mixed_host(mfa_mixed_t* mx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, const uint64_t* seg_first, uint8_t* results, int device) {
    if (!mx || !seg_first) return MFA_ERR_INVALID_ARG;
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t total, void*) {
        return match_mixed_impl(mx, d_bytes, d_off, n, seg_first, d_res, device, nullptr, total); });
}

// Device time of a recent mfa_match_mixed on `device`: from its first region launch to the end of its last region launch, and to the
// end of its last walk (either pointer may be NULL).  back = 0: the last call, 1: the one before, ... (the library keeps the events
// of its last 32 calls, so a caller can time a sequence of calls without synchronising between them).  Synchronises on that call's end.
int mfa_mixed_timing(mfa_mixed_t* mx, int device, uint32_t back, float* region_ms, float* span_ms) {
    if (!mx) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(mx->mu);
    auto it = mx->dev.find(device);
    if (it == mx->dev.end() || !it->second.timed || back >= MIX_TIMINGS || back >= it->second.calls) return MFA_ERR_INVALID_ARG;
    mfa_mixed::Dev& d = it->second;
    const uint32_t k = (uint32_t)((d.calls - 1 - back) % MIX_TIMINGS);
    HIP_TRY(hipEventSynchronize(d.ev_end[k]));
    if (region_ms) { if (d.no_regions[k]) *region_ms = 0.0f; else HIP_TRY(hipEventElapsedTime(region_ms, d.ev_r0[k], d.ev_r1[k])); }
    if (span_ms) HIP_TRY(hipEventElapsedTime(span_ms, d.ev_r0[k], d.ev_end[k]));
    return MFA_OK;
}

int mfa_mixed_last_ms(mfa_mixed_t* mx, int device, float* region_ms, float* span_ms) { return mfa_mixed_timing(mx, device, 0u, region_ms, span_ms); }

}  // extern "C"
