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
// One batch, several automata.  The region pass runs over groups of consecutive segments on one internal stream; what walks a group
// starts as soon as the group's regions are known and runs beside the next group's region pass:
//   * table engine (MFA_WALK=table): ONE launch of the table-driven walk kernel per group, any lane any automaton;
//   * generated kernels (default while they are the faster walk on small automata): one launch per segment, spread over a few walk
//     streams by measured cost -- the first call on a device runs the walks one after the other and times them, later calls give
//     each walk to the stream that can start it first (list scheduling with the groups' region times as release times).
// Memory-less automata (MFA_KIND_NFA) need no regions: the region launches leave their strings out, and their segments are walked by the
// table kernels on an internal stream of their own, behind the call's entry event only -- the eligible ones in ONE launch of
// dfa_mixed_kernel (dfa_mixed.hip), the others in a launch each (walk_plan.h: plan_dfa_items).
constexpr uint32_t MIX_TIMINGS = 32;      // (MIX_MAX_GROUPS, MIX_MAX_STREAMS, MIX_MAX_LAUNCHES: walk_plan.h)

struct mfa_mixed {
    std::vector<mfa_image*> images;
    std::vector<uint32_t>   words;          // the images' table blocks, back to back (table engine)
    std::vector<uint32_t>   block_at;       // word offset of image k's block
    uint32_t K = 1, max_live = 1;
    bool reversed = false, table_ok = true;
    // memory-less automata: per image, 1 = memory-less; those among them the multi-table launch takes; their tables as that launch reads them
    std::vector<uint8_t>    is_dfa, dfa_eligible, dfa_tables;
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
        uint32_t last_dfa_multi = 0, last_dfa_own = 0, last_dfa_items = 0; uint64_t last_dfa_strings = 0;
        bool no_regions[MIX_TIMINGS] = {false};                // a call of the ring that had nothing to scan
        // timing of the last MIX_TIMINGS calls (a ring): first region launch, end of the last region launch, end of the call
        hipEvent_t ev_r0[MIX_TIMINGS] = {nullptr}, ev_r1[MIX_TIMINGS] = {nullptr}, ev_end[MIX_TIMINGS] = {nullptr};
        uint64_t calls = 0;
        uint64_t* d_regions = nullptr; size_t region_bytes = 0;
        uint32_t* d_spill[MIX_MAX_LAUNCHES] = {nullptr}; size_t spill_bytes[MIX_MAX_LAUNCHES] = {0};
        LeanHint lean[MIX_MAX_LAUNCHES];
        unsigned long long* d_counters = nullptr;
        int n_cus = 0;
        uint32_t last_region_launches = 0, last_walk_launches = 0, last_groups = 0;
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
        mx->is_dfa.push_back(dfa ? 1 : 0);
        mx->dfa_eligible.push_back(dfa && dfa_mixed_eligible(img->host) ? 1 : 0);
        if (dfa) { mx->n_dfa++; continue; }
        if (!img->walk_ok) mx->table_ok = false;
        if (mx->n_mem++ == 0) mx->reversed = img->walk.reversed;
        else if (mx->reversed != img->walk.reversed) mx->table_ok = false;                      // one scan direction per table launch
        mx->K = std::max(mx->K, img->walk.K);
        mx->max_live = std::max(mx->max_live, img->walk.max_live);
    }
    if (mx->table_ok)
        for (mfa_image* img : mx->images) {
            mx->block_at.push_back((uint32_t)mx->words.size());
            if (img->host.h.kind != MFA_KIND_MFA) continue;      // (no block)
            if (mx->K > 6 && img->walk.K <= 6) {                  // a kernel for more than 6 cells reads 3-word edges
                WalkTables wide;
                if (build_walk_tables(img->host, wide, true) != MFA_OK) { mx->table_ok = false; break; }
                mx->words.insert(mx->words.end(), wide.words.begin(), wide.words.end());
            } else mx->words.insert(mx->words.end(), img->walk.words.begin(), img->walk.words.end());
        }
    if (mx->n_dfa) {
        std::vector<const HostImage*> hosts;
        for (mfa_image* img : mx->images) hosts.push_back(&img->host);
        mx->dfa_tables = dfa_mixed_pack(hosts, mx->dfa_eligible);
    }
    *out = mx;
    return MFA_OK;
}

void mfa_mixed_destroy(mfa_mixed_t* mx) {
    if (!mx) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (auto& kv : mx->dev) {
        (void)hipSetDevice(kv.first);
        mfa_mixed::Dev& d = kv.second;
        for (hipStream_t w : d.ws) if (w) (void)hipStreamSynchronize(w);
        if (d.calls > 0) (void)hipEventSynchronize(d.ev_end[(d.calls - 1) % MIX_TIMINGS]);      // (region launches on a caller's stream)
        if (d.d_tables) (void)hipFree(d.d_tables);
        if (d.d_dfa) (void)hipFree(d.d_dfa);
        if (d.d_regions) (void)hipFree(d.d_regions);
        for (uint32_t* p : d.d_spill) if (p) (void)hipFree(p);
        for (LeanHint& h : d.lean) lean_hint_free(h);
        if (d.d_counters) (void)hipFree(d.d_counters);
        for (hipEvent_t e : d.ev_g) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : d.ev_w) if (e) (void)hipEventDestroy(e);
        if (d.ev_in) (void)hipEventDestroy(d.ev_in);
        for (uint32_t k = 0; k < MIX_TIMINGS; k++) for (hipEvent_t e : {d.ev_r0[k], d.ev_r1[k], d.ev_end[k]}) if (e) (void)hipEventDestroy(e);
        for (hipStream_t w : d.ws) if (w) (void)hipStreamDestroy(w);
    }
    if (cur >= 0) (void)hipSetDevice(cur);
    delete mx;
}

static int mixed_device(mfa_mixed* mx, int device, mfa_mixed::Dev** out) {
    const int rc = check_device(device);
    if (rc != MFA_OK) return rc;
    auto it = mx->dev.find(device);
    if (it != mx->dev.end()) { *out = &it->second; return MFA_OK; }
    mfa_mixed::Dev d;
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
    auto ins = mx->dev.emplace(device, d);
    *out = &ins.first->second;
    return MFA_OK;
}

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
    const bool table = walk_mode() != 2 && mx->table_ok;      // the table engine unless the generated kernels are asked for
    // groups of strings (walk_plan.h: plan_cuts), by the batch's bytes.  Those are device data (offsets[n] - offsets[0]): a caller that knows
    // them says so (mfa_match_mixed_sized); otherwise they are read back ONCE per string count this object meets -- that call waits for the
    // caller's stream -- and remembered (a later batch with the same count and other bytes gets the same grouping: a matter of speed only).
    const char* spec = getenv("MFA_MIXED_CUTS");
    uint64_t bytes = total_bytes;
    const bool has_mem = mx->n_mem != 0;                      // (without a memory automaton nothing is grouped: the bytes are not needed)
    if (!has_mem) { spec = nullptr; bytes = 1; }
    if (!spec && bytes == 0) {
        auto known = mx->bytes_of.find(n);
        if (known != mx->bytes_of.end()) bytes = known->second;
        else if (n >= 65536) {
            uint64_t ends[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(&ends[0], d_offsets, sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
            HIP_TRY(hipMemcpyAsync(&ends[1], d_offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
            HIP_TRY(hipStreamSynchronize(cs));
            bytes = ends[1] - ends[0];
            if (mx->bytes_of.size() >= 64) mx->bytes_of.clear();
            mx->bytes_of[n] = bytes;
        }
    }
    const std::vector<uint64_t> cut = plan_cuts(n, bytes, table, spec);
    const uint32_t ng = (uint32_t)cut.size() - 1;
    const bool with_regions = regions_enabled() && has_mem;
    const int NW = has_mem ? mixed_walk_streams(table) : 0;

    // One automaton, one group: exactly the single-automaton call (mfa_match_batch: region pass, then the walk, on the caller's stream, with the
    // engine that call would choose) -- the hops to the internal streams and back cost such a batch 0.03-0.06 ms and buy it nothing.  (Cutting a
    // 1.9 GB batch of ONE automaton into two or three groups was measured in round 4, configs[4]: 0.517 ms in one piece, 0.61 / 0.69 / 0.74
    // ms in two / three / four groups: a walk launch is latency-bound, its 0.15 ms are paid per group and hide behind nothing that short.)
    if (ns == 1 && ng == 1 && env_int("MFA_MIXED_SINGLE_DIRECT", 1) != 0) {
        const uint32_t slot1 = (uint32_t)(d->calls % MIX_TIMINGS);
        if (d->calls > 0 && d->last_cs != cs) HIP_TRY(hipStreamWaitEvent(cs, d->ev_end[(d->calls - 1) % MIX_TIMINGS], 0));
        d->last_cs = cs;
        HIP_TRY(hipEventRecord(d->ev_r0[slot1], cs));
        rc = mfa_match_batch(mx->images[0], d_bytes, d_offsets, n, d_results, device, stream);
        HIP_TRY(hipEventRecord(d->ev_r1[slot1], cs));
        HIP_TRY(hipEventRecord(d->ev_end[slot1], cs));
        if (rc != MFA_OK) return rc;
        d->timed = true; d->calls++; d->ng_last = 1;
        d->last_region_launches = with_regions ? 1u : 0u; d->last_walk_launches = has_mem ? 1u : 0u; d->last_groups = 1;
        d->no_regions[slot1] = !has_mem;
        d->last_dfa_multi = 0; d->last_dfa_own = has_mem ? 0u : 1u; d->last_dfa_items = 0; d->last_dfa_strings = 0;
        return MFA_OK;
    }

    // ---- what the call will launch, decided before anything is put on a stream (an error found here leaves the streams untouched)
    std::vector<MixLaunch> plan;
    if (table) {
        std::vector<MixImage> imgs;
        for (uint32_t s = 0; s < ns; s++) imgs.push_back(MixImage{mx->images[s]->walk.K, mx->images[s]->walk.max_live, mx->block_at[s]});
        plan = plan_table_launches(cut, seg_first, imgs, mx->K, (uint32_t)mx->words.size(), NW, mx->n_dfa ? mx->is_dfa.data() : nullptr);
    }
    if (plan.size() > MIX_MAX_LAUNCHES) return MFA_ERR_UNSUPPORTED;      // (more runs of equal cell count than the object has launch slots: nothing was started)
    // the memory-less segments: the items of the multi-table launch, and the segments with a launch of their own (walk_plan.h)
    DfaPlan dfa;
    if (mx->n_dfa) {
        std::vector<DfaImage> di;
        for (uint32_t s = 0; s < ns; s++)
            di.push_back(DfaImage{mx->is_dfa[s] != 0, mx->dfa_eligible[s] != 0, mx->images[s]->host.h.is_reversed != 0,
                                  mx->is_dfa[s] ? dfa_mixed_table_bytes(mx->images[s]->host) : 0u});
        dfa = plan_dfa_items(seg_first, di, table, dfa_knobs());
        if (!dfa.items.empty() && !d->d_dfa) {
            HIP_TRY(hipMalloc((void**)&d->d_dfa, mx->dfa_tables.size()));
            HIP_TRY(hipMemcpy(d->d_dfa, mx->dfa_tables.data(), mx->dfa_tables.size(), hipMemcpyHostToDevice));
        }
    }
    const bool has_dfa = !dfa.items.empty() || !dfa.own.empty();
    // the stream of the memory-less segments: one beyond the walk streams while the object may have one, else the last walk stream (they go first)
    const int KD = has_dfa ? std::min(NW, (int)MIX_MAX_STREAMS - 1) : -1;
    const int NS = std::max(NW, KD + 1);
    uint64_t* d_table = nullptr;
    if (with_regions) {
        rc = ctx_reserve((void**)&d->d_regions, &d->region_bytes, (size_t)n * MFA_REGION_WORDS * sizeof(uint64_t));
        if (rc != MFA_OK) return rc;
        d_table = d->d_regions;
    }
    // which stream walks which segment (generated kernels): first call one after the other (timed), then by cost
    const bool calibrating = !table && !d->calibrated && has_mem;
    const std::vector<int> where = !table && d->calibrated && d->ng_last == ng ? assign_streams(cut, seg_first, ns, d->ready, d->cost.data(), NW) : std::vector<int>(ns, 0);
    for (int k = 0; k < NS; k++)
        if (!d->ws[k]) HIP_TRY(hipStreamCreateWithFlags(&d->ws[k], hipStreamNonBlocking));
    const uint32_t slot_t = (uint32_t)(d->calls % MIX_TIMINGS);
    // ---- from here on work goes to the internal streams.  Whatever happens, the caller's stream is made to wait for all of it before this
    // function returns: a caller that gets an error may free or reuse its buffers in stream order like one that gets MFA_OK.
    struct Join {
        mfa_mixed::Dev* d; hipStream_t cs; int NW; uint32_t slot_t; bool used[MIX_MAX_STREAMS] = {false}; bool started = false; int err = MFA_OK;
        void run() {
            if (!started) return;
            started = false;
            for (int k = 0; k < NW; k++)
                if (used[k]) {
                    if (hipEventRecord(d->ev_w[k], d->ws[k]) != hipSuccess || hipStreamWaitEvent(cs, d->ev_w[k], 0) != hipSuccess) { err = MFA_ERR_HIP; (void)hipStreamSynchronize(d->ws[k]); }
                }
            if (hipEventRecord(d->ev_end[slot_t], cs) != hipSuccess) { err = MFA_ERR_HIP; (void)hipStreamSynchronize(cs); }
        }
        ~Join() { run(); }
    } join{d, cs, NS, slot_t};
    // (the object's buffers -- table, counters, spill areas -- are shared by its calls: a call starts behind the end of the one before it,
    // whichever stream that one came on)
    if (d->calls > 0 && d->last_cs != cs) HIP_TRY(hipStreamWaitEvent(cs, d->ev_end[(d->calls - 1) % MIX_TIMINGS], 0));      // (the walk streams start behind ev_in: below)
    d->last_cs = cs;
    HIP_TRY(hipEventRecord(d->ev_in, cs));
    join.started = true;
    for (int k = 0; k < NS; k++) HIP_TRY(hipStreamWaitEvent(d->ws[k], d->ev_in, 0));
    // the memory-less segments wait for nothing else: they run beside the region launches
    uint32_t dfa_multi = 0;
    if (has_dfa) {
        join.used[KD] = true;
        for (size_t i0 = 0; i0 < dfa.items.size(); i0 += kDfaMaxItems) {
            rc = launch_dfa_mixed(dfa, i0, std::min(dfa.items.size(), i0 + kDfaMaxItems), d->d_dfa, d->n_cus, d_bytes, d_offsets, n, d_results, d->ws[KD]);
            if (rc != MFA_OK) return rc;
            dfa_multi++;
        }
        for (uint32_t s : dfa.own) {
            rc = mfa_match_batch(mx->images[s], d_bytes, d_offsets + seg_first[s], seg_first[s + 1] - seg_first[s], d_results + seg_first[s], device, d->ws[KD]);
            if (rc != MFA_OK) return rc;
        }
    }
    // The region launches go to the CALLER's stream: back-to-back calls pass from the last walk of one to the first region launch of the next
    // through ONE event (walk stream -> caller's stream) instead of three through a region stream of the object's own: 0.02 ms a call.
    HIP_TRY(hipEventRecord(d->ev_r0[slot_t], cs));
    uint32_t region_launches = 0;
    uint32_t slot = 0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint64_t lo = cut[g], hi = cut[g + 1];
        // a group's event: the table engine's is its region launch's completion signal (no packet of its own between region launches)
        bool g_event = false;                                   // the group's event is its (last) region launch's completion signal
        if (with_regions && !mx->n_dfa) {
            rc = launch_region_scan(d->n_cus, d_bytes, d_offsets + lo, hi - lo, d_table + lo * MFA_REGION_WORDS, cs, table ? 128u : 256u, table ? d->ev_g[g] : nullptr);
            if (rc != MFA_OK) return rc;
            region_launches++;
            g_event = table;
        } else if (with_regions) {
            // an object with memory-less automata: one launch per run of memory segments in the group -- their strings are not scanned
            uint32_t ra, rb;
            segments_of(seg_first, ns, lo, hi, ra, rb);
            std::vector<std::pair<uint64_t, uint64_t>> runs;
            for (uint32_t s = ra; s < rb; s++) {
                const uint64_t a = std::max(seg_first[s], lo), b = std::min(seg_first[s + 1], hi);
                if (mx->is_dfa[s] || b <= a) continue;
                if (!runs.empty() && runs.back().second == a) runs.back().second = b; else runs.emplace_back(a, b);
            }
            for (size_t r = 0; r < runs.size(); r++) {
                const bool last = r + 1 == runs.size();
                rc = launch_region_scan(d->n_cus, d_bytes, d_offsets + runs[r].first, runs[r].second - runs[r].first, d_table + runs[r].first * MFA_REGION_WORDS, cs,
                                        table ? 128u : 256u, table && last ? d->ev_g[g] : nullptr);
                if (rc != MFA_OK) return rc;
                region_launches++;
                g_event = table;
            }
        }
        if (!g_event) HIP_TRY(hipEventRecord(d->ev_g[g], cs));
        // a stream's first launch of this group waits for the group's event
        bool waits[MIX_MAX_STREAMS] = {false};
        if (table) {
            for (const MixLaunch& L : plan) {
                if (L.g != g) continue;
                void* wait_for = nullptr;                       // (the launch itself waits, behind its own preparations on the stream)
                if (!waits[L.k]) { waits[L.k] = true; wait_for = d->ev_g[g]; }
                const WalkPlanInput pk{L.Kc, L.ml, mx->reversed, L.w1 - L.w0};
                join.used[L.k] = true;
                rc = launch_walk(pk, d->d_tables + L.w0, d->n_cus, d_bytes, d_offsets + L.a, L.b - L.a, d_results + L.a, d_table ? d_table + L.a * MFA_REGION_WORDS : nullptr,
                                 L.s1 - L.s0, L.sf, L.stb, &d->d_spill[slot], &d->spill_bytes[slot], d->d_counters + 64 * slot, d->ws[L.k], &d->lean[slot], wait_for);
                if (rc != MFA_OK) return rc;
                slot++;
            }
        } else {
            uint32_t sa, sb;
            segments_of(seg_first, ns, lo, hi, sa, sb);
            for (uint32_t s = sa; s < sb; s++) {
                const uint64_t a = std::max(seg_first[s], lo), b = std::min(seg_first[s + 1], hi);
                if (b <= a || mx->is_dfa[s]) continue;
                const int k = where[s];
                if (!waits[k]) { waits[k] = true; HIP_TRY(hipStreamWaitEvent(d->ws[k], d->ev_g[g], 0)); }
                join.used[k] = true;
                rc = mfa_match_batch_regions(mx->images[s], d_bytes, d_offsets + a, b - a, d_results + a, d_table ? d_table + a * MFA_REGION_WORDS : nullptr, device, d->ws[k]);
                if (rc != MFA_OK) return rc;
                slot++;
            }
        }
    }
    HIP_TRY(hipEventRecord(d->ev_r1[slot_t], cs));
    // the caller's stream (and with it the call's end event) waits for every stream that was given work
    join.run();
    if (join.err != MFA_OK) return join.err;
    d->timed = true;
    d->calls++;
    d->ng_last = ng;
    d->last_region_launches = region_launches; d->last_walk_launches = slot; d->last_groups = ng;
    d->no_regions[slot_t] = region_launches == 0 && mx->n_dfa != 0;
    d->last_dfa_multi = dfa_multi; d->last_dfa_own = (uint32_t)dfa.own.size(); d->last_dfa_items = (uint32_t)dfa.items.size(); d->last_dfa_strings = dfa.strings;
    if (calibrating) {                                        // once per device: the walks' costs and the groups' region times
        HIP_TRY(hipEventSynchronize(d->ev_end[slot_t]));
        for (uint32_t s = 0; s < ns; s++) {
            float ms = 0.0f;
            if (seg_first[s + 1] > seg_first[s] && !mx->is_dfa[s] && mfa_last_kernel_ms(mx->images[s], device, &ms) == MFA_OK) d->cost[s] = ms;
        }
        for (uint32_t g = 0; g < ng; g++) {
            // the calibration pass runs a group's walks before the next group's region launch is reached by nothing: region launches
            // follow each other on the caller's stream, so the elapsed time between two group events is the later group's region time
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, d->ev_r0[slot_t], d->ev_g[g]));
            d->ready[g] = ms;
        }
        d->calibrated = true;
    }
    return MFA_OK;
}

int mfa_match_mixed(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* seg_first,
                    uint8_t* d_results, int device, void* stream) {
    return match_mixed_impl(mx, d_bytes, d_offsets, n, seg_first, d_results, device, stream, 0);
}

int mfa_match_mixed_sized(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint64_t total_bytes, const uint64_t* seg_first,
                          uint8_t* d_results, int device, void* stream) {
    return match_mixed_impl(mx, d_bytes, d_offsets, n, seg_first, d_results, device, stream, total_bytes);
}

// what the last call on `device` launched (any pointer may be NULL): region launches, walk launches, groups of strings, and `gated`, always 0
// (kept for compatibility)
int mfa_mixed_last_launches(mfa_mixed_t* mx, int device, uint32_t* region_launches, uint32_t* walk_launches, uint32_t* groups, uint32_t* gated) {
    if (!mx) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(mx->mu);
    auto it = mx->dev.find(device);
    if (it == mx->dev.end() || !it->second.timed) return MFA_ERR_INVALID_ARG;
    if (region_launches) *region_launches = it->second.last_region_launches;
    if (walk_launches) *walk_launches = it->second.last_walk_launches;
    if (groups) *groups = it->second.last_groups;
    if (gated) *gated = 0u;
    return MFA_OK;
}

// what the last call on `device` did with its memory-less segments (any pointer may be NULL): multi-table launches, launches of single
// segments, and the items and strings of the multi-table launches
int mfa_mixed_last_dfa(mfa_mixed_t* mx, int device, uint32_t* multi_launches, uint32_t* own_launches, uint32_t* items, uint64_t* strings) {
    if (!mx) return MFA_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(mx->mu);
    auto it = mx->dev.find(device);
    if (it == mx->dev.end() || !it->second.timed) return MFA_ERR_INVALID_ARG;
    if (multi_launches) *multi_launches = it->second.last_dfa_multi;
    if (own_launches) *own_launches = it->second.last_dfa_own;
    if (items) *items = it->second.last_dfa_items;
    if (strings) *strings = it->second.last_dfa_strings;
    return MFA_OK;
}

// The same with HOST pointers: copies the batch to the device, matches, copies the results back, synchronises (the host mirror's
// match_mixed and the `diploma -match-mixed` command line; throughput is then bounded by the host link).
int mfa_match_mixed_host(mfa_mixed_t* mx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, const uint64_t* seg_first, uint8_t* results, int device) {
    if (!mx || !seg_first) return MFA_ERR_INVALID_ARG;
    return match_host_staged(bytes, offsets, n, results, device, [&](const uint8_t* d_bytes, const uint64_t* d_off, uint8_t* d_res, uint64_t total) {
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
