// What a walk launch and a mixed call will do, decided by pure functions: no HIP, no stream, no memory but std::vector's.  walk_launch.hip
// calls these, and then only allocates, enqueues and launches what they say; tests/emul/plan_emul.cpp runs the same
// functions on a machine without a GPU (tests/test_walk_plan_cpu.py).  The layout of a wave's memory is walk.h's WalkLayout.
#ifndef MFA_WALK_PLAN_H
#define MFA_WALK_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mfa_hip.h"
#include "walk.h"

namespace mfa {

inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}
inline bool env_is_off(const char* name) { const char* e = getenv(name); return e && e[0] == '0'; }
// MFA_REGIONS=0 (or MFA_ACCEL=0): no region pass and no table: every step is executed (A/B runs)
inline bool regions_enabled() { return !env_is_off("MFA_REGIONS") && !env_is_off("MFA_ACCEL"); }

inline int walk_mode() {        // MFA_WALK: 0 automatic (default), 1 "table", 2 "jit"
    const char* e = getenv("MFA_WALK");
    return !e ? 0 : e[0] == 't' ? 1 : e[0] == 'j' ? 2 : 0;
}

// ---- one walk launch ---------------------------------------------------------------------------------------------------------------
struct WalkPlanInput { uint32_t K, max_live; bool reversed; uint32_t table_words; };

// Whether the lean kernel behind a table walk (walk.hip: strings without periodic stretches) has had anything to do lately: the kernel
// reports the length of its queue (+ 1) to a word of pinned host memory, and a launch whose slot last saw an empty queue leaves the lean
// kernel and the queue out (an empty launch beside a region pass costs the stream 0.1-0.35 ms: its workgroups -- 128 VGPRs, LDS for the
// tables and the lists -- queue for room like any other) -- except every 32nd time, with a quarter of the grid, to notice when the input changes.
struct LeanHint {
    uint32_t* h_seen = nullptr;      // pinned, device-visible; 0 = nothing reported yet
    uint32_t quiet = 0, launches = 0;
};
enum class Lean { off, on, probe };

// every MFA_WALK_* / MFA_ACCEL value a launch depends on, read from the environment on every call
struct WalkKnobs {
    bool tables_global, images_global, accel, long_lists, stats;
    int refill, want_c, wgs, waves_per_cu, grid_pct, spill_mb, lean;
};
inline WalkKnobs walk_knobs() {
    WalkKnobs k;
    k.tables_global = getenv("MFA_WALK_TABLES_GLOBAL") != nullptr;      // development: the tables stay in global memory
    k.images_global = env_int("MFA_WALK_IMAGES_GLOBAL", 0) != 0;
    k.accel = !env_is_off("MFA_ACCEL");
    k.long_lists = env_int("MFA_WALK_LONG", 1) != 0;
    k.stats = getenv("MFA_WALK_STATS") != nullptr;
    k.refill = std::max(1, std::min(64, env_int("MFA_WALK_REFILL", 1)));
    k.want_c = env_int("MFA_WALK_C", 0);
    k.wgs = env_int("MFA_WALK_WGS", 0);                        // workgroups per CU to leave LDS for (0: by the size of the batch)
    k.waves_per_cu = env_int("MFA_WALK_WAVES_PER_CU", 0);      // development knob (multiples of 4)
    k.grid_pct = env_int("MFA_WALK_GRID_PCT", 100);
    k.spill_mb = std::max(1, env_int("MFA_WALK_SPILL_MB", 2048));
    k.lean = env_int("MFA_WALK_LEAN", 1);                      // 0: never, 2: always
    return k;
}

// `seen`: what the last lean kernel of this slot that has ended found (+ 1; 0: none has reported yet)
inline Lean lean_decide(uint32_t seen, LeanHint& h, const WalkKnobs& kn) {
    h.quiet = seen == 1u ? h.quiet + 1u : 0u;
    Lean d = Lean::on;
    if (h.quiet >= 1u && kn.lean != 2) d = (h.launches & 31u) != 0u ? Lean::off : Lean::probe;
    h.launches++;
    return d;
}

// Fills everything of L but the pointers and the segment arrays of L.args.  The LDS capacity C of the lists: enough for the automata's
// longest possible list if that leaves room for two workgroups per CU, else what does (longer lists spill).
// lean: Lean::off also when the launch has no region table, MFA_ACCEL=0 or MFA_WALK_LEAN=0.
inline int plan_walk(const WalkPlanInput& p, const WalkKnobs& kn, uint64_t n, int n_cus, uint32_t n_seg, Lean lean, WalkLaunch& L) {
    if (n_seg == 0 || n_seg > WALK_MAX_SEG || n > 0xffffffffull) return MFA_ERR_INVALID_ARG;
    L = WalkLaunch{};
    WalkArgs& a = L.args;
    a.n = n; a.n_seg = n_seg;
    a.table_words = p.table_words;
    a.shared_words = (p.table_words + 63u) & ~63u;
    const size_t lds_max = WALK_LDS_BYTES / 4u;                 // words
    // tables beyond a third of the LDS (or forced: development) stay in global memory
    L.tables_global = a.shared_words > lds_max / 3u || kn.tables_global;
    if (L.tables_global) a.shared_words = 0;
    a.accel = kn.accel ? 1u : 0u;
    a.refill = (uint32_t)kn.refill;
    a.images_global = kn.images_global ? 1u : 0u;
    L.K = p.K; L.reversed = p.reversed;
    // one-cell automata with long lists (the 77-node ex. 8 -bnf / -reverse) have a kernel of their own, which finds a node's entry through a
    // per-lane map in LDS: one byte per node and lane (automata of up to 128 nodes; beyond them the general kernel's key search)
    const bool long_lists = p.K == 1 && p.max_live > 16u && p.max_live < 128u && kn.long_lists && !kn.stats;
    L.kernel = kn.stats && p.K == 1 ? WalkKernel::stats : long_lists ? WalkKernel::long_k1 : WalkKernel::plain;
    a.nm_words = long_lists ? (p.max_live + 1u + 3u) / 4u : 0u;
    const auto layout = [&](uint32_t C, bool lean_walk) { return WalkLayout{p.K, C, p.max_live > C ? p.max_live - C : 1u, kn.images_global, lean_walk, a.nm_words}; };
    const auto lds_words = [&](uint32_t C) { return (size_t)a.shared_words + 4u * (size_t)layout(C, false).lds_words(); };
    // two workgroups per CU when the batch fills the device; a batch that does not even give every CU one workgroup leaves the LDS to that
    // one: longer lists stay in LDS (the 77-node automata: lists of 10, three entries of them in LDS at two workgroups per CU)
    const uint64_t cus = (uint64_t)(n_cus > 0 ? n_cus : 256), want = (n + 255) / 256;
    const uint32_t wgs_goal = kn.wgs != 0 ? (uint32_t)kn.wgs : want <= cus ? 1u : 2u;
    uint32_t C = std::max(1u, std::min(p.max_live, kn.want_c > 0 ? (uint32_t)kn.want_c : 8u));
    while (C > 1 && kn.want_c <= 0 && lds_words(C) > lds_max / wgs_goal) C--;
    while (C > 1 && lds_words(C) > lds_max) C--;
    if (lds_words(C) > lds_max) return MFA_ERR_UNSUPPORTED;      // the tables alone fill the LDS
    const WalkLayout full = layout(C, false), lean_lay = layout(C, true);
    a.C = C; a.CX = full.CX;
    L.lds_bytes = walk_lds_bytes(a.shared_words, full);
    uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(8, lds_max / lds_words(C)));
    if (kn.waves_per_cu > 0 && (uint64_t)(kn.waves_per_cu + 3) / 4 < per_cu) per_cu = (uint64_t)(kn.waves_per_cu + 3) / 4;
    uint64_t grid = cus * per_cu;
    // development: a fraction of the workgroups the device holds (fewer walk waves beside the region pass, each taking more tickets)
    if (kn.grid_pct > 0 && kn.grid_pct < 100) grid = std::max<uint64_t>(1, grid * (uint64_t)kn.grid_pct / 100u);
    if (grid > want) grid = want;
    // What a wave may spill (list entries and probe images beyond the LDS capacity) is sized for the worst case -- every node of the launch's
    // largest automaton alive at once -- per wave of the grid: 4.7 MB per wave for 1024 nodes and one cell.  The grid shrinks (the waves are
    // persistent: fewer of them take more tickets each) until that fits a budget, 2 GiB by default; what does not fit with ONE workgroup is MFA_ERR_NOMEM.
    const size_t per_wave = full.spill_words() * sizeof(uint32_t);
    const size_t budget = (size_t)kn.spill_mb << 20;
    while (grid > 1 && grid * 4u * per_wave > budget) grid = (grid + 1) / 2;
    if (grid * 4u * per_wave > budget) return MFA_ERR_NOMEM;
    L.grid = (unsigned)grid;
    // the lean kernel behind it: the plain step only, lists of the same capacity, four workgroups per CU where the LDS allows; its waves'
    // spill areas and the queue of string numbers share the buffer with this launch's.  A look (Lean::probe) takes a quarter of the grid.
    L.lean_C = a.C; L.lean_CX = a.CX;
    L.lean_lds_bytes = walk_lds_bytes(a.shared_words, lean_lay);
    size_t lean_bytes = 0;
    const uint64_t lean_per_cu = std::min<uint64_t>(4, (size_t)WALK_LDS_BYTES / L.lean_lds_bytes);
    if (lean != Lean::off && lean_per_cu >= 1) {
        uint64_t lg = cus * lean_per_cu;
        if (lean == Lean::probe) lg = std::max<uint64_t>(1, lg / 4u);
        if (lg > want) lg = want;
        const size_t lean_per_wave = lean_lay.spill_words() * sizeof(uint32_t);
        while (lg > 1 && lg * 4u * lean_per_wave > budget) lg = (lg + 1) / 2;
        L.lean_grid = (unsigned)lg;
        lean_bytes = (size_t)lg * 4u * lean_per_wave;
    }
    const size_t need = std::max((size_t)grid * 4u * per_wave, lean_bytes);
    L.queue_at = (need + 255u) & ~(size_t)255u;
    L.spill_bytes = L.queue_at + (L.lean_grid ? (size_t)n * sizeof(uint32_t) : 0);
    if (L.kernel == WalkKernel::stats) L.lean_grid = 0;        // (the counting build has no lean kernel behind it)
    L.counter_words = L.kernel == WalkKernel::stats ? 32u : 3u;      // ticket counter, queue length, the lean kernel's tickets
    return MFA_OK;
}

// ---- a mixed call --------------------------------------------------------------------------------------------------------------------
constexpr uint32_t MIX_MAX_GROUPS = 12, MIX_MAX_STREAMS = 4, MIX_MAX_LAUNCHES = 24;

// Groups: ranges of strings, cut at fractions of the batch (a segment may straddle a cut).  Decreasing sizes: the walk of the last group
// is what the call ends with.  spec: MFA_MIXED_CUTS (fractions, comma separated), or nullptr: by the batch's bytes.
// How many groups pays depends on the batch's BYTES: a group's region launch should take about as long as a walk launch needs anyway
// (a walk is latency-bound: ~0.3-0.5 ms for 20 000 strings as for 200 000): 1.3 GB per group, eight groups at most (measured: 10.7 GB of
// 64 KiB strings 2.02 ms in eight groups, 2.28 ms in four; the 19.4 GB headline batch eight).  Cut finer, a small batch pays the walks'
// latency once per group (a 1.9 GB batch of one automaton: 1.26 ms in eight groups against 0.52 ms in one; 34 ms against 9.8 ms
// for the 77-node automaton).
inline std::vector<uint64_t> plan_cuts(uint64_t n, uint64_t bytes, bool table, const char* spec) {
    std::string made;
    if (!spec) {
        const double per_group = table ? 1.3e9 : 2.0e9;
        const uint32_t most = table ? 8u : 5u;
        uint32_t want = (uint32_t)std::min<double>(most, std::max(1.0, std::floor((double)bytes / per_group + 0.5)));
        if (n < 65536) want = 1;
        // sizes: equal, the last three groups 0.8 / 0.53 / 0.33 of that (two groups: 1, 0.6; three: 1, 0.8, 0.4)
        std::vector<double> w(want, 1.0);
        if (want == 2) w[1] = 0.6;
        else if (want == 3) { w[1] = 0.8; w[2] = 0.4; }
        else if (want >= 4) { w[want - 3] = 0.8; w[want - 2] = 0.53; w[want - 1] = 0.33; }
        double total = 0, acc = 0;
        for (double x : w) total += x;
        for (uint32_t k = 0; k + 1 < want; k++) { acc += w[k]; made += (k ? "," : "") + std::to_string(acc / total); }
        spec = made.c_str();
    }
    std::vector<uint64_t> cut{0};
    for (const char* q = spec; *q && cut.size() < MIX_MAX_GROUPS;) {
        const uint64_t at = (uint64_t)((double)n * atof(q));
        if (at > cut.back() && at < n) cut.push_back(at);
        while (*q && *q != ',') q++;
        if (*q == ',') q++;
    }
    cut.push_back(n);
    return cut;
}

// the segments [first, second) that have strings in [lo, hi)
inline void segments_of(const uint64_t* seg_first, uint32_t ns, uint64_t lo, uint64_t hi, uint32_t& sa, uint32_t& sb) {
    sa = 0;
    while (sa + 1 < ns && seg_first[sa + 1] <= lo) sa++;
    sb = sa;
    while (sb < ns && seg_first[sb] < hi) sb++;
}

// What planning needs to know of an automaton of the object (mfa_mixed_create fills one per image, once).  A memory automaton: cells,
// longest list, and block_at, the word offset of its table block in the object's tables.  A memory-less one (walked by the table kernels:
// plan_dfa_items below; no walk launch holds it, no region launch scans it): whether the multi-table launch takes it, its scan direction,
// and table_bytes, its fused LDS table (n_states * kDfaRow * 2).
struct MixImage { uint32_t K, max_live, block_at; bool memoryless, eligible, reversed; uint32_t table_bytes; };

// Table engine: one launch per group and run of consecutive segments whose automata have the same number of cells (a launch's kernel and
// its LDS footprint are those of its largest cell count; an object with an automaton of more than 6 cells walks all with that kernel: K);
// groups alternate between the NW walk streams, so that a group's walk may start while the one before it drains.  A run ends in front
// of a memory-less segment.  Per-segment engine: a launch is one segment's strings in one group, [s0, s1) = that segment, and nothing of
// the table fields is used.
struct MixLaunch {
    uint32_t g, s0, s1, ml, Kc, w0, w1;      // group, segments [s0, s1), longest list, cells, table words [w0, w1)
    uint64_t a, b;                           // strings [a, b)
    int k;                                   // walk stream
    uint32_t sf[WALK_MAX_SEG + 1], stb[WALK_MAX_SEG];      // launch_walk's seg_first / seg_table
    uint32_t slot;                           // its place in the call's enqueue order: the spill area, counters and lean hint it uses
    bool waits;                              // the first launch of its stream in its group: it waits for the group's event
};
inline std::vector<MixLaunch> plan_table_launches(const std::vector<uint64_t>& cut, const uint64_t* seg_first, const std::vector<MixImage>& img, uint32_t K,
                                                  uint32_t total_words, int NW) {
    const uint32_t ns = (uint32_t)img.size();
    std::vector<MixLaunch> plan;
    for (uint32_t g = 0; g + 1 < cut.size(); g++) {
        const uint64_t lo = cut[g], hi = cut[g + 1];
        uint32_t sa, sb;
        segments_of(seg_first, ns, lo, hi, sa, sb);
        for (uint32_t s0 = sa; s0 < sb;) {
            if (img[s0].memoryless) { s0++; continue; }
            uint32_t s1 = s0 + 1;
            const uint32_t Kc = K > 6 ? K : img[s0].K;
            while (s1 < sb && s1 - s0 < WALK_MAX_SEG && (K > 6 || img[s1].K == Kc) && !img[s1].memoryless) s1++;
            MixLaunch L{};
            L.a = std::max(seg_first[s0], lo); L.b = std::min(seg_first[s1], hi);
            if (L.b > L.a) {
                L.g = g; L.s0 = s0; L.s1 = s1; L.Kc = Kc; L.k = (int)(g % (uint32_t)NW); L.ml = 1;
                // the launch gets the blocks of ITS automata only (they lie back to back): less LDS per workgroup
                L.w0 = img[s0].block_at; L.w1 = s1 < ns ? img[s1].block_at : total_words;
                for (uint32_t j = s0; j < s1; j++) { L.ml = std::max(L.ml, img[j].max_live); L.stb[j - s0] = img[j].block_at - L.w0; }
                for (uint32_t j = s0; j <= s1; j++) L.sf[j - s0] = (uint32_t)(std::min(std::max(seg_first[j], L.a), L.b) - L.a);
                plan.push_back(L);
            }
            s0 = s1;
        }
    }
    return plan;
}

// Generated kernels: which walk stream walks which segment, by measured cost (list scheduling with the groups' region times `ready` as
// release times).  A segment's walk is released when the group that holds its first string is scanned (segments that straddle a cut are rare).
inline std::vector<int> assign_streams(const std::vector<uint64_t>& cut, const uint64_t* seg_first, uint32_t ns, const float* ready, const float* cost, int NW) {
    std::vector<int> where(ns, 0);
    const uint32_t ng = (uint32_t)cut.size() - 1;
    float free_at[MIX_MAX_STREAMS] = {0};
    for (uint32_t s = 0, g = 0; s < ns; s++) {
        while (g + 1 < ng && cut[g + 1] <= seg_first[s]) g++;
        int best = 0;
        for (int k = 1; k < NW; k++)
            if (std::max(free_at[k], ready[g]) < std::max(free_at[best], ready[g])) best = k;
        free_at[best] = std::max(free_at[best], ready[g]) + 1.5f * cost[s];      // beside the region pass a walk takes about 1.5 x its time alone
        where[s] = best;
    }
    return where;
}

// ---- the memory-less segments of a mixed call -----------------------------------------------------------------------------------------
// They need no regions, so they are walked beside the region pass, behind the call's entry event only.  Segments whose table fits the
// tiled table kernel's LDS ("eligible": kernels.hip, launch_dfa_walk's 64 KiB rule) share ONE launch of dfa_mixed_kernel (dfa_mixed.hip);
// the others -- tables in L2, tables beyond 64 KiB with the tile, every memory-less segment of a call on the per-segment schedule
// (MFA_WALK=jit), and segments so large that a launch of their own pays -- get a launch of their own through launch_dfa_walk.
// An item is what the multi-table launch is given: one segment's strings.  The kernel cuts an item into slices of kDfaSliceStrings
// strings, one per lane of a workgroup; a workgroup takes a run of consecutive slices (dfa_slice_lo).
constexpr uint32_t kDfaSliceStrings = 256;      // one workgroup, one string per lane
constexpr uint32_t kDfaMaxItems = 96;           // items per launch: they travel as kernel arguments (no upload, nothing that outlives the launch)
// Neither default rests on a measurement yet (tools/mixed_dfa.py has not been run on an MI355X).  Until it has, the
// multi-table launch is OFF unless MFA_MIXED_DFA=1 asks for it -- every memory-less segment then gets the launch mfa_match_batch gives it,
// code whose speed is known -- and the size from which a segment leaves the multi-table launch is an estimate: 32768 strings of 1 KiB are
// 32 MiB, about what one workgroup per CU-slot of the tiled kernel's own grid takes in one round.
constexpr int      kDfaMultiDefault = 0;        // MFA_MIXED_DFA
constexpr uint64_t kDfaOwnDefault = 32768;      // MFA_MIXED_DFA_OWN

// slices of an item; the first slice of workgroup `wg` of `wgs` (its last: the next workgroup's first): consecutive slices, so that a
// workgroup changes its table as seldom as possible
constexpr uint64_t dfa_slices_of(uint64_t count) { return (count + kDfaSliceStrings - 1) / kDfaSliceStrings; }
constexpr uint64_t dfa_slice_lo(uint64_t slices, uint64_t wg, uint64_t wgs) { return slices * wg / wgs; }

struct DfaItem { uint64_t first; uint32_t count, image; };                         // strings [first, first + count) of the batch, automaton `image`
struct DfaKnobs { bool multi; uint64_t own_min; };
inline DfaKnobs dfa_knobs() {
    DfaKnobs k;
    k.multi = env_int("MFA_MIXED_DFA", kDfaMultiDefault) != 0;      // 0: every memory-less segment gets its own launch; 1: the multi-table launch
    const char* e = getenv("MFA_MIXED_DFA_OWN");              // strings from which a segment gets its own launch
    k.own_min = e && *e ? strtoull(e, nullptr, 10) : kDfaOwnDefault;
    return k;
}
struct DfaPlan {
    std::vector<DfaItem> items;      // in segment order: slices of one automaton lie side by side
    std::vector<uint32_t> own;       // segments with a launch of their own
    uint32_t table_bytes = 0;        // the largest table of the items
    uint64_t strings = 0, slices = 0;      // of the items
};
// table_schedule: the call walks its memory automata with the table engine (else every memory-less segment gets its own launch).
// Image: MixImage, or just the part of it that is read here
struct DfaImage { bool memoryless, eligible, reversed; uint32_t table_bytes; };
template <class Image> DfaPlan plan_dfa_items(const uint64_t* seg_first, const std::vector<Image>& img, bool table_schedule, const DfaKnobs& kn) {
    DfaPlan P;
    for (uint32_t s = 0; s < (uint32_t)img.size(); s++) {
        const uint64_t cnt = seg_first[s + 1] - seg_first[s];
        if (!img[s].memoryless || cnt == 0) continue;
        if (!kn.multi || !table_schedule || !img[s].eligible || cnt >= kn.own_min || cnt > 0xffffffffull) { P.own.push_back(s); continue; }
        P.items.push_back(DfaItem{seg_first[s], (uint32_t)cnt, s});
        P.table_bytes = std::max(P.table_bytes, img[s].table_bytes);
        P.strings += cnt;
        P.slices += dfa_slices_of(cnt);
    }
    return P;
}

// ---- the whole schedule of a mixed call -------------------------------------------------------------------------------------------------
// plan_mixed composes the pieces above into everything mfa_match_mixed puts on a stream, in that order: walk_launch.hip only makes buffers
// and streams, records, waits and launches.  The region launches go to the caller's stream, group after group; a group's event says "its
// regions are known"; what walks a group goes to the NW walk streams behind that event and runs beside the next group's region pass.
struct MixObject { uint32_t K, total_words, n_mem, n_dfa; bool table_ok; };      // K: most cells of a memory automaton; the object's table words
// every variable a mixed call's schedule depends on, read from the environment once per call
struct MixKnobs {
    int walk;                    // MFA_WALK (walk_mode): 2 = the per-segment engine (generated kernels)
    bool regions;                // MFA_REGIONS / MFA_ACCEL
    const char* cuts;            // MFA_MIXED_CUTS as it is given, or nullptr
    bool single_direct;          // MFA_MIXED_SINGLE_DIRECT (default 1)
    int walk_streams[2];         // MFA_MIXED_WALK_STREAMS for the per-segment engine (default 3) and for the table engine (default 2)
    DfaKnobs dfa;                // MFA_MIXED_DFA, MFA_MIXED_DFA_OWN
};
inline int mixed_walk_streams(bool table) { return std::max(1, std::min((int)MIX_MAX_STREAMS, env_int("MFA_MIXED_WALK_STREAMS", table ? 2 : 3))); }
inline MixKnobs mixed_knobs() {
    return MixKnobs{walk_mode(), regions_enabled(), getenv("MFA_MIXED_CUTS"), env_int("MFA_MIXED_SINGLE_DIRECT", 1) != 0, {mixed_walk_streams(false), mixed_walk_streams(true)}, dfa_knobs()};
}
// what the object's first call on a device on the per-segment engine measured: ready[MIX_MAX_GROUPS], cost[one per image]
struct MixCalib { bool calibrated; uint32_t ng_last; const float* ready; const float* cost; };

// group, strings [a, b): a run of memory segments' strings inside the group; signals: its completion signal is the group's event (no packet of its own)
struct MixRegion { uint32_t g; uint64_t a, b; uint32_t threads; bool signals; };
struct MixPlan {
    int rc = MFA_OK;                // MFA_ERR_UNSUPPORTED: more table launches than the object has slots (nothing may be started)
    bool table = false;             // the table engine walks the memory automata (else one launch per segment)
    bool direct = false;            // one automaton, one group: exactly mfa_match_batch on the caller's stream; the lists below stay empty
    bool with_regions = false, calibrating = false;      // the call's own region launches fill a table; its walks are timed when it is over
    int NW = 0, KD = -1, NS = 0;    // walk streams; the stream of the memory-less segments (-1: none); streams in all
    std::vector<uint64_t> cut;
    std::vector<int> where;         // per-segment engine: the walk stream of each segment
    std::vector<MixRegion> regions; // in enqueue order
    bool own_event[MIX_MAX_GROUPS] = {false};      // the group's event is recorded by itself behind the group's region launches
    std::vector<MixLaunch> walks;   // in enqueue order: a group's follow its region launches and its event
    DfaPlan dfa;
    std::vector<std::pair<uint32_t, uint32_t>> dfa_multi;      // items [first, second) of each multi-table launch
    uint32_t n_regions = 0, n_walks = 0, n_groups = 0, n_dfa_multi = 0, n_dfa_own = 0, n_dfa_items = 0;      // what mfa_mixed_last_launches and
    uint64_t dfa_strings = 0;                                                                                 // mfa_mixed_last_dfa report
    bool no_regions = false;        // the call had nothing to scan (mfa_mixed_timing: a region time of 0)
};
// bytes: of the batch, as the caller gave them or as they were read back (used only without kn.cuts)
inline MixPlan plan_mixed(const std::vector<MixImage>& img, const MixObject& ob, const uint64_t* seg_first, uint64_t n, uint64_t bytes, const MixKnobs& kn, const MixCalib& cal) {
    MixPlan P;
    const uint32_t ns = (uint32_t)img.size();
    const bool has_mem = ob.n_mem != 0;      // (without a memory automaton nothing is grouped)
    P.table = kn.walk != 2 && ob.table_ok;   // the table engine unless the generated kernels are asked for
    P.cut = plan_cuts(n, has_mem ? bytes : 1, P.table, has_mem ? kn.cuts : nullptr);
    const uint32_t ng = P.n_groups = (uint32_t)P.cut.size() - 1;
    const bool scans = kn.regions && has_mem;
    P.NW = has_mem ? kn.walk_streams[P.table] : 0;
    // One automaton, one group: exactly the single-automaton call (mfa_match_batch: region pass, then the walk, on the caller's stream, with the
    // engine that call would choose) -- the hops to the internal streams and back cost such a batch 0.03-0.06 ms and buy it nothing.  (Cutting a
    // 1.9 GB batch of ONE automaton into two or three groups was measured in round 4, configs[4]: 0.517 ms in one piece, 0.61 / 0.69 / 0.74
    // ms in two / three / four groups: a walk launch is latency-bound, its 0.15 ms are paid per group and hide behind nothing that short.)
    if (ns == 1 && ng == 1 && kn.single_direct) {
        P.direct = true;
        P.n_regions = scans ? 1u : 0u; P.n_walks = has_mem ? 1u : 0u; P.n_dfa_own = has_mem ? 0u : 1u;
        P.no_regions = !has_mem;
        return P;
    }
    P.with_regions = scans;
    if (P.table) P.walks = plan_table_launches(P.cut, seg_first, img, ob.K, ob.total_words, P.NW);
    if (P.walks.size() > MIX_MAX_LAUNCHES) { P.rc = MFA_ERR_UNSUPPORTED; return P; }      // (more runs of equal cell count than the object has launch slots)
    // the memory-less segments: the items of the multi-table launches, and the segments with a launch of their own
    if (ob.n_dfa) P.dfa = plan_dfa_items(seg_first, img, P.table, kn.dfa);
    for (uint32_t i0 = 0; i0 < P.dfa.items.size(); i0 += kDfaMaxItems) P.dfa_multi.emplace_back(i0, std::min<uint32_t>((uint32_t)P.dfa.items.size(), i0 + kDfaMaxItems));
    // their stream: one beyond the walk streams while the object may have one, else the last walk stream (they go first)
    if (!P.dfa.items.empty() || !P.dfa.own.empty()) P.KD = std::min(P.NW, (int)MIX_MAX_STREAMS - 1);
    P.NS = std::max(P.NW, P.KD + 1);
    // which stream walks which segment (per-segment engine): the first call one after the other (timed), then by cost
    P.calibrating = !P.table && !cal.calibrated && has_mem;
    P.where = !P.table && cal.calibrated && cal.ng_last == ng ? assign_streams(P.cut, seg_first, ns, cal.ready, cal.cost, P.NW) : std::vector<int>(ns, 0);
    size_t w = 0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint64_t lo = P.cut[g], hi = P.cut[g + 1];
        uint32_t sa, sb;
        segments_of(seg_first, ns, lo, hi, sa, sb);
        // one region launch per run of memory segments in the group (an object without memory-less automata: the group): the strings of
        // memory-less segments are not scanned.  The table engine's group event is its last region launch's completion signal.
        const size_t r0 = P.regions.size();
        for (uint32_t s = sa; s < sb; s++) {
            MixLaunch L{};                                     // (per-segment engine: the segment's strings in this group)
            L.g = g; L.s0 = s; L.s1 = s + 1; L.k = P.where[s];
            L.a = std::max(seg_first[s], lo); L.b = std::min(seg_first[s + 1], hi);
            if (img[s].memoryless || L.b <= L.a) continue;
            if (P.with_regions && P.regions.size() > r0 && P.regions.back().b == L.a) P.regions.back().b = L.b;
            else if (P.with_regions) P.regions.push_back(MixRegion{g, L.a, L.b, P.table ? 128u : 256u, false});
            if (!P.table) P.walks.push_back(L);
        }
        P.own_event[g] = !P.table || P.regions.size() == r0;
        if (!P.own_event[g]) P.regions.back().signals = true;
        bool waits[MIX_MAX_STREAMS] = {false};
        for (; w < P.walks.size() && P.walks[w].g == g; w++) {
            P.walks[w].slot = (uint32_t)w;
            P.walks[w].waits = !waits[P.walks[w].k];
            waits[P.walks[w].k] = true;
        }
    }
    P.n_regions = (uint32_t)P.regions.size(); P.n_walks = (uint32_t)P.walks.size();
    P.no_regions = P.regions.empty() && ob.n_dfa != 0;
    P.n_dfa_multi = (uint32_t)P.dfa_multi.size(); P.n_dfa_own = (uint32_t)P.dfa.own.size(); P.n_dfa_items = (uint32_t)P.dfa.items.size(); P.dfa_strings = P.dfa.strings;
    return P;
}
}  // namespace mfa

#endif
