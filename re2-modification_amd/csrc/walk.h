// Launch interface of the live-list walk kernel (walk.hip, one object per cell count K), and the ONE description of how a wave's memory is
// laid out (WalkLayout): the kernels carve their LDS and their spill area by it, the planner (walk_plan.h) sizes launches and allocations
// by it, the host emulation (tests/emul) its buffers.  Free of HIP: host tools include it as it is.
#ifndef MFA_WALK_H
#define MFA_WALK_H

#include <cstddef>
#include <cstdint>

#ifndef WALK_MIN_WAVES
#define WALK_MIN_WAVES 2      /* __launch_bounds__: waves per SIMD the register allocation leaves room for */
#endif

namespace mfa {

constexpr uint32_t WALK_MAX_SEG = 16;      // automata per launch
constexpr uint32_t WALK_LDS_BYTES = 160u * 1024u;      // LDS of a CU: the most one workgroup can have
constexpr uint32_t CMP_CACHE = 4;          // answered comparisons a lane can hold for one step (beyond them it compares by itself: walk_core.h)
#define MFA_RT_CACHED 2u          /* entries kept in LDS beside the header */      // (device_common.h's definition, token for token: a host tool does not include that file)

constexpr uint32_t walk_W(uint32_t K) { return 2u + 2u * K; }             // value words per list entry
constexpr uint32_t walk_DW(uint32_t K) { return (1u + 2u * K + 1u) / 2u; }  // direction words per entry: int16 each (pos, then S, L per cell)

// One wave's block of LDS and its block of the spill area, as word offsets from the block's start (the pieces are walk_core.h's Store).
// `lean`: the lean walk keeps list values only.  Every piece is [..][lanes] with the lane innermost.
struct WalkLayout {
    uint32_t K, C, CX;        // cells; list entries in LDS; list entries beyond them, in the spill area
    bool images_global;       // the two probe images of a lane live in the spill area
    bool lean;
    uint32_t nm_words;        // long-list kernel: words of a lane's node map, else 0
    uint32_t lanes = 64u;     // (1: the host emulation)
    constexpr uint32_t W() const { return walk_W(K); }
    constexpr uint32_t DW() const { return lean ? 0u : walk_DW(K); }
    constexpr uint32_t CI() const { return images_global || lean ? 0u : C; }      // image entries in LDS ...
    constexpr uint32_t XI() const { return lean ? 0u : CX + C - CI(); }           // ... and in the spill area
    // LDS: [lv 2 C W][ld 2 C DW][sb CI W][sa CI DW][rtc 2 MFA_RT_CACHED][nm nm_words]
    constexpr uint32_t lv() const { return 0u; }
    constexpr uint32_t ld() const { return lv() + 2u * C * W() * lanes; }
    constexpr uint32_t sb() const { return ld() + 2u * C * DW() * lanes; }
    constexpr uint32_t sa() const { return sb() + CI() * W() * lanes; }
    constexpr uint32_t rtc() const { return sa() + CI() * DW() * lanes; }
    constexpr uint32_t nm() const { return rtc() + (lean ? 0u : 2u * lanes * MFA_RT_CACHED); }
    constexpr uint32_t lds_words() const { return nm() + nm_words * lanes; }
    // spill area: [gv 2 CX W][gd 2 CX DW][gsb XI W][gsa XI DW][gq CMP_CACHE 4]
    constexpr uint32_t gv() const { return 0u; }
    constexpr uint32_t gd() const { return gv() + 2u * CX * W() * lanes; }
    constexpr uint32_t gsb() const { return gd() + 2u * CX * DW() * lanes; }
    constexpr uint32_t gsa() const { return gsb() + XI() * W() * lanes; }
    constexpr uint32_t gq() const { return gsa() + XI() * DW() * lanes; }
    constexpr uint32_t spill_used() const { return gq() + CMP_CACHE * 4u * lanes; }
    // What a wave's block of the spill area is reserved with, and the stride from one wave's block to the next: room for every entry
    // (also those that are in LDS) in both lists and both images.  It decides grids and allocations; spill_used() <= spill_words().
    constexpr size_t spill_words() const { return (size_t)(CX + C) * lanes * (lean ? 2u * W() : 3u * W() + 3u * DW()) + CMP_CACHE * 4u * lanes; }
};
// bytes of LDS of a workgroup of four waves behind `shared_words` of tables
constexpr size_t walk_lds_bytes(uint32_t shared_words, const WalkLayout& l) { return ((size_t)shared_words + 4u * (size_t)l.lds_words()) * sizeof(uint32_t); }

struct WalkArgs {                     // kernel parameters; every pointer is a device pointer
    const uint8_t*  bytes;
    const uint64_t* offsets;
    uint64_t        n;
    uint8_t*        results;
    const uint64_t* regions;          // region table of the batch, or nullptr
    const uint32_t* tables;           // table blocks of the launch's automata, back to back (walk_tables.h)
    uint32_t*       spill;            // per wave: list entries and probe images beyond the LDS capacity
    unsigned long long* counter;      // ticket counter, zeroed before the launch
    uint32_t table_words, shared_words;      // LDS words: the tables, and the tables rounded up to a multiple of 64
    uint32_t n_seg, C, CX, accel, refill;
    uint32_t images_global;           // the two probe images of a lane live in global memory (less LDS per wave: more waves per CU)
    uint32_t nm_words;                // long-list kernel (WALK_NODE_MAP): words of a lane's node map = (nodes of the launch's largest automaton + 3) / 4, else 0
    uint32_t* lean_queue;             // strings without a periodic stretch are handed to walk_lean_kernel through this queue (nullptr: all are walked here);
                                      //   its length is counter[1] (as 32 bits), the lean kernel's ticket counter counter[2]
    uint32_t* lean_seen;              // pinned host word (or nullptr): the lean kernel stores the queue's length + 1 there (mfa_internal.h: LeanHint)
    uint32_t seg_first[WALK_MAX_SEG + 1];    // segment s = strings seg_first[s] .. seg_first[s+1]-1 of this launch ...
    uint32_t seg_table[WALK_MAX_SEG];        // ... walks the automaton whose table block starts at this word of `tables`
};

constexpr uint32_t WALK_MAX_K = 9;         // walk_k1 .. walk_k9 are built
enum class WalkKernel { plain, long_k1, stats };      // walk_k<K>; K = 1 with the node map (long lists); K = 1 with counters (MFA_WALK_STATS=1; development)

struct WalkLaunch {                   // a planned launch (walk_plan.h: plan_walk); walk.hip launches what it says
    WalkArgs args;
    uint32_t K;                       // cells of the launch's largest automaton: which walk_k<K>
    WalkKernel kernel;
    unsigned grid;                    // workgroups of 256 threads
    size_t   lds_bytes;               // dynamic LDS of a workgroup
    unsigned lean_grid;               // workgroups of the lean kernel that follows (0: none)
    uint32_t lean_C, lean_CX;         // its list capacity in LDS and beyond
    size_t   lean_lds_bytes;
    size_t   spill_bytes, queue_at;   // bytes of the spill buffer (the waves' blocks of either kernel, then the lean queue), and where the queue starts
    uint32_t counter_words;           // 64-bit words to clear in front of the launch
    bool     reversed;
    bool     tables_global;           // the tables do not fit LDS: the kernel reads them from global memory (shared_words = 0)
};

constexpr bool walk_has_kernel(const WalkLaunch& L) { return L.kernel != WalkKernel::plain || (L.K >= 1u && L.K <= WALK_MAX_K); }

#define MFA_WALK_DECL(K) int launch_walk_k##K(const WalkLaunch& L, void* stream);
MFA_WALK_DECL(1) MFA_WALK_DECL(2) MFA_WALK_DECL(3) MFA_WALK_DECL(4) MFA_WALK_DECL(5) MFA_WALK_DECL(6) MFA_WALK_DECL(7) MFA_WALK_DECL(8) MFA_WALK_DECL(9)
#undef MFA_WALK_DECL
int launch_walk_long_k1(const WalkLaunch& L, void* stream);   // K = 1, automata of 17-128 nodes whose lists are long (77-node ex. 8 -bnf / -reverse): a node's entry is found through a per-lane map in LDS (WALK_NODE_MAP)
int launch_walk_stats(const WalkLaunch& L, void* stream);
void walk_print_stats(unsigned long long* d_counter, const char* tag);

}  // namespace mfa

#endif
