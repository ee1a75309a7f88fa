// What a call on ONE memory-less automaton will launch (mfa_match_batch on an NFA image and the three resume calls), decided by pure
// functions: no HIP, no stream, no memory.  kernels.hip, dfa_split.hip, dfa_spec.hip and the nfa_set*.hip files call these and then only
// reserve, record and launch what they say; tests/emul/memless_plan_emul.cpp runs the same functions on a machine without a GPU
// (tests/test_memless_plan_cpu.py).  Figures that a kernel's own header also has are checked against it where both are seen (static_assert).
#ifndef MFA_MEMLESS_PLAN_H
#define MFA_MEMLESS_PLAN_H

#include <cstdint>
#include <cstdlib>

#include "../../include/mfa_hip.h"

namespace mfa {

// ---- grid ----------------------------------------------------------------------------------------------------------------------------
// workgroups of 256 lanes with `lds` bytes of LDS each that a CU keeps resident: what its 160 KiB allow, at most 8 (32 waves), at least 1
inline uint64_t lds_blocks_per_cu(size_t lds) {
    const uint64_t per_cu = (160u * 1024u) / (lds ? lds : 1);
    return per_cu > 8 ? 8 : per_cu < 1 ? 1 : per_cu;
}
// THE grid of a persistent kernel: a block for every per_block units, capped by what the CUs keep resident, at least 1
inline unsigned persistent_grid(uint64_t units, uint64_t per_block, uint64_t n_cus, uint64_t blocks_per_cu) {
    const uint64_t blocks = (units + per_block - 1u) / per_block, cap = n_cus * blocks_per_cu;
    return (unsigned)(blocks > cap ? (cap ? cap : 1u) : blocks ? blocks : 1u);
}

// ---- knobs ---------------------------------------------------------------------------------------------------------------------------
struct EnvU64 { bool set; uint64_t v; };
inline EnvU64 env_opt(const char* name) {
    const char* e = getenv(name);
    if (!e || !*e) return EnvU64{false, 0};
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return EnvU64{end != e, (uint64_t)v};
}
inline uint64_t env_u64(const char* name, uint64_t dflt) { const EnvU64 e = env_opt(name); return e.set ? e.v : dflt; }
inline char env_char(const char* name) { const char* e = getenv(name); return e ? e[0] : 0; }      // its first character; 0: not set

// what runs behind a main kernel for the strings it queued; the index of everything a family of engines shares
enum SplitTail : uint32_t {
    TAIL_FOLD = 0,       // dfa_split.hip: a map per chunk, folded.  Raises split_ran.
    TAIL_SPEC = 1,       // dfa_spec.hip: guess, repair, resolve on one state.  MFA_DFA_SPEC*.  Raises split_ran and spec_ran.
    TAIL_SET = 2,        // nfa_set_split.hip, nfa_set_wave_split.hip: the same on a node set.  MFA_SET_SPLIT*.  Raises set_split_ran.
    TAIL_KINDS = 3,
};

// every variable these launches depend on, read once per call (never cached: tests set them between calls of one process)
struct MemlessKnobs {
    char     split;                  // MFA_DFA_SPLIT: '0' off, '2' always with the tail (measurements); 0: not set
    char     kernel;                 // MFA_DFA_KERNEL: 's' the untiled walk, 'p' the SGPR-packed form; 0: not set
    uint64_t split_min;              // MFA_DFA_SPLIT_MIN, at least 1
    EnvU64   chunk, arena;           // MFA_DFA_CHUNK, MFA_DFA_ARENA (tests shrink it to see the chunk size grow)
    bool     off[TAIL_KINDS];        // MFA_DFA_SPEC=0, MFA_SET_SPLIT=0
    EnvU64   rounds[TAIL_KINDS], lookback[TAIL_KINDS];
};
static constexpr uint64_t kSplitMinDefault = 64u * 1024u;   // MFA_DFA_SPLIT_MIN; never below 64 KiB by default
inline MemlessKnobs memless_knobs() {
    MemlessKnobs k{};
    k.split = env_char("MFA_DFA_SPLIT");
    k.kernel = env_char("MFA_DFA_KERNEL");
    k.split_min = env_u64("MFA_DFA_SPLIT_MIN", kSplitMinDefault);
    if (k.split_min == 0) k.split_min = 1;
    k.chunk = env_opt("MFA_DFA_CHUNK");
    k.arena = env_opt("MFA_DFA_ARENA");
    k.off[TAIL_SPEC] = env_char("MFA_DFA_SPEC") == '0'; k.rounds[TAIL_SPEC] = env_opt("MFA_DFA_SPEC_ROUNDS"); k.lookback[TAIL_SPEC] = env_opt("MFA_DFA_SPEC_LOOKBACK");
    k.off[TAIL_SET] = env_char("MFA_SET_SPLIT") == '0'; k.rounds[TAIL_SET] = env_opt("MFA_SET_SPLIT_ROUNDS"); k.lookback[TAIL_SET] = env_opt("MFA_SET_SPLIT_LOOKBACK");
    return k;
}

// ---- split schemes -------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kSplitQueueCap = 16384;           // long strings per call; the ones beyond are walked by the main kernel
static constexpr uint32_t kSplitArenaChunks = 131072;       // the chunk size grows so that the chunks stay near this count
static constexpr uint32_t kSplitQuietCalls = 4;             // launches in a row without a long string before the tail is left out
static constexpr uint32_t kSplitChunkMin = 4096;            // MFA_DFA_CHUNK of the tabulated engines; DESIGN.md section 4.5 has the sweep
static constexpr uint32_t kSplitEntryBytes = 24;            // sizeof(SplitEntry) (dfa_split.h)
static constexpr uint32_t kSplitRoundsMax = 8;              // kSpecRoundsMax (dfa_spec_core.h)

// One engine's way of cutting its long strings, as data.  The workspace is header[256 bytes], queue[kSplitQueueCap], arena[map_cap * per_chunk].
struct SplitScheme {
    SplitTail tail;
    uint32_t  per_chunk;             // bytes of arena per chunk; 0: this image has no split path
    bool      start_quiet;           // no tail until the workspace has met a long string once (a table in L2: its tail is seven launches)
    bool      never_quiet;           // the tail from the first call on, whatever the pinned word says (one long string walked whole costs seconds)
    uint32_t  chunk_min, arena_cap;  // MFA_DFA_CHUNK where it is not set; the most chunks of arena records are reserved for
    uint32_t  rounds, lookback;      // defaults of the tail's two knobs
};
// table in LDS, 2 to 127 state sets: a map of 1 << lanes_log2 bytes per chunk; quiet after kSplitQuietCalls calls without a long string
inline SplitScheme split_scheme_lds(uint32_t lanes_log2) { return SplitScheme{TAIL_FOLD, 1u << lanes_log2, false, false, kSplitChunkMin, kSplitArenaChunks, 0, 0}; }
static constexpr SplitScheme kSplitSchemeNone = {TAIL_FOLD, 0, false, false, 0, 0, 0, 0};                                // (a table of 128 to 254 state sets)
static constexpr SplitScheme kSplitSchemeL2 = {TAIL_SPEC, 12, true, false, kSplitChunkMin, kSplitArenaChunks, 3, 256};   // start_used, end[2]: three words
static constexpr SplitScheme kSplitSchemeSet = {TAIL_SET, 144, false, true, 256, kSplitArenaChunks, 3, 64};              // ... three records of three quarters
static constexpr SplitScheme kSplitSchemeWave = {TAIL_SET, 816, false, true, 1024, 32768, 3, 64};                        // ... three records of 68 words

// the workspace as a call finds it: the pinned word (1: the last tail met no long string, 2: it met one, 3: a launch without tail met one)
struct SplitWorkspace { bool has_word; uint32_t seen; bool keep; uint32_t quiet; };

struct SplitPlan {
    uint64_t split_min;              // 0: the path is off, the main kernel walks every string as it always has
    bool     tail;                   // false: the main kernel alone (it walks long strings too, and reports them to the pinned word)
    uint32_t chunk_min, arena_chunks, map_cap, rounds, lookback;
    size_t   queue_at, arena_at, bytes;
    bool     keep;                   // the workspace's two words after this call
    uint32_t quiet;
};

// (n < 2^31: the queue counter is a 32-bit word that every long string increments, also when the queue is full; it must not wrap)
inline bool split_on(const SplitScheme& sc, const MemlessKnobs& kn, uint64_t n) { return sc.per_chunk != 0 && !kn.off[sc.tail] && kn.split != '0' && n < 0x80000000ull; }

// room for this many maps: dfa_split_core.h, split_map_capacity
inline uint64_t split_arena_maps(uint64_t arena_chunks, uint64_t queue_cap) { return arena_chunks + arena_chunks / 16u + 2u * queue_cap + 2u; }

// Leaving the tail out.  Memset, plan, chunk and fold cost a stream of 1 KiB strings a few microseconds per call (DESIGN.md section 4.5
// has the figure), so a workspace whose last kSplitQuietCalls launches all reported "no long string" (the plan kernel writes 1) launches
// the main kernel alone.  That kernel walks whatever it meets, and if it meets a long string it writes 3.  A workspace that has read a 3
// once keeps the tail for good: what the hint can cost is ONE long string walked whole per workspace, never one per batch.
inline SplitPlan plan_split(const SplitScheme& sc, const MemlessKnobs& kn, uint64_t n, const SplitWorkspace& ws) {
    SplitPlan p{};
    p.keep = ws.keep; p.quiet = ws.quiet;
    if (!split_on(sc, kn, n)) return p;
    p.split_min = kn.split_min;
    const uint64_t rounds = kn.rounds[sc.tail].set ? kn.rounds[sc.tail].v : sc.rounds, lookback = kn.lookback[sc.tail].set ? kn.lookback[sc.tail].v : sc.lookback;
    p.rounds = (uint32_t)(rounds > kSplitRoundsMax ? kSplitRoundsMax : rounds);
    p.lookback = (uint32_t)(lookback > MFA_MAX_STRING_BYTES ? MFA_MAX_STRING_BYTES : lookback);
    if (sc.never_quiet) p.keep = true;
    if (ws.has_word) {
        if (ws.seen == 3u) p.keep = true;
        p.quiet = ws.seen == 1u ? ws.quiet + 1u : 0u;
        if (!p.keep && (sc.start_quiet || p.quiet >= kSplitQuietCalls) && kn.split != '2') return p;
    }
    p.tail = true;
    uint64_t chunk_min = ((kn.chunk.set ? kn.chunk.v : sc.chunk_min) + 15u) & ~(uint64_t)15;
    if (chunk_min < 16u) chunk_min = 16u;
    if (chunk_min > (1u << 30)) chunk_min = 1u << 30;
    uint64_t arena = kn.arena.set ? kn.arena.v : sc.arena_cap;
    if (arena < 1u) arena = 1u;
    if (arena > sc.arena_cap) arena = sc.arena_cap;
    p.chunk_min = (uint32_t)chunk_min;
    p.arena_chunks = (uint32_t)arena;
    p.map_cap = (uint32_t)split_arena_maps(arena, kSplitQueueCap);
    p.queue_at = 256;
    p.arena_at = p.queue_at + (size_t)kSplitQueueCap * kSplitEntryBytes;
    p.bytes = p.arena_at + (size_t)p.map_cap * sc.per_chunk;
    return p;
}

// ---- engine --------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kMemlessRow = 258;                      // kDfaRow (dfa_split_core.h)
static constexpr size_t kMemlessTileBytes = 4 * 64 * (128 + 16);  // the input tile of dfa_tiled_kernel (kernels.hip)
static constexpr size_t kSetLdsMax = 64u * 1024u;

// the LDS of a set engine's block: the stacks (lanes: `depth` slots of 256 words; waves: four stacks of `depth` words) and, when both fit
// kSetLdsMax, the tables behind them
struct SetLds { uint32_t words, stack_words, in_lds; size_t bytes; };
inline SetLds set_lds(uint32_t table_words, uint32_t depth, bool wave) {
    SetLds l;
    l.words = table_words; l.stack_words = depth * (wave ? 4u : 256u);
    l.in_lds = ((size_t)l.stack_words + l.words) * 4u <= kSetLdsMax ? 1u : 0u;
    l.bytes = ((size_t)l.stack_words + (l.in_lds ? l.words : 0u)) * 4u;
    return l;
}

// (ENGINE_PACKED: asked for, MFA_DFA_KERNEL=packed, and eligible by size; kernels.hip looks at the byte classes and may still say tiled)
enum MemlessEngine : uint32_t { ENGINE_UNSUPPORTED = 0, ENGINE_PACKED, ENGINE_TILED, ENGINE_UNTILED, ENGINE_L2, ENGINE_SET_LANE, ENGINE_SET_WAVE };
struct MemlessImage { uint32_t states, classes; bool set_walk, set_wave; uint32_t set_words, set_depth; };
struct EnginePlan { MemlessEngine engine; size_t lds; uint64_t per_cu; unsigned grid; };

// Which kernel walks the batch, with how much dynamic LDS, on how many blocks.  Tables: in L2 beyond 16-bit pre-multiplied states, else fused
// in LDS, there tiled (table + tile <= 64 KiB), SGPR-packed, or untiled; 128 to 254 state sets (a table of 64 to 128 KiB) are walked by
// the resume call alone, one or two workgroups per CU.  The packed form has no resume instantiation.
inline EnginePlan plan_memless_engine(const MemlessImage& im, bool resume, const MemlessKnobs& kn, uint64_t n, uint64_t n_cus) {
    EnginePlan p{ENGINE_UNSUPPORTED, 0, 0, 0};
    uint64_t per_block = 256;
    const size_t table = (size_t)im.states * kMemlessRow * 2u;
    if (im.set_walk) {
        p.engine = im.set_wave ? ENGINE_SET_WAVE : ENGINE_SET_LANE;
        p.lds = set_lds(im.set_words, im.set_depth, im.set_wave).bytes;
        if (im.set_wave) per_block = 4;                                 // a string per wave
    } else if ((size_t)im.states * kMemlessRow > 0xffffu) {
        p.engine = ENGINE_L2;
    } else if (kn.kernel != 's' && table + kMemlessTileBytes <= 64 * 1024) {
        const bool packed = !resume && kn.kernel == 'p' && im.states <= 8 && im.classes <= 8 && im.classes >= 1;
        p.engine = packed ? ENGINE_PACKED : ENGINE_TILED;
        p.lds = packed ? kMemlessTileBytes : table + kMemlessTileBytes;
    } else if (resume || table <= 64 * 1024) {
        p.engine = ENGINE_UNTILED;
        p.lds = table;
    } else return p;
    p.per_cu = lds_blocks_per_cu(p.lds);
    p.grid = persistent_grid(n, per_block, n_cus, p.per_cu);
    return p;
}

}  // namespace mfa

#endif
