// Host side of an automaton image: blob parsing, the structural checks the MFA kernel
// relies on, tabulation of the memory-less step function for the table-walk kernel, and the tables of the set walk
// for automata whose tabulation passes the limit.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>

#include "mfa_internal.h"
#include "nfa_set_core.h"
#include "nfa_set_wave_core.h"

namespace mfa {

int parse_blob(const void* blob, size_t n_bytes, HostImage& out) {
    if (!blob || n_bytes < sizeof(mfa_blob_header)) return MFA_ERR_BAD_BLOB;
    mfa_blob_header h;
    std::memcpy(&h, blob, sizeof h);
    if (h.magic != MFA_BLOB_MAGIC || h.version != MFA_BLOB_VERSION) return MFA_ERR_BAD_BLOB;
    if (h.kind > MFA_KIND_MFA || h.n_nodes == 0 || h.n_nodes > 0xffffu) return MFA_ERR_BAD_BLOB;
    if (h.start >= h.n_nodes || h.finish >= h.n_nodes || h.n_cells > MFA_MAX_CELLS) return MFA_ERR_BAD_BLOB;
    size_t need = sizeof h + (size_t)(h.n_nodes + 1) * 4 + (size_t)h.n_edges * sizeof(mfa_blob_edge);
    if (n_bytes < need) return MFA_ERR_BAD_BLOB;
    out.h = h;
    out.edge_begin.resize(h.n_nodes + 1);
    out.edges.resize(h.n_edges);
    const char* p = (const char*)blob + sizeof h;
    std::memcpy(out.edge_begin.data(), p, (size_t)(h.n_nodes + 1) * 4);
    p += (size_t)(h.n_nodes + 1) * 4;
    if (h.n_edges) std::memcpy(out.edges.data(), p, (size_t)h.n_edges * sizeof(mfa_blob_edge));
    if (out.edge_begin[0] != 0 || out.edge_begin[h.n_nodes] != h.n_edges) return MFA_ERR_BAD_BLOB;
    for (uint32_t k = 0; k < h.n_nodes; k++)
        if (out.edge_begin[k] > out.edge_begin[k + 1]) return MFA_ERR_BAD_BLOB;
    for (const auto& e : out.edges) {
        if (e.target >= h.n_nodes) return MFA_ERR_BAD_BLOB;
        for (unsigned c = h.n_cells + 1; c <= MFA_MAX_CELLS; c++)
            if (MFA_EDGE_ACTION(e, c)) return MFA_ERR_BAD_BLOB;
        if (MFA_EDGE_ACTION(e, 0u)) return MFA_ERR_BAD_BLOB;
        for (unsigned c = 1; c <= MFA_MAX_CELLS; c++)
            if (MFA_EDGE_ACTION(e, c) == 3u) return MFA_ERR_BAD_BLOB;
        if (!(e.flags & MFA_EDGE_EPS) && e.label >= '1' && e.label <= '9' && (uint32_t)(e.label - '0') > h.n_cells &&
            h.kind == MFA_KIND_MFA)
            return MFA_ERR_BAD_BLOB;
    }
    return MFA_OK;
}

// What bt/bt_mfa.cpp guarantees for every automaton it builds (SURVEY.md section 8a,
// "Structural invariants") and what the MFA kernel is written against:
//   * every epsilon edge targets `finish`, and nothing but epsilon edges does
//     (so states at `finish` only ever exist with pos == len: an accept flag);
//   * `finish` has no out-edges.
// An image that breaks them is refused (there is no CPU fallback behind this library).
int check_mfa_invariants(const HostImage& img) {
    const auto& h = img.h;
    if (h.n_nodes > MFA_MAX_NODES || h.n_cells > MFA_MAX_KERNEL_CELLS) return MFA_ERR_UNSUPPORTED;
    if (img.edge_begin[h.finish + 1] != img.edge_begin[h.finish]) return MFA_ERR_UNSUPPORTED;
    for (uint32_t n = 0; n < h.n_nodes; n++) {
        for (uint32_t e = img.edge_begin[n]; e < img.edge_begin[n + 1]; e++) {
            bool eps = img.edges[e].flags & MFA_EDGE_EPS;
            bool to_finish = img.edges[e].target == h.finish;
            if (eps != to_finish) return MFA_ERR_UNSUPPORTED;
        }
    }
    return MFA_OK;
}

// ---- memory-less automata: tabulate Automata::evaluateStates ---------------------------------
//
// automata.cpp:119-128 maps (state set, letter) -> state set and depends on nothing else
// (letter_index is unused), so it can be tabulated once per automaton.  The tabulation runs
// the reference's own step -- including its quirks: nodes are visited in pointer (= node
// number) order, an edge whose target is already in `visited` is skipped even when it is a
// letter edge (automata.cpp:105-107), and a node is marked visited only after its edges were
// walked (automata.cpp:116).
namespace {

struct Stepper {
    const HostImage& g;
    std::vector<uint8_t> nxt, vis;
    explicit Stepper(const HostImage& img) : g(img), nxt(img.h.n_nodes), vis(img.h.n_nodes) {}

    void eval_state(uint32_t node, int letter) {           // automata.cpp:98-117; letter < 0: the final pass's ""
        if (letter < 0 && node == g.h.finish) {
            nxt[node] = 1;
        } else {
            for (uint32_t e = g.edge_begin[node]; e < g.edge_begin[node + 1]; e++) {
                const mfa_blob_edge& ed = g.edges[e];
                if (vis[ed.target]) continue;
                if (ed.flags & MFA_EDGE_EPS) eval_state(ed.target, letter);
                else if (letter >= 0 && (ed.label == '.' || ed.label == (uint8_t)letter)) nxt[ed.target] = 1;
            }
        }
        vis[node] = 1;
    }

    std::vector<uint8_t> step(const std::vector<uint8_t>& cur, int letter) {   // automata.cpp:119-128
        std::fill(nxt.begin(), nxt.end(), 0);
        std::fill(vis.begin(), vis.end(), 0);
        for (uint32_t v = 0; v < g.h.n_nodes; v++)
            if (cur[v] && !vis[v]) eval_state(v, letter);
        return nxt;
    }
};

}  // namespace

// byte classes: one per distinct literal label, one for every other byte ('.' edges match all); rep: a representative byte per class
static int nfa_byte_classes(HostImage& img, std::vector<int>& rep) {
    int cls_of[256];
    for (int b = 0; b < 256; b++) cls_of[b] = -1;
    rep.clear();
    int other_rep = -1;
    for (const auto& e : img.edges)
        if (!(e.flags & MFA_EDGE_EPS) && e.label != '.' && cls_of[e.label] < 0) {
            cls_of[e.label] = (int)rep.size();
            rep.push_back(e.label);
        }
    for (int b = 0; b < 256; b++)
        if (cls_of[b] < 0 && b != '.') { other_rep = b; break; }
    int other_cls = (int)rep.size();
    rep.push_back(other_rep < 0 ? 0 : other_rep);
    for (int b = 0; b < 256; b++) img.byte_class[b] = (uint8_t)(cls_of[b] >= 0 ? cls_of[b] : other_cls);
    // a '.' byte in the input only matches '.' labels, like any other unlabelled byte -- unless some edge carries the literal label '.',
    // which the reference treats as the wildcard (automata.cpp:111)
    img.n_classes = (uint32_t)rep.size();
    return img.n_classes > 255 ? MFA_ERR_UNSUPPORTED : MFA_OK;
}

// The epsilon edges among the nodes that can be reached from `start`: MFA_ERR_UNSUPPORTED if they close a cycle (the reference's
// evaluateState marks a node after its scan, so it would recurse for ever, and so would Stepper); else *chain = the most nodes on one
// path of epsilon edges (1 when there is none).
int nfa_eps_chain(const HostImage& img, uint32_t* chain, std::vector<uint8_t>* reached) {
    const uint32_t n = img.h.n_nodes;
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> todo{img.h.start};
    seen[img.h.start] = 1;
    while (!todo.empty()) {
        const uint32_t u = todo.back(); todo.pop_back();
        for (uint32_t e = img.edge_begin[u]; e < img.edge_begin[u + 1]; e++)
            if (!seen[img.edges[e].target]) { seen[img.edges[e].target] = 1; todo.push_back(img.edges[e].target); }
    }
    // depth-first over epsilon edges with an explicit stack: colour 1 = on the path, 2 = done (len = nodes on its longest path down)
    std::vector<uint8_t> colour(n, 0);
    std::vector<uint32_t> len(n, 1), at(n, 0), path;
    uint32_t longest = 1;
    for (uint32_t r = 0; r < n; r++) {
        if (!seen[r] || colour[r]) continue;
        path.assign(1, r); colour[r] = 1; at[r] = img.edge_begin[r];
        while (!path.empty()) {
            const uint32_t u = path.back();
            if (at[u] < img.edge_begin[u + 1]) {
                const mfa_blob_edge& ed = img.edges[at[u]++];
                if (!(ed.flags & MFA_EDGE_EPS)) continue;
                if (colour[ed.target] == 1) return MFA_ERR_UNSUPPORTED;
                if (colour[ed.target] == 2) { len[u] = std::max(len[u], len[ed.target] + 1u); continue; }
                colour[ed.target] = 1; at[ed.target] = img.edge_begin[ed.target]; path.push_back(ed.target);
            } else {
                colour[u] = 2; path.pop_back();
                longest = std::max(longest, len[u]);
                if (!path.empty()) len[path.back()] = std::max(len[path.back()], len[u] + 1u);
            }
        }
    }
    if (chain) *chain = longest;
    if (reached) *reached = seen;
    return MFA_OK;
}

// The tables of the set walk (nfa_set_core.h has the layout and the rule).  MFA_ERR_UNSUPPORTED: more nodes, classes, items or a
// longer epsilon chain than the kernel holds, or a cycle of epsilon edges.
// wave: the tables of the wave-cooperative walk instead (nfa_set_wave_core.h): the same header and sections, a mask row of W =
// ceil(n / 32) words for up to kWaveMaxNodes nodes, 11 bits of node number in an epsilon item, a stack of up to n slots (the chain is
// never longer), items held to 2^kWavePosBits; the home set is the wide one (nfa_set_home_wide: 64 words, for nfa_set_wave_split.hip).
static int set_tables_build(HostImage& img, bool wave) {
    const uint32_t n = img.h.n_nodes;
    std::vector<int> rep;
    int rc = nfa_byte_classes(img, rep);
    if (rc != MFA_OK) return rc;
    uint32_t chain = 1;
    std::vector<uint8_t> reached;
    rc = nfa_eps_chain(img, &chain, &reached);
    if (rc != MFA_OK) return rc;
    if (wave ? n > kWaveMaxNodes || chain - 1u > n : n > kSetMaxNodes || chain - 1u > kSetMaxDepth) return MFA_ERR_UNSUPPORTED;
    const uint32_t W = wave ? wave_words_of(n) : n <= 32 ? 1u : n <= 64 ? 2u : n <= 128 ? 4u : 8u, C = img.n_classes;
    std::vector<uint32_t> item_begin(n + 1, 0), items, masks;
    uint32_t runs = 0;
    for (uint32_t u = 0; u < n; u++) {
        item_begin[u] = (uint32_t)items.size();
        bool in_run = false;
        for (uint32_t e = img.edge_begin[u]; reached[u] && e < img.edge_begin[u + 1]; e++) {
            const mfa_blob_edge& ed = img.edges[e];
            if (ed.flags & MFA_EDGE_EPS) { items.push_back(kSetItemEps | ed.target); in_run = false; continue; }
            if (!in_run) { items.push_back(runs++); masks.resize((size_t)runs * C * W, 0u); in_run = true; }
            for (uint32_t c = 0; c < C; c++)
                if (ed.label == '.' || ed.label == (uint8_t)rep[c]) masks[((size_t)(runs - 1u) * C + c) * W + (ed.target >> 5)] |= 1u << (ed.target & 31u);
        }
    }
    item_begin[n] = (uint32_t)items.size();
    if (items.size() >= (1u << (wave ? kWavePosBits : kSetPosBits)) || masks.size() >= (1u << 26)) return MFA_ERR_UNSUPPORTED;
    // accept: the nodes from which `finish` is reached over epsilon edges alone (finish itself among them)
    std::vector<uint32_t> accept(W, 0u);
    for (uint32_t u = 0; u < n; u++) {
        std::vector<uint8_t> seen(n, 0);
        std::vector<uint32_t> todo{u};
        seen[u] = 1;
        bool hit = false;
        while (!todo.empty() && !hit) {
            const uint32_t v = todo.back(); todo.pop_back();
            if (v == img.h.finish) { hit = true; break; }
            for (uint32_t e = img.edge_begin[v]; e < img.edge_begin[v + 1]; e++)
                if ((img.edges[e].flags & MFA_EDGE_EPS) && !seen[img.edges[e].target]) { seen[img.edges[e].target] = 1; todo.push_back(img.edges[e].target); }
        }
        if (hit) accept[u >> 5] |= 1u << (u & 31u);
    }
    std::vector<uint32_t>& out = img.set_tables;
    out.assign(SET_H_SIZE, 0u);
    out[SET_H_NODES] = n; out[SET_H_WORDS] = W; out[SET_H_CLASSES] = C; out[SET_H_DEPTH] = chain - 1u;
    out[SET_H_START] = img.h.start; out[SET_H_REVERSED] = img.h.is_reversed ? 1u : 0u;
    out[SET_H_ITEM_BEGIN] = (uint32_t)out.size(); out.insert(out.end(), item_begin.begin(), item_begin.end());
    out[SET_H_ITEMS] = (uint32_t)out.size();      out.insert(out.end(), items.begin(), items.end());
    out[SET_H_MASKS] = (uint32_t)out.size();      out.insert(out.end(), masks.begin(), masks.end());
    out[SET_H_ACCEPT] = (uint32_t)out.size();     out.insert(out.end(), accept.begin(), accept.end());
    out[SET_H_BYTE_CLASS] = (uint32_t)out.size(); out.resize(out.size() + 64u, 0u);
    std::memcpy(out.data() + out[SET_H_BYTE_CLASS], img.byte_class, 256);
    out[SET_H_TOTAL] = (uint32_t)out.size();
    img.set_walk = true;
    img.set_wave = wave;
    img.dfa_states = 0; img.dfa_trans.clear(); img.dfa_accept.clear();
    if (wave) nfa_set_home_wide(img, img.set_home_wide);
    else nfa_set_home(img, img.set_home);
    return MFA_OK;
}

int nfa_set_build(HostImage& img) { return set_tables_build(img, false); }
int nfa_set_wave_build(HostImage& img) { return set_tables_build(img, true); }

// The second seed of nfa_set_split.hip's guesses (nfa_set_split_core.h), for texts on which a walk from {start} dies in mid-text: what
// spec_home_state (dfa_spec_core.h) is for a table, on node sets.  The set a deterministic pseudo-random walk from {start} ends in:
// every step draws a byte class (xorshift32, the seed of spec_home_state) and takes the first class from there on, cyclically, whose
// step (Stepper: the norm) does not lead to the empty set; a set with no such class ends the walk.  4096 steps.  Never empty.
// img.byte_class and img.n_classes are nfa_byte_classes' (nfa_set_build has called it).
static std::vector<uint8_t> set_home_nodes(const HostImage& img) {
    const uint32_t n = img.h.n_nodes, C = img.n_classes;
    std::vector<int> rep(C, 0);
    for (int b = 255; b >= 0; b--) rep[img.byte_class[b]] = b;       // (any byte of a class steps alike)
    Stepper st(img);
    std::vector<uint8_t> cur(n, 0);
    cur[img.h.start] = 1;
    uint32_t x = 0x9e3779b9u;
    for (uint32_t step = 0; step < 4096u && C != 0u; step++) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        const uint32_t c0 = x % C;
        bool moved = false;
        for (uint32_t k = 0; k < C && !moved; k++) {
            const std::vector<uint8_t> nx = st.step(cur, rep[(c0 + k) % C]);
            if (std::find(nx.begin(), nx.end(), (uint8_t)1) != nx.end()) { cur = nx; moved = true; }
        }
        if (!moved) break;
    }
    return cur;
}

void nfa_set_home(const HostImage& img, uint32_t (&home)[8]) {
    const std::vector<uint8_t> cur = set_home_nodes(img);
    for (uint32_t& w : home) w = 0u;
    for (uint32_t v = 0; v < img.h.n_nodes && v < 256u; v++)
        if (cur[v]) home[v >> 5] |= 1u << (v & 31u);
}

// the same set for a wave image (nfa_set_wave_split_core.h: wave_spec_guess): 64 words, lane l of a wave its word l
void nfa_set_home_wide(const HostImage& img, uint32_t (&home)[64]) {
    const std::vector<uint8_t> cur = set_home_nodes(img);
    for (uint32_t& w : home) w = 0u;
    for (uint32_t v = 0; v < img.h.n_nodes && v < kWaveMaxNodes; v++)
        if (cur[v]) home[v >> 5] |= 1u << (v & 31u);
}

// Which tables an image that is to be walked as a node set gets.  Those of the lane kernel (one string per lane) up to kSetMaxNodes nodes,
// exactly as before the wave kernel existed -- a chain beyond that kernel's stack stays a refusal -- and those of the wave kernel (one
// string per wave) for kSetMaxNodes + 1 to kWaveMaxNodes nodes.  MFA_SET_WAVE=1, read here, once per image: wave tables for every such
// image, the narrow ones too (for measurements and tests; never the default).
static int nfa_set_any_build(HostImage& img) {
    const char* wv = getenv("MFA_SET_WAVE");
    if ((wv && wv[0] == '1') || img.h.n_nodes > kSetMaxNodes) return nfa_set_wave_build(img);
    return nfa_set_build(img);
}

// What mfa_image_create does with a memory-less automaton: tabulate it, and when the state sets pass the limit (MFA_DFA_STATE_LIMIT,
// at most MFA_MAX_DFA_STATES) build the tables of the set walk instead (nfa_set_any_build).  MFA_NFA_SETWALK=1: the set walk without tabulating;
// MFA_NFA_SETWALK=0: no set walk, the refusal of old.  Both are read here, once per image.
int nfa_image_build(HostImage& img) {
    int rc = nfa_eps_chain(img, nullptr, nullptr);
    if (rc != MFA_OK) return rc;
    const char* sw = getenv("MFA_NFA_SETWALK");
    if (sw && sw[0] == '1') return nfa_set_any_build(img);
    uint64_t limit = MFA_MAX_DFA_STATES;
    if (const char* e = getenv("MFA_DFA_STATE_LIMIT")) {
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v >= 2 && v < limit) limit = v;
    }
    rc = tabulate_nfa(img, (uint32_t)limit);
    if (rc != MFA_ERR_UNSUPPORTED || img.n_classes > 255 || (sw && sw[0] == '0')) return rc;
    return nfa_set_any_build(img);
}

int tabulate_nfa(HostImage& img, uint32_t max_states, std::vector<std::string>* sets_out) {
    const uint32_t n = img.h.n_nodes;
    std::vector<int> rep;
    if (nfa_byte_classes(img, rep) != MFA_OK) return MFA_ERR_UNSUPPORTED;

    // state sets as packed bit strings (up to MFA_MAX_DFA_STATES of them: determinisation can be exponential, e.g.
    // (a|b)*a(a|b)^k has 2^(k+1) sets)
    Stepper st(img);
    const size_t key_bytes = (n + 7) / 8;
    auto pack = [&](const std::vector<uint8_t>& set) {
        std::string k(key_bytes, '\0');
        for (uint32_t v = 0; v < n; v++)
            if (set[v]) k[v >> 3] = (char)(k[v >> 3] | (1 << (v & 7)));
        return k;
    };
    auto unpack = [&](const std::string& k, std::vector<uint8_t>& set) {
        for (uint32_t v = 0; v < n; v++) set[v] = (uint8_t)((k[v >> 3] >> (v & 7)) & 1);
    };
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<std::string> sets;
    std::vector<uint8_t> empty(n, 0), start(n, 0), cur(n, 0);
    start[img.h.start] = 1;
    ids[pack(empty)] = 0; sets.push_back(pack(empty));
    if (start != empty) { ids[pack(start)] = 1; sets.push_back(pack(start)); }
    img.dfa_trans.clear();
    for (size_t s = 0; s < sets.size(); s++) {
        unpack(sets[s], cur);
        for (uint32_t c = 0; c < img.n_classes; c++) {
            const std::string t = pack(s == 0 ? empty : st.step(cur, rep[c]));
            auto it = ids.find(t);
            uint32_t id;
            if (it == ids.end()) {
                id = (uint32_t)sets.size();
                if (id >= max_states) { img.dfa_trans.clear(); return MFA_ERR_UNSUPPORTED; }
                ids.emplace(t, id); sets.push_back(t);
            } else id = it->second;
            img.dfa_trans.push_back(id);
        }
    }
    img.dfa_states = (uint32_t)sets.size();
    img.dfa_accept.assign(img.dfa_states, 0);
    for (uint32_t s = 1; s < img.dfa_states; s++) {
        unpack(sets[s], cur);
        std::vector<uint8_t> f = st.step(cur, -1);            // automata.cpp:201-202
        img.dfa_accept[s] = f[img.h.finish];                  // automata.cpp:204-208
    }
    if (sets_out) *sets_out = std::move(sets);                // (tests: state number -> its node set, bit v & 7 of byte v >> 3)
    return MFA_OK;
}

}  // namespace mfa
