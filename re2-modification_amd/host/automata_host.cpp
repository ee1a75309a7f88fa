// Automata / MFA objects of the host mirror: graph bookkeeping the reference does in
// automata.cpp:16-96 and mfa.cpp:11-77, freezing a graph into an automaton image, and match()
// through the C-ABI of libmfa_hip.so.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <thread>

#include "../../include/mfa_hip.h"
#include "diploma_api.h"

namespace {

[[noreturn]] void fail(const char* where, int code) {
    std::string msg = std::string(where) + ": " + mfa_strerror(code);
    if (code == MFA_ERR_HIP) msg += " (hipError " + std::to_string(mfa_last_hip_error()) + ")";
    throw std::runtime_error(msg);
}

void put32(vector<uint8_t>& out, uint32_t v) {
    for (int k = 0; k < 4; k++) out.push_back((uint8_t)(v >> (8 * k)));
}

struct FlatEdge { std::string by; size_t to; const map<string, MemoryAction>* actions; };
struct FlatNode { uint64_t seq; vector<FlatEdge> edges; };

// Serialise per include/mfa_image_format.h.  Nodes are numbered by allocation order (`seq`), the
// stand-in for the pointer order of the reference's state sets.
vector<uint8_t> serialise(uint32_t kind, bool reversed, vector<FlatNode>& nodes, size_t start, size_t finish) {
    vector<size_t> order(nodes.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return nodes[a].seq < nodes[b].seq; });
    vector<uint32_t> rank(nodes.size());
    for (size_t r = 0; r < order.size(); r++) rank[order[r]] = (uint32_t)r;
    vector<uint8_t> edges;
    vector<uint32_t> begin{0};
    uint32_t n_edges = 0, n_cells = 0;
    for (size_t r = 0; r < order.size(); r++) {
        for (const FlatEdge& e : nodes[order[r]].edges) {
            uint8_t label = 0, flags = 0;
            if (e.by.empty() || e.by == "\xce\xb5") flags |= MFA_EDGE_EPS;
            else if (e.by.size() == 1) label = (uint8_t)e.by[0];
            else throw std::runtime_error("automaton has a multi-byte edge label '" + e.by + "': not representable in an image");
            if (!flags && label >= '1' && label <= '9' && kind == MFA_KIND_MFA) n_cells = std::max<uint32_t>(n_cells, label - '0');
            uint32_t actions = 0;
            if (e.actions)
                for (const auto& kv : *e.actions) {
                    if (kv.first.size() != 1 || kv.first[0] < '1' || kv.first[0] > '9')
                        throw std::runtime_error("memory cell name '" + kv.first + "' is not a digit 1..9");
                    uint32_t c = (uint32_t)(kv.first[0] - '0');
                    actions |= (kv.second == open ? MFA_ACT_OPEN : MFA_ACT_CLOSE) << (2 * c);
                    n_cells = std::max(n_cells, c);
                }
            edges.push_back(label); edges.push_back(flags);
            edges.push_back((uint8_t)(rank[e.to] & 0xff)); edges.push_back((uint8_t)(rank[e.to] >> 8));
            put32(edges, actions);
            n_edges++;
        }
        begin.push_back(n_edges);
    }
    vector<uint8_t> out;
    for (uint32_t v : {MFA_BLOB_MAGIC, MFA_BLOB_VERSION, kind, (uint32_t)reversed, (uint32_t)nodes.size(), n_edges,
                       rank[start], rank[finish], n_cells, 0u})
        put32(out, v);
    for (uint32_t v : begin) put32(out, v);
    out.insert(out.end(), edges.begin(), edges.end());
    return out;
}

template <class NodeT, class Index>
size_t index_of(Index& idx, vector<NodeT*>& all, NodeT* n) {
    auto it = idx.find(n);
    if (it != idx.end()) return it->second;
    idx[n] = all.size();
    all.push_back(n);
    return all.size() - 1;
}

}  // namespace

// ---- Automata ---------------------------------------------------------------------------------------

Automata::Automata() {
    start = new Node();
    finish = new Node();
    nodes.push_back(start);
    nodes.push_back(finish);
    last_idx = 0;
}

Automata::~Automata() {
    if (cached_image_) mfa_image_destroy(cached_image_);
}

void Automata::changeFinalState(Node* new_final) {                               // automata.cpp:16-32
    for (Node* n : nodes)
        for (Edge* e : n->edges)
            if (e->to == finish) e->to = new_final;
    auto it = std::find(nodes.begin(), nodes.end(), finish);
    if (it != nodes.end()) nodes.erase(it);
    start->start_for = new_final;
}

bool Automata::isDeterministic() {                                               // automata.cpp:84-96
    set<pair<uint64_t, string>> seen;
    for (Node* n : nodes)
        for (Edge* e : n->edges)
            if (!seen.insert({n->seq, e->by}).second) return false;
    return true;
}

void Automata::makeDOTFile(const string& filename) {                             // automata.cpp:34-66
    string text = "digraph g {\n";
    auto name_of = [&](Node* n) -> const string& {
        if (n->name.empty()) n->name = std::to_string(last_idx++);
        return n->name;
    };
    for (Node* n : nodes) {
        name_of(n);
        for (Edge* e : n->edges) {
            name_of(e->to);
            string by = e->by.empty() ? "\xce\xb5" : (e->by == "." ? "dot" : e->by);
            if (!e->drawn) text += "\t" + n->name + " -> " + e->to->name + " [label=" + by + "]\n";
        }
    }
    text += "}";
    std::ofstream out(filename + ".dot");
    if (out.is_open()) out << text;
}

bool Automata::draw(const string& filename) {
    makeDOTFile(filename);
    return true;
}

vector<uint8_t> Automata::image_blob() const {
    map<Node*, size_t> idx;
    vector<Node*> all;
    for (Node* n : nodes) index_of(idx, all, n);
    index_of(idx, all, start);
    index_of(idx, all, finish);
    for (size_t k = 0; k < all.size(); k++)
        for (Edge* e : all[k]->edges) index_of(idx, all, e->to);
    vector<FlatNode> flat(all.size());
    for (size_t k = 0; k < all.size(); k++) {
        flat[k].seq = all[k]->seq;
        for (Edge* e : all[k]->edges) flat[k].edges.push_back({e->by, idx[e->to], nullptr});
    }
    return serialise(MFA_KIND_NFA, is_reversed, flat, idx[start], idx[finish]);
}

mfa_image* Automata::image_for_match() {
    vector<uint8_t> blob = image_blob();          // the graph's fields are public: re-freeze and compare
    if (!cached_image_ || blob != cached_blob_) {
        if (cached_image_) { mfa_image_destroy(cached_image_); cached_image_ = nullptr; }
        int rc = mfa_image_create(blob.data(), blob.size(), &cached_image_);
        if (rc != MFA_OK) fail("mfa_image_create", rc);
        cached_blob_ = std::move(blob);
    }
    return cached_image_;
}

extern "C" int diploma_partition_by_bytes(const uint64_t* offsets, uint64_t n, uint32_t parts, uint64_t* cuts) {
    if (!offsets || !cuts || parts == 0) return -1;
    const uint64_t total = offsets[n] - offsets[0];
    cuts[0] = 0;
    for (uint32_t r = 1; r < parts; r++) {
        // (128-bit product: a batch may hold more than 2^64 / parts bytes only in theory, but the rule should not depend on that)
        const uint64_t target = offsets[0] + (uint64_t)(((unsigned __int128)total * r) / parts);
        uint64_t k = (uint64_t)(std::lower_bound(offsets, offsets + n + 1, target) - offsets);
        if (k < cuts[r - 1]) k = cuts[r - 1];
        if (k > n) k = n;
        cuts[r] = k;
    }
    cuts[parts] = n;
    return 0;
}

namespace {

constexpr uint64_t kPieceBytes = 8ull << 20;      // pieces of a string beyond the device's per-call limit; a multiple of 16

// Beyond how many bytes a memory-less automaton's string goes in pieces, and the pieces' size: the device's per-call limit and
// kPieceBytes.  DIPLOMA_PIECE_BYTES=n (tests: n a multiple of 16, at least 16; anything else is ignored) makes both n, so that strings
// of a few KiB take the path of those beyond 16 MiB.
struct PieceRule { uint64_t beyond, piece; };
PieceRule piece_rule() {
    if (const char* e = getenv("DIPLOMA_PIECE_BYTES")) {
        char* end = nullptr;
        const unsigned long long n = strtoull(e, &end, 10);
        if (end != e && *end == 0 && n >= 16 && n % 16 == 0) return {n, n};
    }
    return {MFA_MAX_STRING_BYTES, kPieceBytes};
}

// piece r IN SCAN ORDER of the string [b, e) cut every `piece` bytes from the end the scan starts at; empty once the string is used up
void piece_of(uint64_t b, uint64_t e, uint64_t r, bool reversed, uint64_t piece, uint64_t* lo, uint64_t* hi) {
    const uint64_t len = e - b, skip = r * piece < len ? r * piece : len, take = len - skip < piece ? len - skip : piece;
    if (reversed) { *hi = e - skip; *lo = *hi - take; }
    else { *lo = b + skip; *hi = *lo + take; }
}

// the strings `which` of a memory-less automaton's batch, each given to the device in pieces, one round of pieces per call.  What a string's
// state between two pieces is, and so which resume call carries it, is the image's to say (mfa_image_resume_state_bytes): one word of a
// tabulated image, a record of eight node words of a set-walk image of up to 256 nodes, a record of 64 of an image walked one string per wave.
void match_in_pieces(mfa_image* img, bool reversed, const uint8_t* bytes, const uint64_t* offsets, const vector<uint64_t>& which, uint8_t* results, int device) {
    const uint64_t piece = piece_rule().piece;
    uint32_t state_bytes = 0;
    int rc = mfa_image_resume_state_bytes(img, &state_bytes);
    if (rc != MFA_OK) fail("mfa_image_resume_state_bytes", rc);
    if (state_bytes != sizeof(uint32_t) && state_bytes != sizeof(mfa_set_state) && state_bytes != sizeof(mfa_set_state_wide))
        throw std::runtime_error("Automata::match: a string in pieces, and the image carries " + std::to_string(state_bytes) + " bytes from piece to piece: no call for that");
    uint64_t rounds = 1;
    for (uint64_t k : which) rounds = std::max(rounds, (offsets[k + 1] - offsets[k] + piece - 1) / piece);
    vector<uint32_t> states(state_bytes == sizeof(uint32_t) ? which.size() : 0, MFA_DFA_STATE_START);
    vector<mfa_set_state> sets(state_bytes == sizeof(mfa_set_state) ? which.size() : 0, mfa_set_state{});                  // zeroed: MFA_SET_STATE_START
    vector<mfa_set_state_wide> wide(state_bytes == sizeof(mfa_set_state_wide) ? which.size() : 0, mfa_set_state_wide{});
    const char* call = !states.empty() ? "mfa_match_batch_resume_host" : !sets.empty() ? "mfa_match_batch_resume_set_host" : "mfa_match_batch_resume_set_wide_host";
    vector<uint8_t> res(which.size()), stage;
    vector<uint64_t> off(which.size() + 1);
    for (uint64_t r = 0; r < rounds; r++) {
        stage.clear();
        off[0] = 0;
        for (size_t j = 0; j < which.size(); j++) {
            uint64_t lo, hi;
            piece_of(offsets[which[j]], offsets[which[j] + 1], r, reversed, piece, &lo, &hi);
            stage.insert(stage.end(), bytes + lo, bytes + hi);
            off[j + 1] = stage.size();
        }
        stage.resize(stage.size() + 16);
        uint8_t* out = r + 1 == rounds ? res.data() : nullptr;
        rc = !states.empty() ? mfa_match_batch_resume_host(img, stage.data(), off.data(), which.size(), states.data(), out, device)
           : !sets.empty()   ? mfa_match_batch_resume_set_host(img, stage.data(), off.data(), which.size(), sets.data(), out, device)
                             : mfa_match_batch_resume_set_wide_host(img, stage.data(), off.data(), which.size(), wide.data(), out, device);
        if (rc != MFA_OK) fail(call, rc);
    }
    for (size_t j = 0; j < which.size(); j++) results[which[j]] = res[j];
}

}  // namespace

void Automata::match_packed(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results) {
    mfa_image* img = image_for_match();
    mfa_image_info info;
    // (a memory-less image hands its state from call to call -- one word, or for a set-walk image, dfa_states == 0, a record of its node set,
    // narrow or wide -- so its strings may be longer than one call takes; a memory automaton's are refused)
    if (mfa_image_get_info(img, &info) == MFA_OK && info.kind == MFA_KIND_NFA) {
        vector<uint64_t> longs;
        const uint64_t beyond = piece_rule().beyond;
        for (uint64_t k = 0; k < n; k++)
            if (offsets[k + 1] - offsets[k] > beyond) longs.push_back(k);
        if (!longs.empty()) {
            // the runs of shorter strings between them lie back to back in the caller's buffer: each takes the one call it always took
            uint64_t from = 0;
            for (size_t j = 0; j <= longs.size(); j++) {
                const uint64_t to = j < longs.size() ? longs[j] : n;
                if (to > from) match_packed_short(img, bytes, offsets + from, to - from, results + from);
                from = to + 1;
            }
            match_in_pieces(img, info.is_reversed != 0, bytes, offsets, longs, results, device);
            return;
        }
    }
    match_packed_short(img, bytes, offsets, n, results);
}

// text_match.cpp: the text split on the device and matched where it lies
int diploma_match_text_on_device(mfa_image_t* img, const uint8_t* text, size_t n, uint32_t mode, const char* stop, uint64_t longest_allowed,
                                 int device, std::vector<uint8_t>& results, uint64_t* longest);

namespace {

// the splitting rule of include/mfa_hip.h ("text to batch") on the host: what match_text falls back to
void split_on_host(const uint8_t* text, size_t n, bool tokens, const char* stop, vector<uint8_t>& bytes, vector<uint64_t>& offsets) {
    bytes.clear();
    offsets.assign(1, 0);
    const size_t stop_len = stop ? strlen(stop) : 0;
    auto is_sep = [&](uint8_t c) { return tokens ? ((c >= 0x09 && c <= 0x0d) || c == 0x20) : c == 0x0a; };
    size_t p = 0;
    while (p < n) {
        if (tokens) {
            while (p < n && is_sep(text[p])) p++;
            if (p == n) break;
        }
        size_t e = p;
        while (e < n && !is_sep(text[e])) e++;
        if (tokens && stop_len && e - p == stop_len && memcmp(text + p, stop, stop_len) == 0) break;
        bytes.insert(bytes.end(), text + p, text + e);
        offsets.push_back(bytes.size());
        p = tokens ? e : e + 1;                                // (lines: behind the newline; a text that ends there has no further line)
    }
}

}  // namespace

void Automata::match_text(const uint8_t* text, size_t n, bool tokens, const char* stop, vector<uint8_t>& results) {
    mfa_image* img = image_for_match();
    uint64_t longest = 0;
    const uint64_t beyond = piece_rule().beyond;
    int rc = diploma_match_text_on_device(img, text, n, tokens ? MFA_SPLIT_TOKENS : MFA_SPLIT_LINES, stop, beyond, device, results, &longest);
    if (rc != MFA_OK) fail("Automata::match_text", rc);
    if (longest <= beyond) {
        for (uint8_t& r : results) r = r == 1 ? 1 : 0;
        return;
    }
    // a string beyond what one device call takes: match_packed knows how to cut such strings (or, for a memory automaton, refuses them)
    vector<uint8_t> bytes;
    vector<uint64_t> offsets;
    split_on_host(text, n, tokens, stop, bytes, offsets);
    results.assign(offsets.size() - 1, 0);
    bytes.resize(bytes.size() + 16);
    if (!results.empty()) match_packed(bytes.data(), offsets.data(), offsets.size() - 1, results.data());
}

// text_match.cpp: the same with the selection on the device too
int diploma_select_text_on_device(mfa_image_t* img, const uint8_t* text, size_t n, uint32_t mode, const char* stop, uint64_t longest_allowed,
                                  int device, bool invert, std::string& out, uint64_t* n_unanswered, uint64_t* longest);

void Automata::select_text(const uint8_t* text, size_t n, bool tokens, const char* stop, bool invert, std::string& out, uint64_t* n_unanswered) {
    out.clear();
    uint64_t unanswered = 0;
    const char* on_device = getenv("DIPLOMA_DEVICE_SELECT");
    if (!(on_device && on_device[0] == '0' && on_device[1] == 0)) {
        mfa_image* img = image_for_match();
        uint64_t longest = 0;
        const uint64_t beyond = piece_rule().beyond;
        int rc = diploma_select_text_on_device(img, text, n, tokens ? MFA_SPLIT_TOKENS : MFA_SPLIT_LINES, stop, beyond, device, invert, out, &unanswered,
                                               &longest);
        if (rc != MFA_OK) fail("Automata::select_text", rc);
        if (longest <= beyond) {
            if (n_unanswered) *n_unanswered = unanswered;
            return;
        }
    }
    // the selection on the host: the answers of match_text (which cuts a string beyond what one device call takes) and the split rule again
    vector<uint8_t> results, bytes;
    vector<uint64_t> offsets;
    match_text(text, n, tokens, stop, results);
    split_on_host(text, n, tokens, stop, bytes, offsets);
    out.clear();
    for (size_t k = 0; k + 1 < offsets.size() && k < results.size(); k++) {
        if ((results[k] == 1) == invert) continue;
        out.append(reinterpret_cast<const char*>(bytes.data()) + offsets[k], offsets[k + 1] - offsets[k]);
        out += '\n';
    }
    if (n_unanswered) *n_unanswered = 0;
}

// text_match.cpp: the lines of the text searched on the device
int diploma_search_text_on_device(mfa_image_t* img, const uint8_t* text, size_t n, int device, bool invert, bool only_matching, std::string& out,
                                  uint64_t* n_unanswered);

void Automata::search_text(const uint8_t* text, size_t n, bool invert, bool only_matching, std::string& out, uint64_t* n_unanswered) {
    uint64_t unanswered = 0;
    const int rc = diploma_search_text_on_device(image_for_match(), text, n, device, invert, only_matching, out, &unanswered);
    if (rc != MFA_OK) fail("Automata::search_text", rc);
    if (n_unanswered) *n_unanswered = unanswered;
}

void Automata::match_packed_short(mfa_image* img,const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results) {
    // the devices of the node: all of them by default (north_star: "the string batch shards trivially across the 8 GPUs of one node")
    const int count = mfa_device_count();
    int want = devices;
    if (const char* e = getenv("DIPLOMA_DEVICES")) want = atoi(e);
    unsigned use = count <= 0 ? 1u : (want <= 0 ? (unsigned)count : (unsigned)std::min(want, count));
    unsigned shards = use;
    if (const char* e = getenv("DIPLOMA_FORCE_SHARDS")) shards = (unsigned)std::max(1, atoi(e));      // (tests: several shards on the devices there are)
    const uint64_t total = n ? offsets[n] - offsets[0] : 0;
    if (shards <= 1 || (!getenv("DIPLOMA_FORCE_SHARDS") && (n < 2ull * shards || total < (4ull << 20)))) {
        int rc = mfa_match_batch_host(img, bytes, offsets, n, results, device);
        if (rc != MFA_OK) fail("mfa_match_batch_host", rc);
        return;
    }
    vector<uint64_t> cuts(shards + 1);
    diploma_partition_by_bytes(offsets, n, shards, cuts.data());
    vector<int> rcs(shards, MFA_OK);
    vector<std::thread> workers;
    for (unsigned r = 0; r < shards; r++) {
        if (cuts[r + 1] == cuts[r]) continue;
        const int dev = (device + (int)(r % use)) % std::max(count, 1);
        workers.emplace_back([&, r, dev]() {                      // (HIP's current device is per host thread; the C-ABI is re-entrant per device)
            rcs[r] = mfa_match_batch_host(img, bytes, offsets + cuts[r], cuts[r + 1] - cuts[r], results + cuts[r], dev);
        });
    }
    for (std::thread& t : workers) t.join();
    for (unsigned r = 0; r < shards; r++)
        if (rcs[r] != MFA_OK) fail("mfa_match_batch_host (one of the devices)", rcs[r]);
}

vector<bool> Automata::match_batch(const vector<string>& strs) {
    vector<uint64_t> off(strs.size() + 1, 0);
    for (size_t k = 0; k < strs.size(); k++) off[k + 1] = off[k] + strs[k].size();
    vector<uint8_t> bytes(off.back() + 16);
    for (size_t k = 0; k < strs.size(); k++) std::copy(strs[k].begin(), strs[k].end(), bytes.begin() + off[k]);
    vector<uint8_t> res(strs.size() + 1);
    match_packed(bytes.data(), off.data(), strs.size(), res.data());
    return vector<bool>(res.begin(), res.begin() + strs.size());
}

bool Automata::match(const string& str) {
    uint64_t off[2] = {0, str.size()};
    uint8_t res = 0;
    match_packed(reinterpret_cast<const uint8_t*>(str.data()), off, 1, &res);
    return res != 0;
}

// ---- Automata::Stream -----------------------------------------------------------------------------------

Automata::Stream::Stream(Automata& automata) : automata_(automata) { reset(); }

void Automata::Stream::reset() {
    state_ = MFA_DFA_STATE_START;
    feed(string());                              // the answer for the empty text
}

void Automata::Stream::feed(const string& block) {
    mfa_image* img = automata_.image_for_match();
    mfa_image_info info;
    int rc = mfa_image_get_info(img, &info);
    if (rc != MFA_OK) fail("mfa_image_get_info", rc);
    if (info.kind == MFA_KIND_NFA && info.dfa_states == 0)
        throw std::runtime_error("Automata::Stream: the automaton's state sets pass the tabulation limit; it is walked as a set of nodes, which is not carried from block to block");
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(block.data());
    vector<uint8_t> stage;
    for (uint64_t r = 0; r == 0 || r * kPieceBytes < block.size(); r++) {
        uint64_t lo, hi;
        piece_of(0, block.size(), r, info.is_reversed != 0, kPieceBytes, &lo, &hi);
        stage.assign(bytes + lo, bytes + hi);
        stage.resize(stage.size() + 16);
        const uint64_t off[2] = {0, hi - lo};
        uint8_t res = 0;
        rc = mfa_match_batch_resume_host(img, stage.data(), off, 1, &state_, &res, automata_.device);
        if (rc != MFA_OK) fail("mfa_match_batch_resume_host", rc);
        accepted_ = res == 1;
    }
}

// ---- MFA ----------------------------------------------------------------------------------------------

MFA::MFA() {
    start = new MemoryNode();
    finish = new MemoryNode();
    nodes.push_back(start);
    nodes.push_back(finish);
    last_idx = 0;
}

void MFA::changeFinalState(MemoryNode* new_final) {                              // mfa.cpp:11-26
    for (MemoryNode* n : nodes)
        for (MemoryEdge* e : n->edges)
            if (e->to == finish) e->to = new_final;
    auto it = std::find(nodes.begin(), nodes.end(), finish);
    if (it != nodes.end()) nodes.erase(it);
}

void MFA::makeDOTFile(const string& filename) {                                  // mfa.cpp:28-61
    string text = "digraph g {\n";
    for (MemoryNode* n : nodes) {
        if (n->name.empty()) n->name = std::to_string(last_idx++);
        for (MemoryEdge* e : n->edges) {
            if (e->to->name.empty()) e->to->name = std::to_string(last_idx++);
            if (e->by.empty()) e->by = "\xce\xb5";          // the reference rewrites the label itself (mfa.cpp:40-42)
            if (e->drawn) continue;
            string acts;
            for (const auto& kv : e->memoryActions) acts += string(kv.second == open ? "o" : "c") + kv.first + "/";
            text += "\t" + n->name + " -> " + e->to->name + " [label=\"" + e->by + "/" + acts + "\"]\n";
        }
    }
    text += "}";
    std::ofstream out(filename + ".dot");
    if (out.is_open()) out << text;
}

bool MFA::draw(const string& filename) {
    makeDOTFile(filename);
    return true;
}

vector<uint8_t> MFA::image_blob() const {
    map<MemoryNode*, size_t> idx;
    vector<MemoryNode*> all;
    for (MemoryNode* n : nodes) index_of(idx, all, n);
    index_of(idx, all, start);
    index_of(idx, all, finish);
    for (size_t k = 0; k < all.size(); k++)
        for (MemoryEdge* e : all[k]->edges) index_of(idx, all, e->to);
    vector<FlatNode> flat(all.size());
    for (size_t k = 0; k < all.size(); k++) {
        flat[k].seq = all[k]->seq;
        for (MemoryEdge* e : all[k]->edges) flat[k].edges.push_back({e->by, idx[e->to], &e->memoryActions});
    }
    return serialise(MFA_KIND_MFA, is_reversed, flat, idx[start], idx[finish]);
}

void MFA::match_packed(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results) {
    Automata::match_packed(bytes, offsets, n, results);        // image_blob() is virtual: freezes the MFA graph
}

vector<bool> MFA::match_batch(const vector<string>& strs) { return Automata::match_batch(strs); }

void MFA::match_text(const uint8_t* text, size_t n, bool tokens, const char* stop, vector<uint8_t>& results) {
    Automata::match_text(text, n, tokens, stop, results);      // image_blob() is virtual, as for match_packed
}

void MFA::select_text(const uint8_t* text, size_t n, bool tokens, const char* stop, bool invert, std::string& out, uint64_t* n_unanswered) {
    Automata::select_text(text, n, tokens, stop, invert, out, n_unanswered);      // image_blob() is virtual, as for match_packed
}

void MFA::search_text(const uint8_t* text, size_t n, bool invert, bool only_matching, std::string& out, uint64_t* n_unanswered) {
    Automata::search_text(text, n, invert, only_matching, out, n_unanswered);      // (the library refuses a memory automaton: the caller hears its message)
}

vector<vector<bool>> match_mixed(const vector<MFA*>& automata, const vector<vector<string>>& strs) {
    return match_mixed(vector<Automata*>(automata.begin(), automata.end()), strs);
}

// automata of either kind, as compile() returns them (image_blob() is virtual: an MFA behind an Automata* gives its own image)
vector<vector<bool>> match_mixed(const vector<Automata*>& automata, const vector<vector<string>>& strs) {
    if (automata.empty() || automata.size() != strs.size()) throw std::runtime_error("match_mixed: one list of strings per automaton");
    vector<mfa_image_t*> images;
    for (Automata* m : automata) images.push_back(m->image_for_match());
    mfa_mixed_t* mx = nullptr;
    int rc = mfa_mixed_create(images.data(), (uint32_t)images.size(), &mx);
    if (rc != MFA_OK) fail("mfa_mixed_create", rc);
    vector<uint64_t> off{0}, seg{0};
    vector<uint8_t> bytes;
    // a string of a memory-less automaton beyond the device's per-call limit stands in the batch as an empty one and is matched by itself, in pieces
    vector<std::pair<size_t, const string*>> longs;      // (index in the batch, the string)
    vector<Automata*> long_owner;
    for (size_t k = 0; k < strs.size(); k++) {
        mfa_image_info info;
        const bool memory_less = mfa_image_get_info(images[k], &info) == MFA_OK && info.kind == MFA_KIND_NFA;      // (tabulated or set walk: its strings may go in pieces)
        for (const string& s : strs[k]) {
            if (memory_less && s.size() > piece_rule().beyond) { longs.push_back({off.size() - 1, &s}); long_owner.push_back(automata[k]); }
            else bytes.insert(bytes.end(), s.begin(), s.end());
            off.push_back(bytes.size());
        }
        seg.push_back(off.size() - 1);
    }
    bytes.resize(bytes.size() + 16);
    const uint64_t n = off.size() - 1;
    vector<uint8_t> res(n + 1);
    rc = mfa_match_mixed_host(mx, bytes.data(), off.data(), n, seg.data(), res.data(), automata[0]->device);
    mfa_mixed_destroy(mx);
    if (rc != MFA_OK) fail("mfa_match_mixed_host", rc);
    for (size_t j = 0; j < longs.size(); j++) res[longs[j].first] = long_owner[j]->Automata::match(*longs[j].second);
    vector<vector<bool>> out;
    for (size_t k = 0; k < strs.size(); k++) out.emplace_back(res.begin() + seg[k], res.begin() + seg[k + 1]);
    return out;
}

bool MFA::match(string str) { return Automata::match(str); }
