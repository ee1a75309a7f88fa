// Host-side mirror of the reference's C++ API for the match path, backed by the MI355X
// kernels through the C-ABI of include/mfa_hip.h.
//
// Same class names, public fields and call signatures as the reference, so code written
// against it (matchers/match.cpp:10-32, matchers/match_mfa.cpp:13-97,
// matchers/example_runner.cpp:106-111) compiles against this header unchanged:
//
//   reference                              here
//   ---------------------------------------------------------------------------------------
//   variable.h:8-41    Variable            Variable            (kept for source parity; the
//                                                               kernels hold cells as spans)
//   edge.h:13-49       Edge, MemoryEdge,   same                + `seq`
//                      MemoryAction
//   node.h:11-38       Node, MemoryNode    same                + `seq`
//   automata.h:18-84   Automata, MFA       same                match() runs on the GPU;
//                                                              + match_batch(), image_blob()
//   bt/binary_tree.h   BinaryTree          same                toThomson/toGlushkov/toMFA
//   regex/regex.h      Regexp, RegexpType  same                parse_regexp/to_binary_tree/
//                                                              compile/reverse (memory-less)
//
// What is different, and why:
//  * `seq`: the reference orders nodes, edges and states by raw heap pointers
//    (automata.h:12-13, bt/bt_mfa.cpp:51,87,91,122-128, bt/bt_thomson.cpp:26-27).  Under the
//    canonical allocation-order model a pointer comparison is an
//    allocation-sequence comparison; every graph object here carries the sequence number the
//    reference's allocation would have had, and every place the reference compares pointers
//    compares `seq` instead.  Results are then independent of the host heap.
//  * match() does not walk the graph on the CPU.  The graph is frozen into an automaton
//    image (include/mfa_image_format.h) and handed to libmfa_hip.so; there is no CPU fallback:
//    without a usable GPU match() throws std::runtime_error.
//  * The BNF rewriter and the reversal of memory regexes (regex/bnf.cpp, helpers.cpp, reverse.cpp) are restated in
//    bnf_rewrite.cpp.  Two paths of the reference's rewriter read freed or uninitialised memory (a default argument that
//    is an iterator into a destroyed temporary, bnf.cpp:805 with 544-552; an uninitialised iterator, bnf.cpp:409-418):
//    regexes that reach them throw std::runtime_error here instead of repeating an accident.
#ifndef DIPLOMA_API_H
#define DIPLOMA_API_H

#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

using namespace std;   // the reference's headers do this (automata.h:15, node.h:9, edge.h:8)

struct mfa_image;      // include/mfa_hip.h

namespace diploma {
uint64_t next_seq();   // allocation sequence number (monotonic, process-wide)
}

// ---- variable.h -----------------------------------------------------------------------------------
class Variable {
public:
    bool is_open = false;
    bool is_read = false;
    string value;
    Variable() = default;
    Variable(bool open_, string v, bool read_ = false) : is_open(open_), is_read(read_), value(std::move(v)) {}
    void open() { is_open = true; is_read = false; value.clear(); }
    void close() { is_open = false; }
    string& read() { is_read = true; return value; }
    void write(const string& a) { value += a; }
};

// ---- edge.h / node.h --------------------------------------------------------------------------------
class Node;
class MemoryNode;

class Edge {
public:
    string by;
    Node* to = nullptr;
    bool drawn = false;
    uint64_t seq = diploma::next_seq();
    Edge() = default;
    Edge(string label, Node* target) : by(std::move(label)), to(target) {}
};

enum MemoryAction { open, close };

class MemoryEdge : public Edge {
public:
    map<string, MemoryAction> memoryActions;
    MemoryNode* to = nullptr;
    MemoryEdge() = default;
    MemoryEdge(string label, MemoryNode* target) : to(target) { by = std::move(label); }
    void addAction(const string& var, MemoryAction action) { memoryActions[var] = action; }
};

class Node {
public:
    list<Edge*> edges;
    string name;
    Node* finish_for = nullptr;
    Node* start_for = nullptr;
    uint64_t seq = diploma::next_seq();
    Node() = default;
    explicit Node(string n) : name(std::move(n)) {}
};

class MemoryNode {
public:
    list<MemoryEdge*> edges;
    string name;
    uint64_t seq = diploma::next_seq();
    MemoryNode() = default;
    explicit MemoryNode(string n) : name(std::move(n)) {}
};

// ---- automata.h ---------------------------------------------------------------------------------------
#define Memory map<string, Variable*>
#define MemoryState pair<int, pair<MemoryNode*, Memory>>

class MFA;
class Automata;
vector<vector<bool>> match_mixed(const vector<MFA*>& automata, const vector<vector<string>>& strs);
vector<vector<bool>> match_mixed(const vector<Automata*>& automata, const vector<vector<string>>& strs);

class Automata {
public:
    Node* start;
    Node* finish;
    int last_idx;
    list<Node*> nodes;
    bool is_reversed = false;

    Automata();
    virtual ~Automata();

    void makeDOTFile(const string& filename);
    bool draw(const string& filename);
    void changeFinalState(Node* new_final);
    bool isDeterministic();

    // reference automata.cpp:177-210, on the GPU (a batch of one).  A memory-less automaton takes strings of any length: one beyond the
    // device's per-call limit (MFA_MAX_STRING_BYTES) is cut into pieces of 8 MiB that go through mfa_match_batch_resume_host (for an automaton
    // walked as a set of nodes: mfa_match_batch_resume_set_host, or _set_wide_host when it is walked one string per wave;
    // mfa_image_resume_state_bytes says which) round by round, last piece first for a reversed automaton; match_batch, match_packed and the memory-less segments of match_mixed do the
    // same, and the shorter strings of the batch take the one call they always took.  A memory automaton refuses such a string as before.
    // Environment, for tests: DIPLOMA_PIECE_BYTES=n (a multiple of 16, at least 16) makes both the limit and the piece size n.
    bool match(const string& str);
    // the same for many strings in one launch; result[k] is what match(strs[k]) returns
    vector<bool> match_batch(const vector<string>& strs);
    // packed form: string k is bytes[offsets[k], offsets[k+1]); results gets n bytes of 0/1
    void match_packed(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results);
    // A whole text: split into strings ON THE DEVICE (include/mfa_hip.h, "text to batch") and matched where they lie -- one upload of the
    // text, the split, one read-back of the 32-byte info record, the plain match call, the results back -- on `device` alone.  tokens:
    // false = one string per line, as std::getline cuts them; true = one per whitespace-separated token, as `cin >> text` does, up to
    // the first token equal to `stop` (nullptr: none).  results gets one 0/1 byte per string.  If the text holds a string beyond what one
    // device call takes, the text is split on the host instead and goes through match_packed, which knows how to cut such strings.
    void match_text(const uint8_t* text, size_t n, bool tokens, const char* stop, vector<uint8_t>& results);
    // The strings of a text that the automaton accepts -- rejects, with `invert` -- as a text of their own in `out`, each with a 0x0a
    // behind it: what `grep -x` (`grep -vx`) prints.  Split, matched and SELECTED on the device (include/mfa_hip.h, "batch to text"): one
    // upload of the text, the split, the plain match call, mfa_select_count, one read-back of the 32-byte info record, mfa_select_write
    // with MFA_SELECT_NEWLINE, one read-back of exactly the kept bytes; no offsets and no result bytes come to the host.  text, tokens
    // and stop as for match_text.  *n_unanswered (may be nullptr): strings the device answered neither 0 nor 1; they are never kept.  If
    // the text holds a string beyond what one device call takes, or under DIPLOMA_DEVICE_SELECT=0, the selection is done on the host from
    // the answers of match_text; the output is the same.
    void select_text(const uint8_t* text, size_t n, bool tokens, const char* stop, bool invert, std::string& out, uint64_t* n_unanswered);
    // The lines of a text that CONTAIN a match -- with `invert`: that contain none -- each with a 0x0a behind it: what `grep` (`grep -v`)
    // prints; with `only_matching` instead the leftmost-longest match of every line that has one, one per output line (an empty match
    // is an empty line).  Split, searched (include/mfa_hip.h, "search inside lines") and selected on one device: upload, split,
    // mfa_search_batch, the selection, its info record back, the kept bytes back.  For a tabulated memory-less automaton; anything the
    // library refuses throws with its message.  *n_unanswered (may be nullptr): lines beyond what the search reads; they are never kept.
    void search_text(const uint8_t* text, size_t n, bool invert, bool only_matching, std::string& out, uint64_t* n_unanswered);

    // the automaton image handed to the device (include/mfa_image_format.h)
    virtual vector<uint8_t> image_blob() const;
    int device = 0;    // HIP device the match calls run on (the first one, when a batch is spread over several)
    // How many HIP devices a packed batch is spread over: 0 = all the node has, 1 = `device` only.  Strings are independent: the batch is
    // cut into contiguous ranges of about equal BYTES (diploma_partition_by_bytes), one host thread per device copies its range in,
    // matches it through the C-ABI and copies the answers back into place; no exchange between devices.  Small batches (under 4 MiB, or
    // fewer strings than twice the devices) go to `device` alone.  Environment: DIPLOMA_DEVICES=N overrides this field.
    int devices = 0;

    // A memory-less automaton on text that arrives in blocks (a log, a file larger than memory): feed() the blocks in the order the
    // automaton scans -- front to back, and for a reversed automaton (is_reversed) LAST block first -- and accepted() tells whether the
    // text fed so far matches, what match() answers for the concatenation.  Every feed() is one device call (mfa_match_batch_resume_host);
    // blocks of any size.  The automaton must outlive the stream and must not change while it is fed.  A memory automaton throws.
    class Stream {
    public:
        explicit Stream(Automata& automata);
        void feed(const string& block);
        bool accepted() const { return accepted_; }
        void reset();                           // back to the empty text
    private:
        Automata& automata_;
        uint32_t  state_ = 0;                   // the state-set number the device hands back; meaningless outside this object
        bool      accepted_ = false;
    };

protected:
    friend vector<vector<bool>> match_mixed(const vector<Automata*>& automata, const vector<vector<string>>& strs);
    mfa_image* image_for_match();
    void match_packed_short(mfa_image* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results);      // every string within the per-call limit
    mfa_image* cached_image_ = nullptr;
    vector<uint8_t> cached_blob_;
};

class MFA : public Automata {
public:
    MemoryNode* start;
    MemoryNode* finish;
    list<MemoryNode*> nodes;
    bool is_reversed = false;

    MFA();

    void changeFinalState(MemoryNode* new_final);
    void makeDOTFile(const string& filename);
    bool draw(const string& filename);

    // reference mfa.cpp:215-236, on the GPU.  Non-virtual like the reference's: callers that hold an
    // Automata* static_cast to MFA* when compile() set is_mfa (matchers/match.cpp:16-19).
    bool match(string str);
    vector<bool> match_batch(const vector<string>& strs);
    void match_packed(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* results);
    void match_text(const uint8_t* text, size_t n, bool tokens, const char* stop, vector<uint8_t>& results);
    void select_text(const uint8_t* text, size_t n, bool tokens, const char* stop, bool invert, std::string& out, uint64_t* n_unanswered);
    void search_text(const uint8_t* text, size_t n, bool invert, bool only_matching, std::string& out, uint64_t* n_unanswered);

    vector<uint8_t> image_blob() const override;
};

// ---- regex/regex.h ---------------------------------------------------------------------------------------
class BinaryTree;

enum RegexpType {
    leftParenthesis, rightParenthesis, leftBrace, rightBrace, leftSquareBr, rightSquareBr, dash,
    kleeneStar, kleenePlus, alternation, literal, epsilon,
    alternationExpr, concatenationExpr, backreferenceExpr, reference, rootExpr
};

class Regexp {
public:
    RegexpType regexp_type = rootExpr;
    string regexp_str;
    char rune = 0;                    // literal
    Regexp* sub_regexp = nullptr;     // kleene, backreference body
    list<Regexp*> sub_regexps;        // alternation, concatenation
    string variable;                  // backreference / reference name
    bool is_read = false;
    Regexp* reference_to = nullptr;
    bool have_backreference = false;
    bool is_one_unamb = false;
    bool is_bad_bnf = false;

    bool is_slided = false;           // an iteration over a read/write block that has been unrolled already (regex.h:97)

    // variable-flow sets (regex.h:99-121), maintained while a tree is analysed or rebuilt
    map<string, list<Regexp*>> initialized;   // cells initialised on every path, with their initialisations in order
    set<string> read;                         // cells read on every path
    set<string> maybe_initialized;            // cells some path may initialise
    set<string> maybe_read;                   // cells some path may read
    set<string> uninited_read;                // reads some path reaches without an initialisation before them
    set<string> unread_init;                  // initialisations some path leaves unread
    set<string> definitely_unread_init;       // initialisations nothing behind them reads (cleared from the result)
    set<string> definitely_uninit_read;       // reads no initialisation precedes (under an iteration)
    set<string> rw_vars;                      // cells that form a read..write block at this level

    Regexp() = default;
    explicit Regexp(RegexpType t) : regexp_type(t) {}

    static Regexp* parse_regexp(string& s);           // consumes s, like the reference (parser.cpp:8)
    string to_string();
    bool is_backref_correct();
    BinaryTree* to_binary_tree();
    Regexp* reverse();                                // regex/reverse.cpp:104-113
    Regexp* bnf(bool is_log = false);                 // regex/bnf.cpp:894-919
    bool is_acreg();                                  // regex/helpers.cpp:4-21
    Automata* compile(bool& is_mfa, bool use_reverse, bool use_bnf, bool use_ssnf, bool use_log = false);

private:
    void close_alternative();                         // '|'
    void close_group();                               // ')'
    void wrap_kleene(char c);
    void close_backreference(string name);
    void close_enumeration();
    Regexp* mirrored();

    // ---- bnf_rewrite.cpp: the reference's regex/helpers.cpp, regex/bnf.cpp, regex/reverse.cpp and the flow analysis of
    //      regex/regex.cpp:91-147 restated (same order of every list and set operation, since the result is order sensitive)
    void analyse(set<string>& seen_inits);
    bool same_shape(Regexp* other);
    Regexp* last_init(const string& var);
    Regexp* prefix_last_init(const string& var, list<Regexp*>::iterator it);
    bool crosses_references();
    map<string, list<string>> reads_inside_inits();
    void put(Regexp* r, bool front);
    void put_sequence(Regexp* r, bool front);
    void put_choice(Regexp* r, bool front);
    void add(Regexp* r, bool front = false);
    void flow_after(Regexp* r);                       // concat_vars
    void flow_beside(Regexp* r);                      // alt_vars
    void flow_under_star(Regexp* r);                  // star_kleene_vars
    void flow_same(Regexp* r);                        // copy_vars
    void flow_replace(Regexp* r);                     // change_vars
    static Regexp* clone(Regexp* r);                  // copy
    Regexp* unwrap_single();                          // simplify_conc_alt
    set<string> choice_free_reads();
    map<string, int> choice_init_counts();
    Regexp* strip_dead_memory(set<string> init_vars, set<string> read_vars);
    Regexp* unroll_plus(set<string> vars, bool strip = true);
    Regexp* unroll(set<string> vars, bool strip = true);
    Regexp* unroll_for_reads(set<string> vars, Regexp* parent, list<Regexp*>::iterator where);
    list<string> order_choice_vars(bool smallest_first);
    Regexp* split_choice_under_star(bool smallest_first = false);
    Regexp* split_choice_on(const string& var);
    Regexp* denest(Regexp* a_alt, Regexp* b_alt);
    Regexp* slide_last_init(set<string> vars);
    Regexp* rw_sequence_under_star(Regexp* parent, bool have_where, list<Regexp*>::iterator where);
    Regexp* rw_choice_under_star();
    Regexp* rw_under_star(Regexp* parent, bool have_where, list<Regexp*>::iterator where);
    Regexp* hoist_choice_out_of_init();
    Regexp* spread_right(int alt_pos);
    Regexp* spread_left(int alt_pos);
    Regexp* spread_both(int alt_pos);
    Regexp* sequence_fix_unread_inits();
    Regexp* sequence_fix_free_reads();
    Regexp* normalise(Regexp* parent, bool under_star, bool have_where, list<Regexp*>::iterator where);
    Regexp* swap_reads_and_inits(set<Regexp*>& done);
    void bind_reads(map<string, Regexp*>& init);
};

// ---- bt/binary_tree.h ---------------------------------------------------------------------------------
class BinaryTree {
public:
    BinaryTree() {}
    explicit BinaryTree(RegexpType t) : type(t) {}

    RegexpType type = epsilon;
    BinaryTree* left = nullptr;     // concatenation and alternation
    BinaryTree* right = nullptr;
    BinaryTree* child = nullptr;    // Kleene, backreference body
    char rune = 0;                  // literal
    string variable;                // reference and backreferenceExpr
    string name;

    bool epsilonProducing();
    list<string> linearize(int&);
    list<string> doFIRST();
    list<string> doLAST();
    set<pair<string, string>> doFOLLOW();
    bool is_one_unambiguity();
    BinaryTree* toSSNF();           // star normal form (bt/bt_ssnf.cpp:73-108)
    BinaryTree* starBody();         // the same for a subtree that sits under an iteration (bt/bt_ssnf.cpp:18-71); nullptr: nothing left

    Automata* toThomson();
    Automata* toGlushkov();
    MFA* toMFA();
};

std::string substr(std::string originalString, int maxLength);

// matchers/match.cpp:10 -- the `-match` loop: compile once, then 0/1 per whitespace-separated token of
// stdin until the token `exit` (or end of input), batched onto the GPU
void match(string regexp_str, bool reverse, bool bnf, bool ssnf, bool use_log = false);
// `diploma -match-lines FILE`: compile as match() does (the header lines are printed), then one 0/1 line per line of FILE, the file
// split into lines on the device (Automata::match_text).  false: FILE cannot be read
bool match_lines(string regexp_str, const string& path, bool reverse, bool bnf, bool ssnf);
// `diploma -grep-lines FILE [-v]`: compile as match() does (the header lines are printed), then the lines of FILE that match -- with
// `invert` those that do not -- each followed by a newline, selected on the device (Automata::select_text).  false: FILE cannot be read.
// *n_unanswered: lines the device answered neither 0 nor 1 (they are not printed)
bool grep_lines(string regexp_str, const string& path, bool invert, bool reverse, bool bnf, bool ssnf, uint64_t* n_unanswered);
// `diploma -search-lines FILE [-v | -o]`: compile as match() does (the header lines are printed), then the lines of FILE that contain a
// match (`invert`: that contain none), or with `only_matching` the leftmost-longest match of every line that has one, each followed by a
// newline (Automata::search_text).  false: FILE cannot be read.  *n_unanswered: lines the search did not read (they are not printed)
bool search_lines(string regexp_str, const string& path, bool invert, bool only_matching, bool reverse, bool bnf, bool ssnf, uint64_t* n_unanswered);
// matchers/match_mfa.cpp:13,58 counterparts: strings from a file (one per line), one batch, results and
// timing on stdout
// The cut points of a batch over `parts` devices: cuts[r] .. cuts[r+1]-1 are the strings of part r (parts + 1 values, cuts[0] = 0,
// cuts[parts] = n), balanced by bytes -- the rule of mfa_amd/sharding.py: part r starts at the first string whose offset is at least
// r / parts of the batch's bytes.  Returns 0, or -1 for bad arguments.
extern "C" int diploma_partition_by_bytes(const uint64_t* offsets, uint64_t n, uint32_t parts, uint64_t* cuts);

// several automata, one batch: strs[k] are matched against automata[k] (memory automata only) by ONE device call
// (mfa_match_mixed: the region pre-pass and the walks of all of them scheduled together); results[k][j] = automata[k] matches strs[k][j]
vector<vector<bool>> match_mixed(const vector<MFA*>& automata, const vector<vector<string>>& strs);
void match_gt(string regexp_str, const string& input_path = "input_strings.txt");
void match_mfa(string regexp_str, const string& input_path = "mfa_str.txt");

// matchers/example_runner.cpp:15 -- the attack-string generator: only pump parts 0 and 1 are used
std::string pumped_string(int n, vector<string> pump_v);
// matchers/example_runner.cpp:84 (`./diploma -match N`): reads test/example_N/regexp.txt and pump.txt below
// the working directory, matches ever longer pumped strings one at a time and writes "len seconds" lines to
// test/example_N/diploma_results.txt until one match takes 0.5 s or longer (see drivers.cpp for what differs)
void run_configuration_examples(const string& number);

#endif  // DIPLOMA_API_H
