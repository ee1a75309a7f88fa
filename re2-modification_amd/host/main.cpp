// `diploma` command line (reference main.cpp:9-87).
//   diploma -match [-bnf] [-reverse] [-ssnf] [-all] [-log]    regex token, then string tokens until `exit`
//   diploma -match N                                          timing series over test/example_N (example_runner.cpp)
//   diploma -match-blocks N [-bnf] [-reverse] [-ssnf] [-all]  as -match for a memory-less regex, every token fed to an Automata::Stream N bytes at a time
//   diploma -match-lines FILE [-bnf] [-reverse] [-ssnf] [-all]  regex token from stdin, then one 0/1 line per line of FILE, split on the device
//   diploma -grep-lines FILE [-v] [-bnf] [-reverse] [-ssnf] [-all]  regex token from stdin, then the lines of FILE that match (-v: that do not), selected on the device
//   diploma -search-lines FILE [-v | -o] [-bnf] [-reverse] [-ssnf] [-all]  regex token from stdin, then the lines of FILE that contain a match (-v: that contain none; -o: the first leftmost-longest match of each line, one per output line -- unlike grep -o one match per line, and an empty match prints an empty line), searched on the device
//   diploma -dump  [-thompson|-glushkov|-mfa]                 regex token -> automaton image as text
//   diploma -match-file <gt|mfa> <file>                       matchers/match_mfa.cpp counterparts
//   diploma -match-mixed [-bnf|-reverse|-ssnf|-all] FILE...   one regex and its strings per file, all files in ONE device call
#include <algorithm>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "diploma_api.h"

namespace {

string hexlabel(const string& by) {
    if (by.empty() || by == "\xce\xb5") return "-";
    static const char* d = "0123456789abcdef";
    string h;
    for (unsigned char c : by) { h += d[c >> 4]; h += d[c & 15]; }
    return h;
}

template <class NodeT, class EdgeFn>
void dump_graph(const char* kind, bool reversed, const list<NodeT*>& listed, NodeT* start, NodeT* finish, EdgeFn print_extra) {
    vector<NodeT*> all;
    map<NodeT*, size_t> idx;
    auto add = [&](NodeT* n) { if (!idx.count(n)) { idx[n] = all.size(); all.push_back(n); } };
    for (NodeT* n : listed) add(n);
    add(start); add(finish);
    for (size_t k = 0; k < all.size(); k++)
        for (auto* e : all[k]->edges) add(e->to);
    vector<uint64_t> seqs;
    for (NodeT* n : all) seqs.push_back(n->seq);
    std::sort(seqs.begin(), seqs.end());
    cout << "kind " << kind << "\nreversed " << (reversed ? 1 : 0) << "\nnodes " << all.size() << "\nstart " << idx[start]
         << "\nfinish " << idx[finish] << "\n";
    for (size_t k = 0; k < all.size(); k++) {
        size_t rank = std::lower_bound(seqs.begin(), seqs.end(), all[k]->seq) - seqs.begin();
        cout << "node " << k << " " << rank << " " << all[k]->edges.size() << "\n";
        for (auto* e : all[k]->edges) {
            cout << "edge " << hexlabel(e->by) << " " << idx[e->to];
            print_extra(e);
            cout << "\n";
        }
    }
}

int do_dump(int argc, char** argv) {
    string mode = argc > 2 ? argv[2] : "";
    string regex;
    cin >> regex;
    std::ostringstream sink;                       // compile() prints its header lines: keep the dump clean
    std::streambuf* old = cout.rdbuf(sink.rdbuf());
    Regexp* re = Regexp::parse_regexp(regex);
    Automata* nfa = nullptr;
    MFA* mfa = nullptr;
    if (mode == "-thompson") nfa = re->to_binary_tree()->toThomson();
    else if (mode == "-glushkov") nfa = re->to_binary_tree()->toGlushkov();
    else if (mode == "-mfa") { re->is_backref_correct(); mfa = re->to_binary_tree()->toMFA(); }
    else {
        bool is_mfa = false;
        const bool all = mode == "-all";                   // -all = -bnf -reverse -ssnf (main.cpp:25-29)
        Automata* a = re->compile(is_mfa, mode == "-reverse" || all, mode == "-bnf" || mode == "-reverse" || all, mode == "-ssnf" || all);
        if (is_mfa) mfa = static_cast<MFA*>(a); else nfa = a;
    }
    cout.rdbuf(old);
    if (mfa)
        dump_graph("mfa", mfa->is_reversed, mfa->nodes, mfa->start, mfa->finish, [](MemoryEdge* e) {
            for (const auto& kv : e->memoryActions) cout << " " << (kv.second == open ? 'o' : 'c') << kv.first;
        });
    else
        dump_graph("nfa", nfa->is_reversed, nfa->nodes, nfa->start, nfa->finish, [](Edge*) {});
    return 0;
}

}  // namespace

int main(int argc, char* argv[]) {
    try {
        if (argc > 1 && std::strcmp(argv[1], "-dump") == 0) return do_dump(argc, argv);
        if (argc > 2 && std::strcmp(argv[1], "-match-mixed") == 0) {
            // diploma -match-mixed FILE...: every file holds a regex (line 1) and strings (one per line); all of them are matched by
            // ONE device call; prints the 0/1 lines of file 1, then of file 2, ...
            // diploma -match-mixed -bnf|-reverse|-ssnf|-all FILE...: each regex goes through compile() as in `-match` with these flags and is
            // whichever kind compile() returns, with or without memory; a file's answers follow the lines compile() prints for it, as in `-match`; without a flag every regex becomes a memory automaton (toMFA)
            bool bnf = false, reverse = false, ssnf = false, compiled = false;
            int first = 2;
            for (; first < argc && argv[first][0] == '-'; first++) {
                const string flag = argv[first];
                if (flag == "-all") bnf = reverse = ssnf = true;
                else if (flag == "-bnf") bnf = true;
                else if (flag == "-reverse") reverse = bnf = true;
                else if (flag == "-ssnf") ssnf = true;
                else { std::cerr << "diploma: -match-mixed: unknown flag " << flag << "\n"; return 1; }
                compiled = true;
            }
            vector<Automata*> automata;
            vector<vector<string>> strs;
            vector<string> headers;                                  // with a flag: what compile() prints for a file goes in front of the file's answers, as in `-match`
            for (int a = first; a < argc; a++) {
                std::ostringstream sink;
                std::ifstream f(argv[a]);
                if (!f.is_open()) { cout << "ERROR\n"; return 1; }
                string regex, line;
                std::getline(f, regex);
                std::streambuf* old = cout.rdbuf(sink.rdbuf());      // compile() prints its header lines
                Regexp* re = Regexp::parse_regexp(regex);
                if (compiled) {
                    bool is_mfa = false;
                    automata.push_back(re->compile(is_mfa, reverse, bnf, ssnf));
                } else {
                    re->is_backref_correct();
                    automata.push_back(re->to_binary_tree()->toMFA());
                }
                cout.rdbuf(old);
                headers.push_back(compiled ? sink.str() : string());
                strs.emplace_back();
                while (std::getline(f, line)) strs.back().push_back(line);
            }
            const vector<vector<bool>> results = match_mixed(automata, strs);
            for (size_t k = 0; k < results.size(); k++) {
                cout << headers[k];
                for (bool b : results[k]) cout << (b ? 1 : 0) << "\n";
            }
            return 0;
        }
        if (argc > 3 && std::strcmp(argv[1], "-match-file") == 0) {
            string regex;
            cin >> regex;
            if (std::strcmp(argv[2], "gt") == 0) match_gt(regex, argv[3]); else match_mfa(regex, argv[3]);
            return 0;
        }
        if (argc > 2 && std::strcmp(argv[1], "-match-blocks") == 0) {
            // text that arrives in blocks: compile() as in `-match`, then every token goes through an Automata::Stream in blocks of N bytes,
            // in the order the automaton scans (a reversed one is fed the token's last block first); one 0/1 line per token
            const size_t block = (size_t)std::strtoull(argv[2], nullptr, 10);
            if (block == 0) { std::cerr << "diploma: -match-blocks: block size?\n"; return 1; }
            set<string> flags;
            for (int i = 3; i < argc; i++) flags.insert(argv[i]);
            const bool all = flags.count("-all") != 0, reverse = all || flags.count("-reverse"), bnf = reverse || flags.count("-bnf"), ssnf = all || flags.count("-ssnf");
            string regex, text;
            cin >> regex;
            bool is_mfa = false;
            Automata* automata = Regexp::parse_regexp(regex)->compile(is_mfa, reverse, bnf, ssnf, false);
            if (is_mfa) { std::cerr << "diploma: -match-blocks: the regex needs memory; only a memory-less automaton carries its state from block to block\n"; return 1; }
            Automata::Stream stream(*automata);
            while (cin >> text && text != "exit") {
                stream.reset();
                const size_t n_blocks = (text.size() + block - 1) / block;
                for (size_t k = 0; k < n_blocks; k++) {
                    const size_t j = automata->is_reversed ? n_blocks - 1 - k : k;
                    stream.feed(text.substr(j * block, block));
                }
                cout << (stream.accepted() ? 1 : 0) << endl;
            }
            return 0;
        }
        if (argc > 1 && std::strcmp(argv[1], "-match-lines") == 0) {
            // the lines of FILE as `-match` answers tokens: compile() prints its header lines, then one 0/1 line per line of the file; the file
            // goes to the device whole and is cut into lines there
            if (argc < 3) { std::cerr << "diploma: -match-lines: which file?\n"; return 1; }
            bool bnf = false, reverse = false, ssnf = false;
            for (int i = 3; i < argc; i++) {
                const string flag = argv[i];
                if (flag == "-all") bnf = reverse = ssnf = true;
                else if (flag == "-bnf") bnf = true;
                else if (flag == "-reverse") reverse = bnf = true;
                else if (flag == "-ssnf") ssnf = true;
                else { std::cerr << "diploma: -match-lines: unknown flag " << flag << "\n"; return 1; }
            }
            string regex;
            cin >> regex;
            if (!match_lines(regex, argv[2], reverse, bnf, ssnf)) { cout << "ERROR\n"; return 1; }
            return 0;
        }
        if (argc > 1 && std::strcmp(argv[1], "-grep-lines") == 0) {
            // what `-match-lines` prints before its answers, then the lines of FILE it would answer 1 (-v: 0), each followed by a newline; the
            // file goes to the device whole and only the kept lines come back
            if (argc < 3) { std::cerr << "diploma: -grep-lines: which file?\n"; return 1; }
            bool bnf = false, reverse = false, ssnf = false, invert = false;
            for (int i = 3; i < argc; i++) {
                const string flag = argv[i];
                if (flag == "-all") bnf = reverse = ssnf = true;
                else if (flag == "-bnf") bnf = true;
                else if (flag == "-reverse") reverse = bnf = true;
                else if (flag == "-ssnf") ssnf = true;
                else if (flag == "-v") invert = true;
                else { std::cerr << "diploma: -grep-lines: unknown flag " << flag << "\n"; return 1; }
            }
            string regex;
            cin >> regex;
            uint64_t unanswered = 0;
            if (!grep_lines(regex, argv[2], invert, reverse, bnf, ssnf, &unanswered)) { cout << "ERROR\n"; return 1; }
            if (unanswered) { std::cerr << "diploma: -grep-lines: " << unanswered << " lines were not answered\n"; return 2; }
            return 0;
        }
        if (argc > 1 && std::strcmp(argv[1], "-search-lines") == 0) {
            // what `-match-lines` prints before its answers, then the lines of FILE that CONTAIN a match of the regex (-v: that contain none),
            // each followed by a newline: `grep` where `-grep-lines` is `grep -x`.  -o: instead, the leftmost-longest match of every line that
            // has one, one match per output line.  Unlike `grep -o` that is ONE match per line, not every non-overlapping one, and a line
            // whose match is empty prints an empty line.  For a regex that compiles to a tabulated memory-less automaton of at most 127 state
            // sets; anything else ends with the library's message and exit status 1.
            if (argc < 3) { std::cerr << "diploma: -search-lines: which file?\n"; return 1; }
            bool bnf = false, reverse = false, ssnf = false, invert = false, only_matching = false;
            for (int i = 3; i < argc; i++) {
                const string flag = argv[i];
                if (flag == "-all") bnf = reverse = ssnf = true;
                else if (flag == "-bnf") bnf = true;
                else if (flag == "-reverse") reverse = bnf = true;
                else if (flag == "-ssnf") ssnf = true;
                else if (flag == "-v") invert = true;
                else if (flag == "-o") only_matching = true;
                else { std::cerr << "diploma: -search-lines: unknown flag " << flag << "\n"; return 1; }
            }
            if (invert && only_matching) { std::cerr << "diploma: -search-lines: -v and -o exclude each other\n"; return 1; }
            string regex;
            cin >> regex;
            uint64_t unanswered = 0;
            if (!search_lines(regex, argv[2], invert, only_matching, reverse, bnf, ssnf, &unanswered)) { cout << "ERROR\n"; return 1; }
            if (unanswered) { std::cerr << "diploma: -search-lines: " << unanswered << " lines were not answered\n"; return 2; }
            return 0;
        }
        if (argc > 1 && std::strcmp(argv[1], "-match") == 0) {
            if (argc > 2 && argv[2][0] != '-') {
                run_configuration_examples(argv[2]);      // main.cpp:11-13: growth curve of test/example_N
                return 0;
            }
            bool bnf = false, reverse = false, ssnf = false, use_log = false;
            set<string> flags;
            for (int i = 2; i < argc; i++) flags.insert(argv[i]);
            if (argc > 2 && std::strcmp(argv[2], "-all") == 0) bnf = reverse = ssnf = true;      // main.cpp:25-29
            if (flags.count("-bnf")) bnf = true;
            if (flags.count("-reverse")) reverse = bnf = true;
            if (flags.count("-ssnf")) ssnf = true;
            if (flags.count("-log")) use_log = true;
            string regex;
            cin >> regex;
            match(regex, reverse, bnf, ssnf, use_log);
            return 0;
        }
        // main.cpp:50-85: no mode flag -> one regex token per round: its backreference normal form and the reversal of that.
        // (The reference never leaves this loop: parse_regexp erases the token before it is compared with "exit", and at end of
        // input it spins.  Here `exit` and end of input end it.)
        const bool use_log = argc > 2 && std::strcmp(argv[2], "-log") == 0;
        string token;
        while (cin >> token && token != "exit") {
            Regexp* regexp = Regexp::parse_regexp(token);
            regexp->is_backref_correct();
            Regexp* normal = regexp->bnf(use_log);
            if (normal->is_bad_bnf) continue;
            cout << "BNF: " << normal->to_string() << endl;
            cout << "Reverse: " << normal->reverse()->to_string() << endl;
        }
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "diploma: " << e.what() << "\n";
        return 1;
    }
}
