// TEST INFRASTRUCTURE ONLY: what libstdc++ itself makes of a text -- `cin >> s` up to the stop token, or getline -- for
// tests/test_text_split_cpu.py to hold the splitting rule against.   iostream_split tokens [STOP] | lines  < TEXT > u64 n, then (u64 len, bytes) per string
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "", stop = argc > 2 ? argv[2] : "";
    std::vector<std::string> out;
    std::string s;
    if (mode == "tokens") while (std::cin >> s && (stop.empty() || s != stop)) out.push_back(s);
    else if (mode == "lines") while (std::getline(std::cin, s)) out.push_back(s);
    else return 2;
    const uint64_t n = out.size();
    fwrite(&n, 8, 1, stdout);
    for (const std::string& t : out) {
        const uint64_t len = t.size();
        fwrite(&len, 8, 1, stdout);
        fwrite(t.data(), 1, t.size(), stdout);
    }
    return 0;
}
