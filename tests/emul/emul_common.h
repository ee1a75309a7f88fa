// TEST INFRASTRUCTURE ONLY: what the harnesses of this folder do before they reach the code under test -- read a file, load a memory-less
// image, build its fused table the way the kernels do, and give a batch exactly the room the library's read rule makes readable -- and what
// the set-walk harnesses (nfa_set*_emul.cpp) share besides: the exit for a difference, lists on the command line, records, rounds of pieces.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mfa_internal.h"

namespace emul {

inline std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}

// the image of a blob file, tabulated; anything but a memory-less automaton ends the harness with exit code 2
inline void load_memoryless(const char* path, mfa::HostImage& img) {
    const std::vector<uint8_t> blob = slurp(path);
    if (mfa::parse_blob(blob.data(), blob.size(), img) != MFA_OK || img.h.kind != MFA_KIND_NFA || mfa::tabulate_nfa(img) != MFA_OK) {
        fprintf(stderr, "%s: not a memory-less image\n", path);
        exit(2);
    }
}

// the fused table as every kernel builds it in LDS: dfa_fill_table on the 16-bit transitions the library uploads (capi.hip)
inline std::vector<uint16_t> fused_table(const mfa::HostImage& img) {
    if (img.dfa_states > 127) { fprintf(stderr, "table does not fit LDS\n"); exit(2); }
    const std::vector<uint16_t> trans(img.dfa_trans.begin(), img.dfa_trans.end());
    std::vector<uint16_t> next((size_t)img.dfa_states * mfa::kDfaRow, 0);
    mfa::dfa_fill_table(next.data(), trans.data(), img.byte_class, img.dfa_states, img.n_classes, 0u, 1u);
    return next;
}

// `total` bytes of strings in exactly the room include/mfa_hip.h makes readable: whole 16-byte blocks (at least one), 16-byte aligned,
// zero behind the strings, and not a byte more -- so that a host sanitizer sees a read beyond the rule.  The caller frees it.
inline uint8_t* padded(const uint8_t* src, size_t total) {
    const size_t room = total ? (total + 15) & ~(size_t)15 : 16;
    uint8_t* bytes = (uint8_t*)aligned_alloc(16, room);
    memset(bytes, 0, room);
    memcpy(bytes, src, total);
    return bytes;
}

// BATCH.bin: u64 n, u64 offsets[n + 1], then offsets[n] bytes
struct Batch {
    std::vector<uint64_t> off;
    uint8_t* bytes;                                                           // padded(); the caller frees it
};

inline Batch read_batch(const std::vector<uint8_t>& file) {
    uint64_t n;
    memcpy(&n, file.data(), 8);
    Batch b{std::vector<uint64_t>(n + 1), nullptr};
    memcpy(b.off.data(), file.data() + 8, (n + 1) * 8);
    b.bytes = padded(file.data() + 8 + (n + 1) * 8, (size_t)b.off[n]);
    return b;
}

// a difference the harness was built to find: exit code 5
[[noreturn]] inline void fail(const char* what) { fprintf(stderr, "%s\n", what); exit(5); }

// "16,32,64" -> the numbers
inline std::vector<uint64_t> list_of(const char* arg) {
    std::vector<uint64_t> out;
    for (const char* p = arg; *p;) {
        char* end = nullptr;
        out.push_back(strtoull(p, &end, 10));
        if (end == p) { fprintf(stderr, "bad list %s\n", arg); exit(2); }
        p = *end == ',' ? end + 1 : end;
    }
    return out;
}

// n records of `words` u32 in exactly n * words * 4 bytes, 16-byte aligned (at least one record's room, so that n == 0 allocates
// something), every byte `fill`: 0 for records at their start, 0xa5 for ones that must be written before they are read.  The caller frees them.
inline uint32_t* new_records(uint64_t n, uint32_t words, int fill) {
    const size_t bytes = (size_t)(n ? n : 1) * words * 4u;
    uint32_t* rec = (uint32_t*)aligned_alloc(16, bytes);
    memset(rec, fill, bytes);
    return rec;
}

// ROUND.bin: one round of pieces as one call gets it -- u64 n, u64 total, u64 offsets[n + 1], then `total` bytes
struct Round {
    std::vector<uint64_t> off;                                                // piece k is [off[k], off[k + 1]) and may lie outside the bytes
    uint8_t* bytes;                                                           // padded(); the caller frees it
};

// the round of a file; n: the pieces of the rounds before it (first: there is none, and n is set).  A file that does not fit itself or
// the rounds before it, or offsets that go down, end the harness with exit code 2
inline Round read_round(const char* path, bool first, uint64_t& n) {
    const std::vector<uint8_t> file = slurp(path);
    uint64_t n_here, total;
    if (file.size() < 16) { fprintf(stderr, "%s: not a round\n", path); exit(2); }
    memcpy(&n_here, file.data(), 8); memcpy(&total, file.data() + 8, 8);
    if (file.size() != 16 + (n_here + 1) * 8 + total || (!first && n_here != n)) { fprintf(stderr, "%s: does not fit the batch\n", path); exit(2); }
    n = n_here;
    Round r{std::vector<uint64_t>(n + 1), nullptr};
    memcpy(r.off.data(), file.data() + 16, (n + 1) * 8);
    for (uint64_t k = 0; k < n; k++)
        if (r.off[k + 1] < r.off[k]) { fprintf(stderr, "%s, string %llu: offsets go down\n", path, (unsigned long long)k); exit(2); }
    r.bytes = padded(file.data() + 16 + (n + 1) * 8, (size_t)total);
    return r;
}

}  // namespace emul
