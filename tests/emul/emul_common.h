// TEST INFRASTRUCTURE ONLY: what the harnesses of this folder do before they reach the code under test -- read a file, load a memory-less
// image, build its fused table the way the kernels do, and give a batch exactly the room the library's read rule makes readable.
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

}  // namespace emul
