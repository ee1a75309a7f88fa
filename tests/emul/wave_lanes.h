// TEST INFRASTRUCTURE ONLY: the host form of the lane-crossing primitives of csrc/nfa_set_wave_core.h -- a wave is 64 lanes as an array,
// so the rule that header states once runs here on all 64 words of a mask (tests/emul/nfa_set_wave_emul.cpp).  The one-lane shim
// (shim/hip/hip_runtime.h) supplies the HIP names beside it.  Nothing in the product includes this.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace emul {

struct Lanes {
    uint32_t w[64];
};
inline Lanes operator|(const Lanes& a, const Lanes& b) { Lanes r; for (int l = 0; l < 64; l++) r.w[l] = a.w[l] | b.w[l]; return r; }
inline Lanes operator&(const Lanes& a, const Lanes& b) { Lanes r; for (int l = 0; l < 64; l++) r.w[l] = a.w[l] & b.w[l]; return r; }
inline Lanes operator~(const Lanes& a) { Lanes r; for (int l = 0; l < 64; l++) r.w[l] = ~a.w[l]; return r; }

struct WaveHost {
    typedef Lanes Reg;
    static uint32_t uni(uint32_t x) { return x; }
    static Reg zero() { Reg r; memset(&r, 0, sizeof r); return r; }
    static bool any(const Reg& r) {
        for (int l = 0; l < 64; l++) if (r.w[l]) return true;
        return false;
    }
    static uint32_t lowest(const Reg& r) {
        for (uint32_t l = 0; l < 64; l++) if (r.w[l]) return l;
        abort();                                                  // only asked when there is one
    }
    static uint32_t word(const Reg& r, uint32_t k) { if (k >= 64) abort(); return r.w[k]; }
    static void or_bit(Reg& r, uint32_t k, uint32_t bit) { if (k >= 64) abort(); r.w[k] |= bit; }
    // lanes at and beyond W load nothing: a row shorter than the header says is a read a sanitizer sees
    static Reg load_row(const uint32_t* row, uint32_t W) {
        Reg r = zero();
        for (uint32_t l = 0; l < W && l < 64; l++) r.w[l] = row[l];
        return r;
    }
    static uint32_t load_uni(const uint32_t* p) { return *p; }
    static uint32_t load_uni8(const uint8_t* p) { return *p; }
    // lane l loads block l, the lanes at and beyond n_blocks nothing
    static void load_blocks(const uint8_t* bytes, uint64_t first, uint32_t n_blocks, Reg (&d)[4]) {
        if (n_blocks > 64 || (first & 15u)) abort();
        for (int q = 0; q < 4; q++) d[q] = zero();
        for (uint32_t l = 0; l < n_blocks; l++)
            for (int q = 0; q < 4; q++) memcpy(&d[q].w[l], bytes + first + (uint64_t)l * 16u + 4u * (uint32_t)q, 4);
    }
    static void push(uint32_t* stack, uint32_t sp, uint32_t v) { stack[sp] = v; }
    static uint32_t pop(const uint32_t* stack, uint32_t sp) { return stack[sp]; }
};

}  // namespace emul
