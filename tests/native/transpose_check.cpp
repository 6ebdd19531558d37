// Host check of tr32_step (csrc/ldpc_bitplane.h), the exchange the word mode's output kernel
// builds its 32 x 32 bit transpose from: 32 lanes are simulated as an array, every lane takes its
// partner's word of the round before, and after the five rounds lane r must hold bit r of every
// lane's first word.  Random matrices, the unit matrices (one bit each) and every order of the
// rounds the kernel could take.  Built and run by tests/test_word_transpose.py (g++).  Prints
// "ok <cases>" or the first mismatches; exit status 1 on any.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#define LDPC_BP_FN inline
#define LDPC_BITOP3(a, b, c, F) 0u
#include "ldpc_bitplane.h"

using ldpc::bs::tr32_step;

static long g_bad = 0, g_cases = 0;

static void transpose(const uint32_t (&a)[32], const int (&order)[5], uint32_t (&out)[32]) {
    uint32_t x[32], y[32];
    for (int i = 0; i < 32; ++i) x[i] = a[i];
    for (const int j : order) {
        for (int i = 0; i < 32; ++i) y[i] = tr32_step(x[i], x[i ^ j], j, (i & j) != 0);
        for (int i = 0; i < 32; ++i) x[i] = y[i];
    }
    for (int i = 0; i < 32; ++i) out[i] = x[i];
}

static void check(const uint32_t (&a)[32], const int (&order)[5]) {
    uint32_t t[32];
    transpose(a, order, t);
    ++g_cases;
    for (int r = 0; r < 32; ++r)
        for (int c = 0; c < 32; ++c)
            if (((t[r] >> c) & 1u) != ((a[c] >> r) & 1u)) {
                if (g_bad++ < 8) std::printf("order %d..: out[%d] bit %d wrong\n", order[0], r, c);
                return;
            }
}

int main() {
    int order[5] = {1, 2, 4, 8, 16};
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    do {
        uint32_t a[32];
        for (int n = 0; n < 8; ++n) {
            for (int i = 0; i < 32; ++i) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                a[i] = (uint32_t)(rng >> 32);
            }
            check(a, order);
        }
    } while (std::next_permutation(order, order + 5));
    const int kernel_order[5] = {16, 8, 4, 2, 1};
    for (int i = 0; i < 32; ++i)
        for (int c = 0; c < 32; ++c) {
            uint32_t a[32] = {};
            a[i] = 1u << c;
            check(a, kernel_order);
        }
    if (g_bad) return 1;
    std::printf("ok %ld\n", g_cases);
    return 0;
}
