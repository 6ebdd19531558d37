// The int8-LLR conversion of csrc/ldpc_bitplane.h (l8_bytes, l8_invalid) on the host: prints what
// the functions return, tests/test_llr8_convert.py compares it with the format's statement.
//   bytes: for qmax in {15, 7, 3}, big in {0, 1}, lane 0..3, byte 0..255 (the other lanes hold
//          the valid byte 0): "qmax big lane byte out invalid" -- the lane's output byte and flag,
//          and "other" on a line of its own if another lane's output or flag moved
//   mask:  for valid4 0..15 and every set of invalid lanes 0..15: "valid4 lanes result"
#include <cstdint>
#include <cstdio>
#include <cstring>

#define LDPC_BP_FN static inline
#define LDPC_BITOP3(a, b, c, F) 0u
#include "ldpc_bitplane.h"

using namespace ldpc::bs;

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "mask")) {
        for (uint32_t valid4 = 0; valid4 < 16; ++valid4)
            for (uint32_t lanes = 0; lanes < 16; ++lanes) {
                uint32_t w = 0;
                for (int l = 0; l < 4; ++l)
                    if ((lanes >> l) & 1) w |= 0x40u << (8 * l);         // 64: invalid on every grid
                uint32_t inv;
                (void)l8_bytes(w, 15, true, inv);
                std::printf("%u %u %u\n", valid4, lanes, l8_invalid(inv, valid4) != 0u ? 1u : 0u);
            }
        return 0;
    }
    const int qmaxs[3] = {15, 7, 3};
    for (int qi = 0; qi < 3; ++qi)
        for (int big = 0; big < 2; ++big)
            for (int lane = 0; lane < 4; ++lane)
                for (uint32_t b = 0; b < 256; ++b) {
                    uint32_t inv;
                    const uint32_t k = l8_bytes(b << (8 * lane), qmaxs[qi], big != 0, inv);
                    std::printf("%d %d %d %u %u %u\n", qmaxs[qi], big, lane, b, (k >> (8 * lane)) & 0xFFu,
                                (inv >> (8 * lane)) & 0xFFu);
                    const uint32_t rest = ~(0xFFu << (8 * lane));
                    if ((k & rest) != (0x10101010u & rest) || (inv & rest) != 0u) std::printf("other\n");
                }
    return 0;
}
