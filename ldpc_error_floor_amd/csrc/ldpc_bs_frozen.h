// ldpc_bs_frozen.h — the pack geometry of the bit-sliced kernel (k_bs, ldpc_bs_kernel.h) as
// compile-time constants: the geometry-frozen builds (template parameter FZ) of kBsInst[0] for the
// wman N576 R3/4 z = 24 graph, DESIGN 3.3.  Every other build reads these values from its kernel
// arguments.
//
// What bs_plan / slot_layout compute for a graph is the same at every call; read from the
// arguments inside the pack loop, each such value is a scalar load and a wait that also drains the
// LDS reads in flight, or a register held (and spilled) through the T loop.  The frozen builds take
// the values below as literals instead.  The host (ldpc_bs.hip, bs_frozen_fit) launches a frozen
// build only when the plan it computed equals every constant here, field by field, so a change of
// the layout code switches the fast path off loudly (tests/test_bs_frozen.py), never silently
// wrong.
#pragma once
#include <cstdint>

namespace ldpc {
namespace bs {

// wman N576 R3/4, z = 24 (24 x 6 proto graph, row degrees 14 / 15), kBsInst[0] {D 15, DV 6, LPC 4},
// one alpha and one beta per iteration.  The slot region is slot_layout's (stride A = 104 slots,
// rows 408 slots apart); RED holds the frame-error words of up to T_CAP iterations, and the tables
// and per-lane words follow it where plan_inst puts them for T_CAP - 3 .. T_CAP iterations.
struct BsFrozenWman {
    static constexpr int inst = 0;               // the kBsInst entry the geometry belongs to
    static constexpr int n_vars = 576, n_checks = 144, z = 24, N = 24;
    static constexpr int btid_n = N;             // columns of the channel-table id rows
    static constexpr int cn_lanes = 576, cn_dmin = 14;
    static constexpr int NT = 576, nw = 9;       // workgroup size, waves
    static constexpr int arows = 1, bcols = 1;
    static constexpr int AL = 64, BL = 68;       // words of one iteration's alpha / beta tables
    static constexpr uint32_t cstride = 480;     // the check lane's slot stride: z slots, bytes
    static constexpr uint32_t off_slots = 0, off_pad = 48480, off_zero = 48500, off_red = 48528,
                              off_alut = 48800, off_blut = 49312, off_ch = 49856;
    static constexpr uint32_t lds = 52160;       // dynamic LDS bytes
    static constexpr int T_CAP = 20;             // iterations the RED region has words for
};

// how many fields bs_frozen_fields / bs_plan_fields (ldpc_bs.hip) report: all of the above but
// btid_n (= N) and T_CAP
constexpr int kBsFrozenFields = 22;

}  // namespace bs
}  // namespace ldpc
