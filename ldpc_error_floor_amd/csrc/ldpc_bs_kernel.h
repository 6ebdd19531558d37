// ldpc_bs_kernel.h — bit-sliced fused QMS decoder ("bsl"): 32 codewords per 32-bit word.
//
// Same semantics as the v5 kernel (ldpc_fused5_kernel.h) and the reference graph
// (Main_Functions.py:157-335): all T flooding iterations of a block in one launch, integer
// arithmetic in units of the q-bit grid (q = 5 / -5: qmax = 15).  What changes is the data
// layout: a workgroup decodes one PACK of 32 codewords and every quantity is held as bit
// planes (plane word p of a value holds bit p of that value for the 32 codewords, bit r =
// codeword b0 + r).  The min-sum arithmetic — V->C subtraction, |.| with saturation, the
// two-minimum search, the sign parity, the weighted quantization (a 16-entry table per
// iteration, evaluated as a mux tree) and the variable-node sums — is boolean algebra on whole
// words, which gfx950 issues as v_bitop3_b32 (any function of three words in one VALU op).
// One lane does the work of 32 codeword-lanes of v5.
//
// LDS holds one 5-word SLOT per lifted edge:
//   between the variable and the check phase: V->C = clamp(Tv - C->V, +-15), as a negative flag
//     and 4 magnitude planes (the nudged zero is positive, Main_Functions.py:229-230);
//   between the check and the variable phase: C->V, as a negative flag and 4 magnitude planes.
// Each slot is read and then rewritten by exactly one lane per phase, so the two share it.
// Check phase: LPC lanes per check (padding edges read the all-ones PAD slot: negative,
// magnitude 15, so they change neither minimum nor parity).  Variable phase: one lane per
// variable (variables ordered by degree so a wave's loop bound is tight; padding edges read the
// all-zero ZERO slot); the channel stays in the lane's registers for the whole decode.
//
// Instances (kBsInst): the small graphs (wman, all variables and check lanes of a pack in one
// <= 16-wave workgroup, 16-bit packed slot addresses, 64 VGPRs: three workgroups per CU) and
// the large ones (5G BG2: VPL variables and CPL check groups per lane, 32-bit addresses, one
// 16-wave workgroup per CU), with or without UCN (Main_Functions.py:180-209: the syndrome of the
// previous hard decisions selects alpha' on unsatisfied checks) and shortened bits (LLR = the
// clip value, off the quantizer grid: Q(ch) = +-15, |Q(beta ch)| from a per-column table).
// Packs with any other LLR off the quantizer grid are flagged in `bad` and decoded by the v5
// kernel instead, so the result is exact for any input.
#pragma once
#include <type_traits>
#include <cstdint>

#include "ldpc_beta_tabs.h"
#include "ldpc_fused.h"
#include "ldpc_fused5_kernel.h"
#include "ldpc_bitplane.h"
#include "ldpc_bs_frozen.h"

namespace ldpc {
namespace bs {

constexpr int PACK = 32;                 // codewords per workgroup
constexpr int SLOT_W = 5;                // words per edge slot: negative flag, magnitude 0..3
constexpr int SLOT_B = SLOT_W * 4;
constexpr int LUT_W = 64;                // words per 16-entry table: [bit j][pair p] {X, Y}
constexpr int BLUT_W = LUT_W + 4;        // beta tables: + |Q(beta clip)| planes (shortened bits)
constexpr int QMAX = 15;
constexpr size_t BS_LDS_MAX = 160 * 1024;

// kernel instances: D = check-degree bound, DV = variable-degree bound, LPC = lanes per check,
// VPL / CPL = variables / 64-lane check chunks per lane, UCN / BIG = unsatisfied-check weights /
// shortened bits supported, PK = 16-bit packed slot addresses, WPE = waves per SIMD (registers).
// The multi-chunk instances (VPL / CPL > 1) run 16 waves.
// ES: an early-stop-only instance: its builds carry the syndrome stop rule, and
// bs_plan takes it for early-stop requests and never otherwise.
struct BsInst { int D, DV, LPC, VPL, CPL; bool UCN, BIG, PK; int WPE; bool ES = false; };
constexpr BsInst kBsInst[] = {
    {15, 6, 4, 1, 1, false, false, true, 8},     // wman (C2), LPC 4 measured 6.31 ms vs 6.73
    {16, 8, 4, 1, 1, false, false, true, 8},
    {15, 6, 2, 1, 1, false, false, true, 8},     // LDPC_BS_LPC=2 A/B
    {24, 4, 4, 1, 1, true, true, true, 6},       // 802.11n (C3): degree 22, UCN
    {10, 8, 2, 2, 2, false, true, false, 4},     // 5G BG2 without UCN weighting (C4's trained
                                                 // alpha' = alpha folds to it)
    {10, 8, 2, 2, 2, true, true, false, 4},      // 5G BG2 (C4): 1,280 variables, 640 checks;
                                                 // 18.2 ms vs 21.2 for LPC 4 (CPL 3), same box
    {10, 8, 4, 2, 3, true, true, false, 4},      // LDPC_BS_LPC=4 A/B
    {15, 6, 4, 1, 1, true, false, true, 6, true},   // wman, early stop (UCN-compiled: HD / syndromes)
    {24, 4, 4, 1, 1, true, true, true, 6, true},    // 802.11n, early stop
    {15, 6, 4, 1, 1, true, false, true, 6},      // wman with alpha' != alpha (the boosting cascade):
                                                 // last, and planned for UCN requests only (bs_plan)
};
constexpr int kBsNInst = sizeof(kBsInst) / sizeof(kBsInst[0]);
// The one-chunk UCN instance of wman's geometry for decodes without early stop (the decode, the
// in-prologue channel and the export / word builds; no pack loop, no frozen build).  It has the
// degree bounds of entry 0, which comes first and serves every request without alpha', so bs_plan
// considers it for requests with UCN weights alone, after every other entry: a request that had a
// plan before this entry keeps that plan.
constexpr int kBsInstUcn1 = 9;
static_assert(kBsInstUcn1 == kBsNInst - 1 && kBsInst[kBsInstUcn1].UCN && !kBsInst[kBsInstUcn1].ES &&
              kBsInst[kBsInstUcn1].VPL == 1 && kBsInst[kBsInstUcn1].CPL == 1 && kBsInst[kBsInstUcn1].PK,
              "the one-chunk UCN instance is the table's last entry");

// The QMS channel generated in the kernel's prologue (Q8 builds; ldpc_decode_awgn, SURVEY 8 f
// rank 1): the byte each LLR would have on the q-bit grid (level + 16 + kmin), from the same
// Philox stream and level sampler as ldpc_channel_awgn (ldpc_awgn.h), so the decode is
// bit-identical to ldpc_channel_awgn + ldpc_decode.  The sampler's tables (awgn_gen_table,
// 8.25 KB) are copied into LDS at `lds`, a region the kernel writes only after the prologue.
struct BsGen {
    const uint32_t* tab;         // [AWGN_TAB_W] (awgn_gen_table)
    uint32_t k0, k1;             // Philox key (the seed)
    int64_t offset;              // global index of the batch's first codeword
    int nb, kmin;                // level count - 1, grid index of level 0
    int ps, pe, ss, se;          // 1-based puncture / shorten ranges (0: none)
    uint32_t lds;                // LDS byte address of the tables
};

struct BsArgs {
    const float* llr;            // (Q8 builds: unused, the channel is generated: gen)
    int64_t B;
    int n_vars, n_checks, T, target_bits, cn_lanes, cn_dmin;
    float inv;
    float cu;                    // |LLR| / step of a shortened bit (BIG instances), > qmax
    int qmax;                    // the grid's largest magnitude in grid units (15, 7 or 3)
    int ucn;                     // UCN weights present (UCN instances)
    uint64_t beta_id;            // bit t: iteration t's channel table is the identity (skipped)
    const int32_t* row_ptr;      // [M + 1] proto edges of each row (the check degrees)
    const int32_t* row_lay;      // [M][2] slot layout of each proto row: first slot, j-block stride
    int z;
    const uint32_t* vn_tab;      // [VPL][64 nw][VNW]: slot byte addresses (2 per word if PK), variable (-1 idle)
    const int32_t* vn_wdeg;      // [VPL][nw][3] most and fewest edges of a variable of each wave,
                                 // the chunk's column when it has one (else -1)
    const int32_t* cn_chunk;     // [nw][CPL] 64-lane check chunk of each wave's group (-1 idle)
    const uint32_t* cn_hd;       // [chunks * 64][HDW] UCN: LDS byte addresses of the edges' hard decisions
                                 // (the pack loop's units, which have no UCN: the ticket word, zero at
                                 // the launch, or null: packs by fixed stride -- BS_RED_NEXT)
    const uint32_t* alut;        // [T][AR][LUT_W]: Q(relu(alpha m step)) for m = 0..15 (AR = arows, x2 with UCN)
    const uint32_t* blut;        // [T][bcols][BLUT_W]: |Q(beta m)| for m = 0..15 (grid units), |Q(beta cu)|
    int arows, bcols;
    const int32_t* btid;        // [T][btid_n] kBetaTab index of each column's channel table
    int btid_n;                  // (-1: evaluate from the table words), or null
    int64_t* counters;
    uint8_t* flags;
    uint32_t* bad;               // [packs] 1: decoded by the v5 fixup instead
    uint32_t* iter_wrong;        // [T][packs] per-iteration frame-error words, or null
    int stagger, stagger_n;      // start offsets of workgroups 0 .. stagger_n - 1 (the first
                                 // generation, one per CU), spread over 0 .. stagger x 512 clocks
    uint32_t* hdx;               // XP builds: [T][packs][n_vars] hard decisions (bit r = codeword
                                 // 32 pack + r), the hard-bit / syndrome export
    uint32_t off_slots, off_pad, off_zero, off_red, off_alut, off_blut, off_hdz;   // LDS byte offsets
    uint32_t fold_wave;          // (one-chunk instances) the wave that folds the frame-error
                                 // words in the T loop: the last wave where it holds no check
                                 // lanes, else wave 1 (bs_run)
    uint32_t off_ch;             // per-lane LDS words (one-chunk instances): the check lane's
                                 // slot base (| alpha-table address << 16), [lane]
                                 // (RED: 16 words, then T words: iteration t's frame-error word)
    int ablate;   // timing diagnostics, builds with -DBS_DIAG only (LDPC_DIAG_ABLATE, wrong
                  // results): 1 no check phase, 2 no beta table, 4 no V->C pass, 8 no frame
                  // flags, 16 no iterations, 32 no LLR loads.  (Compiled in, the uniform
                  // tests alone cost 4 %.)
    uint64_t ucn_iter;           // bit t (t < 64): iteration t's alpha' differs from alpha (its
                                 // check phase needs the syndromes); iterations >= 64: on
    uint32_t off_hdl;            // (one-chunk UCN instances) the check lanes' packed
                                 // hard-decision addresses, [HDW][lane] words
    BsGen gen;                   // Q8 builds: the in-prologue channel
    unsigned long long* stamps;  // -DBS_STAMP builds only: [16 waves][16] shader-clock sums per
                                 // phase (0 check, 1 check barrier, 2 variable, 3 variable barrier,
                                 // 4 prologue's check setup, 5 epilogue, 8 entry, 9 channel, 10 its
                                 // barrier, 11 tables, 12 first variable phase; 15 packs), timing
                                 // diagnostics; then one record of BS_WG_REC words per workgroup
};
constexpr int BS_WG_BASE = 256, BS_WG_REC = 8;   // (the stamp builds' per-workgroup records)

// The early-stop builds' arguments (ES instances): BsArgs and what the mode adds, so the other
// builds' kernel arguments stay as they are.
struct BsArgsEs : BsArgs {
    uint8_t* n_iter;             // [B] iterations run per codeword (0: pack off the grid), or null
    int64_t* iter_hist;          // [T] += codewords with n_iter = t + 1, or null
    // (LDS: the T syndrome words follow the FLORW words of the RED region, RED[flor + FLORW + t]:
    // word t = OR over the checks of the syndrome of iteration t's hard decisions)
};

// The arguments of the early-stop builds that keep the decoded word (EW): BsArgsEs and
// the plane buffer, so the ES builds' kernel arguments stay as they are.
struct BsArgsEw : BsArgsEs {
    uint32_t* hdw;               // [packs][n_vars] each codeword's hard decisions at its stop
                                 // iteration (bit r = codeword 32 pack + r), or null: off
};

// The export builds' arguments (XP): BsArgs and the word mode's switch, carried the
// same way.
struct BsArgsXp : BsArgs {
    int word;                    // 1: hdx is [packs][n_vars] and takes the last iteration's hard
                                 // decisions alone (ldpc_decode_word); 0: every iteration's
};

// the kernel's own arguments read from the kernel-argument segment (scalar loads): how the
// early-stop statements reach their fields, also where the pack loop's units rename `a`
template <class A>
__device__ __forceinline__ const __attribute__((address_space(4))) A& kern_args() {
    return *(const __attribute__((address_space(4))) A*)__builtin_amdgcn_kernarg_segment_ptr();
}

// bit-plane arithmetic (B3, the truth tables, add_b / set_b / sub_tv / abs_sat / lt4 / clamp6):
// ldpc_bitplane.h
// LDS accesses by byte address (all slots and tables are LDS-absolute: the kernel's dynamic
// LDS starts at 0, checked at entry)
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) uint32_t LdsW;
typedef __attribute__((address_space(3))) v4u LdsQ;

__device__ __forceinline__ uint32_t lds_w(uint32_t addr) { return *reinterpret_cast<const LdsW*>(addr); }
__device__ __forceinline__ v4u lds_q(uint32_t addr) { return *reinterpret_cast<const LdsQ*>(addr); }
__device__ __forceinline__ void lds_put(uint32_t addr, uint32_t x) { *reinterpret_cast<LdsW*>(addr) = x; }

__device__ __forceinline__ void read_slot(uint32_t& n, uint32_t (&M)[4], uint32_t addr) {
    const LdsW* p = reinterpret_cast<const LdsW*>(addr);
    n = p[0];
    M[0] = p[1];
    M[1] = p[2];
    M[2] = p[3];
    M[3] = p[4];
}
__device__ __forceinline__ void write_slot(uint32_t addr, uint32_t n, const uint32_t (&M)[4]) {
    LdsW* p = reinterpret_cast<LdsW*>(addr);
    p[0] = n;
    p[1] = M[0];
    p[2] = M[1];
    p[3] = M[2];
    p[4] = M[3];
}

// 16-entry table g(m) (4 -> 4 bits) at LDS byte address `tab`: level 1 of the mux tree is
// (m0 & X) ^ Y per pair of entries, levels 2-4 select by m1, m2, m3
template <int NI>
__device__ __forceinline__ void lut(uint32_t (&o)[NI][4], const uint32_t (&in)[NI][4], uint32_t tab) {
    uint32_t tj = tab;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // one output bit at a time (the next bit's table loads wait for this bit's result), so
        // that the scheduler cannot hoist all 16 table loads into 64 registers
        if (j > 0) asm volatile("" : "+v"(tj) : "v"(o[0][j - 1]));
        uint32_t g[NI][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4u w = lds_q(tj + (uint32_t)(j * 64 + q * 16));      // pairs 2q, 2q + 1
#pragma unroll
            for (int u = 0; u < NI; ++u) {
                const uint32_t l0 = B3(T_LEAF, in[u][0], w.x, w.y), l1 = B3(T_LEAF, in[u][0], w.z, w.w);
                g[u][q] = mux(in[u][1], l1, l0);
            }
        }
#pragma unroll
        for (int u = 0; u < NI; ++u)
            o[u][j] = mux(in[u][3], mux(in[u][2], g[u][3], g[u][2]), mux(in[u][2], g[u][1], g[u][0]));
    }
}

// the same 16-entry table when it is one table for the whole workgroup (uniform weights): its
// 64 leaf words come by scalar loads (constant address space) into SGPRs, so the evaluation
// costs no LDS traffic; a leaf is a v_and + v_xor with SGPR operands (the 2-cycle VOP2 forms,
// one SGPR per instruction) in place of one v_bitop3 — the same issue cycles
typedef __attribute__((address_space(4))) const uint32_t ConstW;
// (m & X) ^ Y with X, Y in SGPRs as two VOP2 instructions (the compiler's own form is a v_mov
// of one SGPR plus a v_bitop3 reading the other: the same issue cost, every VALU op with an
// SGPR operand takes ~4.2 cycles against 2.4 for VGPR-only ones; tools/valu_rate.hip)
__device__ __forceinline__ uint32_t leaf_s(uint32_t m, uint32_t X, uint32_t Y) {
    uint32_t t, l;
    asm("v_and_b32 %0, %1, %2" : "=v"(t) : "s"(X), "v"(m));
    asm("v_xor_b32 %0, %1, %2" : "=v"(l) : "s"(Y), "v"(t));
    return l;
}
__device__ __forceinline__ void lut_s(uint32_t (&o)[4], const uint32_t (&a)[4], const ConstW* tab) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t l0 = leaf_s(a[0], tab[j * 16 + 4 * q], tab[j * 16 + 4 * q + 1]);
            const uint32_t l1 = leaf_s(a[0], tab[j * 16 + 4 * q + 2], tab[j * 16 + 4 * q + 3]);
            g[q] = mux(a[1], l1, l0);
        }
        o[j] = mux(a[3], mux(a[2], g[3], g[2]), mux(a[2], g[1], g[0]));
    }
}

// bit j of the table output for NI inputs (4 b128 loads of the table's bit-j leaves at tab_j)
template <int NI>
__device__ __forceinline__ void lut_bit(uint32_t (&o)[NI], const uint32_t (&in)[NI][4], uint32_t tab_j) {
    uint32_t g[NI][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4u w = lds_q(tab_j + (uint32_t)(q * 16));      // pairs 2q, 2q + 1
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const uint32_t l0 = B3(T_LEAF, in[u][0], w.x, w.y), l1 = B3(T_LEAF, in[u][0], w.z, w.w);
            g[u][q] = mux(in[u][1], l1, l0);
        }
    }
#pragma unroll
    for (int u = 0; u < NI; ++u)
        o[u] = mux(in[u][3], mux(in[u][2], g[u][3], g[u][2]), mux(in[u][2], g[u][1], g[u][0]));
}

// n consecutive words src[0..n) to LDS byte address lds (a table for the next iteration),
// global -> LDS without registers (global_load_lds_dword: lane l of the wave whose first word is
// w0 writes word w0 + l).  Nothing waits for the loads here: the next __syncthreads (vmcnt(0))
// retires them, before any wave reads the table.
__device__ __forceinline__ void copy_async(uint32_t lds, const uint32_t* src, int n, int wave, int NT) {
    // (wave-uniform loop; the lane index from mbcnt, so no thread index is kept live for it)
    for (int w0 = wave * 64; w0 < n; w0 += NT) {
        const int w = w0 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        if (w < n)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + w),
                                             (__attribute__((address_space(3))) void*)(uintptr_t)(lds + 4u * (uint32_t)w0),
                                             4, 0, 0);
    }
}

// Fixed-set weight tables (ldpc_beta_tabs.h) by a computed call: the wave-uniform table index k
// selects an entry of a jump table (s_getpc + offset, s_swappc); the entry computes the output
// planes with immediate truth tables (v_bitop3) and returns (s_setpc to s[44:45]).  The table
// follows the call in the instruction stream and the call skips it.  s40-s45 are the call's
// scratch.  The caller keeps k in [0, kNBetaTab).
#define LDPC_TAB_CALL(SH, AL, TABLE)                                                           \
    "s_getpc_b64 s[40:41]\n"                                                                      \
    ".Lbpc%=:\n\t"                                                                                \
    "s_lshl_b32 s42, %[k], " SH "\n\t"                                                           \
    "s_add_u32 s40, s40, s42\n\t"                                                                \
    "s_addc_u32 s41, s41, 0\n\t"                                                                 \
    "s_add_u32 s40, s40, .Lbtab%=-.Lbpc%=\n\t"                                                    \
    "s_addc_u32 s41, s41, 0\n\t"                                                                 \
    "s_swappc_b64 s[44:45], s[40:41]\n\t"                                                        \
    "s_branch .Lbend%=\n"                                                                        \
    "\t.p2align " AL "\n"                                                                        \
    ".Lbtab%=:\n" TABLE ".Lbend%=:\n"

// The channel-weight table |Q(beta_t ch)| (Main_Functions.py:164-177) when beta_t's table is
// table k of the fixed set: each output bit j is mux(m3, f_hi(m2, m1, m0), f_lo(m2, m1, m0))
// with compile-time truth tables, at most three v_bitop3 with immediates, against 16 leaves with
// SGPR operands (4.2-cycle forms) and 7 muxes per bit for a table held in SGPRs.  (A C++ switch
// over the 210 tables, a binary tree of scalar branches with 210 leaves, made the register
// allocator spill 291 VGPRs.)
__device__ __forceinline__ void beta_asm(uint32_t (&o)[4], const uint32_t (&m)[4], int k) {
    uint32_t t0, t1;
    asm volatile(LDPC_TAB_CALL("7", "7", LDPC_BETA_ASM_TABLE)
        : [o0] "=&v"(o[0]), [o1] "=&v"(o[1]), [o2] "=&v"(o[2]), [o3] "=&v"(o[3]),
          [t0] "=&v"(t0), [t1] "=&v"(t1)
        : [m0] "v"(m[0]), [m1] "v"(m[1]), [m2] "v"(m[2]), [m3] "v"(m[3]), [k] "s"(k)
        : "s40", "s41", "s42", "s43", "s44", "s45", "scc");
}

// lane permutation inside each group of 4 lanes (DPP quad_perm, a VALU move).  bound_ctrl on:
// every lane of a quad_perm / row mirror has a source lane, so the "old" operand is dead, and a
// DPP move whose consumer is a VOP2 op folds into it (v_xor_b32_dpp)
template <int CTRL>
__device__ __forceinline__ uint32_t qperm(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
constexpr int QP_X1 = 0xB1;          // [1, 0, 3, 2]
constexpr int QP_X2 = 0x4E;          // [2, 3, 0, 1]

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
// OR / sum over the wave (wave-uniform result): butterflies inside each row of 16 lanes by DPP
// (quad_perm, row_half_mirror, row_mirror), then the four row results by readlane
__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
    x |= dpp<QP_X1>(x);
    x |= dpp<QP_X2>(x);
    x |= dpp<0x141>(x);
    x |= dpp<0x140>(x);
    return (uint32_t)(__builtin_amdgcn_readlane((int)x, 15) | __builtin_amdgcn_readlane((int)x, 31) |
                      __builtin_amdgcn_readlane((int)x, 47) | __builtin_amdgcn_readlane((int)x, 63));
}
__device__ __forceinline__ uint32_t wave_add(uint32_t x) {
    x += dpp<QP_X1>(x);
    x += dpp<QP_X2>(x);
    x += dpp<0x141>(x);
    x += dpp<0x140>(x);
    return (uint32_t)(__builtin_amdgcn_readlane((int)x, 15) + __builtin_amdgcn_readlane((int)x, 31) +
                      __builtin_amdgcn_readlane((int)x, 47) + __builtin_amdgcn_readlane((int)x, 63));
}

// AND over the LPC lanes of a check's group: one v_and_b32_dpp per step.  (Each step's result
// goes through an empty asm, so the two ANDs are not reassociated into one v_bitop3 AND3 — which
// left both DPP moves unfolded: 2 DPP moves + 2 VALU per step pair instead of 2 DPP ANDs.)
template <int LPC>
__device__ __forceinline__ uint32_t grp_and(uint32_t a) {
    a &= qperm<QP_X1>(a);
    asm("" : "+v"(a));
    if (LPC == 4) {
        a &= qperm<QP_X2>(a);
        asm("" : "+v"(a));
    }
    return a;
}
// The check's two minima by a bit-serial search over the whole lane group, most significant
// plane first: plane i of the minimum is the AND over the edges still tied with it on the planes
// above (cand), taken across the group by DPP; cand ends as [|V->C| = m1], the edges that get the
// second minimum in pass 2.  The second minimum is the same search over the other edges, or m1
// where two or more edges tie at it.  (Against the pair tournament and the two lane-group merges:
// C2, 4 edges per lane, 98 VALU with 22 DPP per lane against 117 with 18, and pass 2 no longer
// compares each edge with m1.)  Padding slots (all ones) are magnitude 15: with degree >= 2 they
// change neither minimum.
// (the first K of the EPL slots: the multi-chunk instances skip the positions that are padding
// for the whole chunk, K = gm by a switch)
template <int K, int LPC, int EPL>
__device__ __forceinline__ void min2_bits(uint32_t (&m1)[4], uint32_t (&m2)[4], uint32_t (&cand)[EPL],
                                          const uint32_t (&X)[EPL][4]) {
    static_assert(K >= 1 && K <= EPL, "active slots");
    constexpr unsigned T_ANDORN = (TA & (TB | ~TC)) & 0xFF;      // a & (b | ~c)
    constexpr unsigned T_ANDOR = (TA & (TB | TC)) & 0xFF;        // a & (b | c)
    constexpr unsigned T_ANDEQ = (TA & ~(TB ^ TC)) & 0xFF;       // a & (b == c)
    constexpr unsigned T_NANDEQ = (~TA & ~(TB ^ TC)) & 0xFF;     // ~a & (b == c)
    constexpr unsigned T_ORAND = (TA | (TB & TC)) & 0xFF;        // a | (b & c)
    // m1, most significant plane first
    uint32_t a = X[0][3];
#pragma unroll
    for (int m = 1; m < K; ++m) a &= X[m][3];
    a = grp_and<LPC>(a);
    m1[3] = a;
#pragma unroll
    for (int m = 0; m < K; ++m) cand[m] = ~(X[m][3] ^ a);
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        a = X[0][i] | ~cand[0];
#pragma unroll
        for (int m = 1; m < K; ++m) a = B3(T_ANDORN, a, X[m][i], cand[m]);
        a = grp_and<LPC>(a);
        m1[i] = a;
#pragma unroll
        for (int m = 0; m < K; ++m) cand[m] = B3(T_ANDEQ, cand[m], X[m][i], a);
    }
    // two or more edges of the group at the minimum
    uint32_t one = cand[0], two = 0u;
#pragma unroll
    for (int m = 1; m < K; ++m) {
        two = B3(T_ORAND, two, one, cand[m]);
        one |= cand[m];
    }
    {
        const uint32_t op = qperm<QP_X1>(one);
        two = qperm<QP_X1>(two) | B3(T_ORAND, two, one, op);
        one |= op;
    }
    if (LPC == 4) {
        const uint32_t op = qperm<QP_X2>(one);
        two = qperm<QP_X2>(two) | B3(T_ORAND, two, one, op);
    }
    // the minimum of the other edges (c2: not at m1, tied with the search so far)
    uint32_t c2[K];
    a = X[0][3] | cand[0];
#pragma unroll
    for (int m = 1; m < K; ++m) a = B3(T_ANDOR, a, X[m][3], cand[m]);
    a = grp_and<LPC>(a);
    m2[3] = a;
#pragma unroll
    for (int m = 0; m < K; ++m) c2[m] = B3(T_NANDEQ, cand[m], X[m][3], a);
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        a = X[0][i] | ~c2[0];
#pragma unroll
        for (int m = 1; m < K; ++m) a = B3(T_ANDORN, a, X[m][i], c2[m]);
        a = grp_and<LPC>(a);
        m2[i] = a;
        if (i > 0) {
#pragma unroll
            for (int m = 0; m < K; ++m) c2[m] = B3(T_ANDEQ, c2[m], X[m][i], a);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) m2[i] = mux(two, m1[i], m2[i]);
}

#ifdef BS_DIAG
#define ABL(bit) (a.ablate & (bit))
#else
#define ABL(bit) 0
#endif
// Phase markers for the ISA attribution (tools/isa_phase_table.py), analysis builds only
// (-DBS_MARK: an assembler comment ";@ph NAME.K" at each phase start; the product build has none)
// PH4 / PH8 / PH9 tie the marker to the values the phase starts from ("+v"), so the phase's first
// instructions cannot be scheduled above it
#ifdef BS_MARK
#define PH(name, k) asm volatile(";@ph " name ".%0" ::"i"(k))
#define PH4(name, k, x) asm volatile(";@ph " name ".%4" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]) : "i"(k))
#define PH8(name, k, x, y)                                                                        \
    asm volatile(";@ph " name ".%8" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(y[0]),  \
                 "+v"(y[1]), "+v"(y[2]), "+v"(y[3]) : "i"(k))
#define PH9(name, k, x, y, z)                                                                     \
    asm volatile(";@ph " name ".%9" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(y[0]),  \
                 "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(z) : "i"(k))
#else
#define PH(name, k) ((void)0)
#define PH4(name, k, x) ((void)0)
#define PH8(name, k, x, y) ((void)0)
#define PH9(name, k, x, y, z) ((void)0)
#endif
// The channel planes of one variable for the 32 codewords of a pack: sign cs, magnitude planes
// cm[0..3] of Q(ch) in grid units, shortened-bit flags bg (BIG); returns 1 when a row is off the
// grid (the pack then goes to the v5 fixup).  Per row: x = llr / step, q = clamp(rint(x), +-qmax)
// — on the grid iff q == x, or a shortened bit (|x| == cu, decoded as +-qmax) — and q is stored
// as the byte q + 16 (+ 32 for a shortened bit) by v_cvt_pk_u8_f32, four rows per word.  The 32
// bytes become bit planes by four 8x8 bit-matrix transposes (three delta swaps each) and a 4x4
// byte transpose (v_perm); offset binary q + 16 gives the sign (NOT bit 4) and, bit-sliced, the
// magnitude (the low 4 bits, negated mod 16 where negative).  About 300 VALU per variable against
// ~750 for a per-row insertion of each bit into each plane (2 ops per bit and plane).
// (valid: the pack's codewords; rows past it read 0 and are masked)
__device__ __forceinline__ void t8x8(uint32_t& lo, uint32_t& hi) {
    uint32_t t;
    t = B3((TA ^ TB) & TC, lo, lo >> 7, 0x00AA00AAu);
    lo = B3(T_XOR3, lo, t, t << 7);
    t = B3((TA ^ TB) & TC, hi, hi >> 7, 0x00AA00AAu);
    hi = B3(T_XOR3, hi, t, t << 7);
    t = B3((TA ^ TB) & TC, lo, lo >> 14, 0x0000CCCCu);
    lo = B3(T_XOR3, lo, t, t << 14);
    t = B3((TA ^ TB) & TC, hi, hi >> 14, 0x0000CCCCu);
    hi = B3(T_XOR3, hi, t, t << 14);
    t = B3((TA ^ TB) & TC, lo, hi << 4, 0xF0F0F0F0u);
    lo ^= t;
    hi ^= t >> 4;
}
// the 32 bytes (byte r of D[r / 4]: q + 16, + 32 on a shortened bit) -> sign / magnitude /
// shortened planes
template <bool BIG>
__device__ __forceinline__ void pack_bytes(const uint32_t (&D)[8], uint32_t valid, uint32_t& cs,
                                           uint32_t (&cm)[4], uint32_t& bg) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        lo[g] = D[2 * g];
        hi[g] = D[2 * g + 1];
        t8x8(lo[g], hi[g]);
    }
    // byte p of lo[g] (p < 4) / hi[g] (p >= 4): plane p of rows 8 g .. 8 g + 7
    const uint32_t a = __builtin_amdgcn_perm(lo[1], lo[0], 0x06020400u), b = __builtin_amdgcn_perm(lo[1], lo[0], 0x07030501u);
    const uint32_t c = __builtin_amdgcn_perm(lo[3], lo[2], 0x06020400u), d = __builtin_amdgcn_perm(lo[3], lo[2], 0x07030501u);
    const uint32_t L0 = __builtin_amdgcn_perm(c, a, 0x05040100u) & valid, L2 = __builtin_amdgcn_perm(c, a, 0x07060302u) & valid;
    const uint32_t L1 = __builtin_amdgcn_perm(d, b, 0x05040100u) & valid, L3 = __builtin_amdgcn_perm(d, b, 0x07060302u) & valid;
    const uint32_t e = __builtin_amdgcn_perm(hi[1], hi[0], 0x05010400u), f = __builtin_amdgcn_perm(hi[3], hi[2], 0x05010400u);
    const uint32_t n = ~__builtin_amdgcn_perm(f, e, 0x05040100u) & valid;
    bg = BIG ? (__builtin_amdgcn_perm(f, e, 0x07060302u) & valid) : 0u;
    cs = n;
    cm[0] = L0;
    cm[1] = B3(T_XAND, L1, n, L0);
    cm[2] = B3(T_XAND, L2, n, L0 | L1);
    cm[3] = B3(T_XAND, L3, n, L0 | L1 | L2);
}
template <bool BIG>
__device__ __forceinline__ int pack_channel(const float (&xv)[PACK], float inv, int qmax, float cu,
                                            uint32_t valid, uint32_t& cs, uint32_t (&cm)[4], uint32_t& bg) {
    const float qf = (float)qmax;
    uint32_t D[8];
    int off = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) D[k] = 0u;
#pragma unroll
    for (int r = 0; r < PACK; ++r) {
        const float x = xv[r] * inv;
        const float q = __builtin_amdgcn_fmed3f(rintf(x), -qf, qf);
        const bool big = BIG && fabsf(x) == cu;
        off |= (q != x && !big) ? 1 : 0;
        D[r >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(q + (big ? 48.f : 16.f), r & 3, D[r >> 2]);
    }
    pack_bytes<BIG>(D, valid, cs, cm, bg);
    return off;
}
// The bytes of variable v for the 32 codewords of pack pk, generated (Q8 builds): byte r of
// D[r / 4] = level + 16 + kmin of codeword offset + 32 pk + r (a shortened bit: 48 - qmax, a
// punctured one: 16; oracle/philox_oracle.py awgn_q8).  Four codewords per Philox call; a batch offset
// off the quads takes two quads per word and a byte funnel shift (wave-uniform).
typedef unsigned int v2u_g __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const v2u_g LdsU2;
__device__ __forceinline__ void gen_bytes(const BsGen& g, int64_t pk, int v, int qmax, uint32_t (&D)[8]) {
    const int bit = v + 1;
    if (g.ss > 0 && bit >= g.ss && bit <= g.se) {
#pragma unroll
        for (int i = 0; i < 8; ++i) D[i] = (uint32_t)(48 - qmax) * 0x01010101u;
        return;
    }
    if (g.ps > 0 && bit >= g.ps && bit <= g.pe) {
#pragma unroll
        for (int i = 0; i < 8; ++i) D[i] = 0x10101010u;
        return;
    }
    LdsU2* bucket = reinterpret_cast<LdsU2*>((uintptr_t)g.lds);
    const LdsW* thi = reinterpret_cast<const LdsW*>((uintptr_t)(g.lds + 8u * (1u << AWGN_KB)));
    const LdsW* tlo = thi + AWGN_NB_MAX;
    const uint64_t g0 = (uint64_t)g.offset + (uint64_t)pk * 32u;
    const int sh = (int)(g.offset & 3);
    const uint32_t boff = (uint32_t)(16 + g.kmin);
    auto word = [&](const int (&l)[4]) __attribute__((always_inline)) -> uint32_t {
        return ((uint32_t)l[0] + boff) | ((uint32_t)l[1] + boff) << 8 | ((uint32_t)l[2] + boff) << 16 |
               ((uint32_t)l[3] + boff) << 24;
    };
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t gq = (g0 + 4u * (uint32_t)i) >> 2;
        int la[4];
        awgn_levels4b(g, bucket, thi, tlo, (uint32_t)v, gq, la);
        uint32_t w = word(la);
        if (sh) {
            int lb[4];
            awgn_levels4b(g, bucket, thi, tlo, (uint32_t)v, gq + 1, lb);
            w = __builtin_amdgcn_alignbyte(word(lb), w, (uint32_t)sh);
        }
        D[i] = w;
    }
}
// the generator's tables into LDS (every thread of the workgroup): asynchronous global -> LDS
// copies that the caller's barrier retires by its vmcnt(0), one L2 round trip for all of them
__device__ __forceinline__ void gen_tables(const BsGen& g, int tid, int NT) {
    copy_async(g.lds, g.tab, AWGN_TAB_W, __builtin_amdgcn_readfirstlane(tid >> 6), NT);
}

// first-generation start spread of the one-workgroup-per-CU instances, microseconds (bs_stagger):
// about a pack's duration on 5G BG2 (C4); bsc passes one_per_cu = false and starts at 0
constexpr double STAGGER_US = 60.0;
// the LDS words the variable phases OR their frame-error words into (lane & 31: two lanes per
// word, distinct banks); one wave folds them in the next iteration, before its check barrier
constexpr int FLORW = 32;
// The pack loop: a workgroup of a one-chunk instance without UCN (wman) decodes packs blockIdx.x,
// blockIdx.x + gridDim.x, ... instead of one, on a grid of the workgroups that are resident at
// once (ldpc_bs.hip; LDPC_BS_GRID), so a pack after the first pays no wave launch, no
// kernel-argument and vn_tab / vn_wdeg loads.  Only what the T loop holds anyway (the lane's slot
// addresses and variable, the wave's degree bounds) survives the loop back; the check-lane setup,
// the channel planes and the LDS init are redone per pack.
constexpr bool bs_loops(const BsInst& k) { return k.VPL == 1 && k.CPL == 1 && !k.UCN; }
// BS_LOOP_TU: this translation unit's instance (ldpc_bs_inst.hip, -DBS_INST=i) has the loop:
// kBsInst 0-2 (launch_bs_x checks it against bs_loops).  The loop's statements are compiled only
// there, so the units of the other instances see the kernel text without them -- compiled in but
// constant-false, the added statements alone changed those instances' register allocation.
#if defined(BS_INST) && BS_INST <= 2
#define BS_LOOP_TU 1
#else
#define BS_LOOP_TU 0
#endif
// The arguments of the pack-loop units' builds (kBsInst 0-2, every build of theirs): the build's
// own struct and, appended, the check tables' places in the fixed set, so that no existing field
// moves and the other instances' kernel arguments stay as they are.
template <class K>
struct BsArgsAf : K {
    const int32_t* atid;         // [T] kBetaTab index of iteration t's check table Q(relu(alpha m))
                                 // (host::WeightInfo::alpha_tid, every entry >= 0), or null: the
                                 // check phase reads the alpha tables from LDS
};
template <class K>
using BsKernArgs = std::conditional_t<BS_LOOP_TU != 0, BsArgsAf<K>, K>;
// How the pack loop hands out its packs.  A workgroup's first pack is blockIdx.x; every pack's
// prologue takes the ticket of the pack after it -- one lane's returning atomic add on the launch's
// ticket word, issued ahead of the channel's loads (the in-prologue channel: ahead of the sampler's
// tables) so that their round trip covers its own -- and parks gridDim.x + ticket in RED[BS_RED_NEXT]
// once the LLRs are packed, before the channel barrier (the in-prologue channel: after the tables'
// barrier, so the ticket is not held through the sampler); every wave reads the word in the loop
// condition, behind the channel barrier at the least.  So a workgroup that decodes faster takes more packs: the three
// workgroups of a CU run at different rates for the whole launch (profiles/r10), and by fixed
// stride the launch lasted as long as the slowest.  Without a ticket word (BsArgs::cn_hd null)
// the parked index is pack + gridDim.x, the fixed stride.  RED[8..15] are outside the per-pack
// init (RED[12]: the stamp builds' SIMD of wave 0).
constexpr int BS_RED_NEXT = 8;
// The WF builds' id words (k_bs, WF), T words at the start of the alpha-table region of LDS, which
// those builds leave unused: word t = the fixed-set id of iteration t's check table | the code of
// iteration t + 1's channel table << 16 (the variable phase of iteration t forms |Q(beta_{t+1} ch)|;
// the last takes none).  A channel table's code is its fixed-set id, or BS_WF_IDENT: the identity.
constexpr int BS_WF_IDENT = kNBetaTab;
// what a pack (index pk) derives from the arguments alone: at the kernel's entry with one pack
// per workgroup, at each pack's top in the pack loop.  RED: [0] wrong_t, [1] all t, [2] APP > 0,
// [3] bits; flor: the FLORW OR words; ALUT [2][AR][LUT_W], BLUT [2][bcols][BLUT_W];
// ucn_on(t): UCN work of iteration t's check phase (the syndromes, the alpha' table) and of the
// hard decisions the variable phase writes for it, skipped where alpha'_t = alpha_t
#define BS_PACK_SETUP(pk)                                                                          \
    const int64_t b0 = (int64_t)(pk) * PACK;                                                       \
    const int nvalid = (int)min<int64_t>(PACK, a.B - b0);                                          \
    const uint32_t valid = (nvalid >= 32) ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);                   \
    uint32_t* RED = reinterpret_cast<uint32_t*>(smem + (FZ ? W::off_red : a.off_red));             \
    const int flor = 16 + ((a.T + 3) & ~3);                                                        \
    const int AR = UCN ? 2 * (FZ ? W::arows : a.arows) : (FZ ? W::arows : a.arows);                \
    const int AL = AR * LUT_W, BL = (FZ ? W::bcols : a.bcols) * BLUT_W;                            \
    uint32_t* ALUT = reinterpret_cast<uint32_t*>(smem + (FZ ? W::off_alut : a.off_alut));          \
    uint32_t* BLUT = reinterpret_cast<uint32_t*>(smem + (FZ ? W::off_blut : a.off_blut));          \
    const bool ucn = UCN && a.ucn;                                                                 \
    auto ucn_on = [&](int t) __attribute__((always_inline)) -> bool {                              \
        return ucn && (t >= 64 || ((a.ucn_iter >> t) & 1));                                        \
    };

// Register budget: the small instances run at 64 VGPRs (WPE 8: three 9-wave workgroups per CU).
// At a 72-register budget only two were resident (the waves of a workgroup are not spread evenly
// over the SIMDs): measured 7.56 ms (72 VGPRs) -> 6.51 ms (64) per 2^20-codeword C2 decode.
// XP: the hard-bit export build (a.hdx: every iteration's hard decisions, for the hard_bits /
// synd_bits outputs); the counters-only build is the one the bench and the sweeps run.
// LB: the workgroup size bound (1024 lanes for every instance)
// Q8: the channel generated in the prologue (a.gen: ldpc_decode_awgn) instead of read as float
// LLRs; a build of its own (a run-time branch moved the register allocation of the whole kernel: C3's
// spills 5 -> 9 VGPRs)
// EW: the early-stop build that also keeps each codeword's hard decisions at its stop iteration
// (DESIGN 3.9): a build of its own beside the ES build, which stays as it is.
// L8: the LLRs read as int8 grid values (a.llr points at bytes: ldpc_decode_q8), a
// build of its own for the reason Q8 is one; a pack with an invalid byte is marked, never fixed up;
// with ES / EW the int8 builds of the early-stop kernels (ldpc_decode_q8_es)
// ES: the early-stop build (one-chunk UCN-compiled instances, one pack per
// workgroup).  The hard decisions go to HD and the check phases take their syndromes at every
// iteration; a pack leaves the T loop once each of its codewords has had a zero syndrome, and the
// epilogue takes every codeword's outputs at its own first zero-syndrome iteration.
template <int D, int DV, int LPC, int VPL, int CPL, bool UCN, bool BIG, bool PK, int WPE, bool XP, int LB, bool Q8,
          bool ES = false, bool EW = false, bool FZ = false, bool L8 = false, bool WF = false>
__global__ void __launch_bounds__(LB) __attribute__((amdgpu_waves_per_eu(WPE)))
k_bs(BsKernArgs<std::conditional_t<ES, std::conditional_t<EW, BsArgsEw, BsArgsEs>, std::conditional_t<XP, BsArgsXp, BsArgs>>> a) {
    static_assert(LPC == 2 || LPC == 4, "lanes per check");
    using KArgs = std::conditional_t<ES, std::conditional_t<EW, BsArgsEw, BsArgsEs>, std::conditional_t<XP, BsArgsXp, BsArgs>>;
    static_assert(!ES || (UCN && VPL == 1 && CPL == 1 && !XP), "early stop: one-chunk UCN-compiled instances");
    static_assert(!EW || ES, "the stop-iteration word: early-stop builds");
    static_assert(!L8 || (!Q8 && !FZ), "int8 LLRs: the decode, export and early-stop builds");
    // FZ: the geometry-frozen build (ldpc_bs_frozen.h): the pack geometry is W's literals instead
    // of kernel arguments, (FZ ? W::x : a.x) at each read -- written out, not behind an accessor:
    // through one the other builds' code changed; the pack-loop decode and in-prologue channel
    // builds of wman
    static_assert(!FZ || (BS_LOOP_TU && !UCN && !XP && !ES && VPL == 1 && CPL == 1 && D == 15 && DV == 6 && LPC == 4),
                  "frozen geometry: the wman pack-loop builds");
    using W = BsFrozenWman;
    static_assert(W::cstride == W::z * SLOT_B && W::AL == W::arows * LUT_W && W::BL == W::bcols * BLUT_W &&
                  W::NT == 64 * W::nw && W::off_zero == W::off_pad + SLOT_B, "BsFrozenWman is consistent");
    constexpr int SB = (DV * QMAX + QMAX <= 127) ? 8 : 9;     // planes of S and of lw + S
    constexpr int EPL = (D + LPC - 1) / LPC;                     // edge slots per check lane
    constexpr bool SKIPM = CPL > 1;                              // chunk-wide padding skipped
    constexpr int OB = 4 / LPC;                                  // alpha-table output bits per lane
    constexpr int VNA = PK ? (DV + 1) / 2 : DV;                  // address words per variable
    constexpr int VNW = VNA + 1;
    constexpr int HDW = (EPL + 1) / 2;                           // packed hd addresses per check lane
    // the check lane's slot base and alpha-table address packed in one register (16-bit-address
    // one-chunk instances; ldpc_bs.hip checks that the tables end below 64 KB)
    constexpr bool PKG = PK && CPL == 1;
    // ---- per-instance tuning values (ONE: a one-chunk instance, several workgroups per CU) ----
    constexpr bool ONE = VPL == 1 && CPL == 1;
    // the loop's wave priorities: 4 wman (DV 6: check phase 2, variable phase 1 on the waves of
    // the heaviest variables), 2 802.11n (check phase 1, variable phase 0), 0 the multi-chunk ones
    constexpr int PRIO = ONE ? (DV >= 6 ? 4 : 2) : 0;
    // the prologue's wave priority: 3 on the PRIO 4 instances (wman), 0 elsewhere
    constexpr int PROPRIO = PRIO == 4 ? 3 : 0;
    // iteration 0's tables copied asynchronously behind the channel loads: the one-chunk
    // instances; the multi-chunk ones copy through registers after the channel barrier
    constexpr bool T0A = ONE;
    // the prologue's first barrier after the first LLR loads are issued: where T0A
    constexpr bool EBR = T0A;
    // plane counts below the instance's that get a copy of the variable phase (1 seven, 2
    // eight): both on the one-chunk instances, eight only on the multi-chunk ones
    constexpr int SBSET = ONE ? 3 : 2;
    // C->V messages kept in registers from the sum pass to the V->C pass: all DV where DV <= 4
    // (802.11n), else 3 of wman's 6, 7 of 5G BG2's 8 and 4 of them with UCN
    constexpr int KEEP0 = ONE ? 3 : (UCN ? 4 : 7);
    constexpr int KEEP = DV <= 4 ? DV : (KEEP0 < DV ? KEEP0 : DV - 1);
    // the channel-table ids of the next variable phase loaded before the check phase: the
    // multi-chunk instances (one workgroup per CU: nothing else hides the L2 round trip)
    constexpr bool BKPF = !XP && VPL > 1;
    // AFX: the build can weigh the check minima through the fixed-set tables (beta_asm) when the
    // launch gives their ids (BsArgsAf::atid): the pack-loop units
    constexpr bool AFX = BS_LOOP_TU != 0;
    static_assert(!AFX || (ONE && !UCN), "fixed-set check tables: the one-chunk instances without UCN");
    // WF: the weights frozen in kind: every iteration's check table and channel table
    // is a table of the fixed set (or the identity channel table), so the build has no other path
    // for either -- no table words in LDS or SGPRs, no table copies, no tests of the ids' pointers --
    // and its T loop reads the ids from LDS words (BS_WF_* below), not from scalar memory: a scalar
    // load's result returns out of order, so each use of one waits for lgkmcnt(0), which also drains
    // the slot reads in flight.  The host takes it only when all T ids of both kinds exist
    // (ldpc_bs.hip, bs_weight_path); builds of the geometry-frozen decode and in-prologue channel
    // builds of wman.
    static_assert(!WF || (FZ && AFX && !BIG && !L8), "weights frozen in kind: on the geometry-frozen builds");
    // (the variable phase's channel code comes out of the check phase's id word: every wave runs it)
    static_assert(!WF || BsFrozenWman::cn_lanes >= BsFrozenWman::NT, "weights frozen in kind: every wave holds check lanes");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if ((uint32_t)(uintptr_t)smem != 0u) __builtin_trap();          // slots are LDS-absolute
#ifdef BS_STAMP
    // per-wave phase times (wave-uniform, s_memtime shader clocks): where a wave's time goes,
    // barrier waits included (diagnostic builds only)
    uint64_t sacc[13] = {};
    uint64_t sts = __builtin_amdgcn_s_memtime();
    // one record per workgroup behind the per-wave table (BS_WG_REC words each, at stamps +
    // BS_WG_BASE): [0] packs run, [1] / [2] the 100 MHz constant-rate clock at entry / exit,
    // [3] / [4] wave 0's shader clock at entry / exit, [5] XCC_ID << 32 | HW_ID of wave 0.  The
    // entry values are stored at once, so nothing of the record is held through the T loop.
    // Analysis: tools/wg_tail.py
    if (a.stamps && threadIdx.x == 0) {
        unsigned long long* rec = a.stamps + BS_WG_BASE + (size_t)BS_WG_REC * blockIdx.x;
        rec[1] = __builtin_amdgcn_s_memrealtime();
        rec[3] = sts;
    }
#define BS_ST(i)                                                                                   \
    do {                                                                                           \
        const uint64_t tn_ = __builtin_amdgcn_s_memtime();                                         \
        sacc[i] += tn_ - sts;                                                                      \
        sts = tn_;                                                                                 \
    } while (0)
#else
#define BS_ST(i) ((void)0)
#endif
    const int tid = threadIdx.x;
    const int NT = FZ ? W::NT : (int)blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwv = NT >> 6;
    const int nv = (FZ ? W::n_vars : a.n_vars);
#if !BS_LOOP_TU
    BS_PACK_SETUP(blockIdx.x)
#endif

    if (PROPRIO > 0) __builtin_amdgcn_s_setprio(PROPRIO);
    // ---- per-lane variables: slot addresses, variable index, degree bounds of the wave ----------
    uint32_t va[VPL][VNA];
    int vv[VPL], dw[VPL], dwmin[VPL], pcol[VPL];
    uint32_t tab_b[VPL];
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
        const uint32_t* vt = a.vn_tab + ((size_t)u * NT + tid) * VNW;
#pragma unroll
        for (int p = 0; p < VNA; ++p) va[u][p] = vt[p];
        vv[u] = (int)vt[VNA];                                // -1: no variable (UCN: v | HD index << 16)
        dw[u] = __builtin_amdgcn_readfirstlane(a.vn_wdeg[3 * (u * nwv + wave)]);
        dwmin[u] = __builtin_amdgcn_readfirstlane(a.vn_wdeg[3 * (u * nwv + wave) + 1]);
        pcol[u] = __builtin_amdgcn_readfirstlane(a.vn_wdeg[3 * (u * nwv + wave) + 2]);
        tab_b[u] = ((FZ ? W::bcols : a.bcols) > 1 && vv[u] >= 0) ? (uint32_t)(((UCN ? (vv[u] & 0xFFFF) : vv[u]) / (nv / (FZ ? W::bcols : a.bcols))) * BLUT_W * 4) : 0u;
    }
    // (the pack loop's units: bit 8 marks the wave that folds the frame-error words in the T loop,
    // a.fold_wave, carried in a word the loop holds anyway -- there the arguments are read through
    // the pack's opaque pointer, and read at the fold the index was a scalar load and its wait on
    // every wave, every iteration; degrees are below 256.  The other units compare a.fold_wave,
    // which they hold in SGPRs: carrying the mark cost the 802.11n early-stop build 7 reloads.)
    constexpr int FOLDB = BS_LOOP_TU ? 0x100 : 0;
    int cn_dmin = (FZ ? W::cn_dmin : a.cn_dmin) | ((FOLDB && (uint32_t)wave == a.fold_wave) ? FOLDB : 0);

    // ---- channel planes: the lane's variables for the 32 codewords of the pack ------------------
    // (no __syncthreads_or: it allocates static LDS, which would move the dynamic LDS base
    // away from 0; the flag word lives in RED)
    // one workgroup per CU: the first generation starts in lockstep, and with every pack taking
    // the same time, each later generation again fetches its LLR blocks in one chip-wide burst
    // while HBM idles the rest of the pack.  Spreading the first starts over a pack's duration
    // keeps the fetches apart for the whole grid (later workgroups inherit the offsets).
    if (a.stagger > 0 && (int)blockIdx.x < a.stagger_n) {
        const int n = (int)(((uint32_t)blockIdx.x * 97u % (uint32_t)a.stagger_n) * (uint32_t)a.stagger /
                            (uint32_t)a.stagger_n);
        for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(8);
    }
    // ---- the packs of this workgroup (BS_LOOP_TU; else the one pack blockIdx.x) ----------------
    // (the body keeps the indentation it had as the whole kernel)
#if BS_LOOP_TU
    auto lane_now = [&]() __attribute__((always_inline)) -> int {
        uint32_t all = ~0u;
        asm volatile("" : "+s"(all));
        return (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
    };
    unsigned pack = blockIdx.x;
#ifdef BS_STAMP
    unsigned long long npk = 0ull;
#endif
    do {
    if (pack != blockIdx.x) {
        // the pack before: its epilogue's reads of RED (and, off the grid, of RED[7]) come before
        // this pack's init writes
        __syncthreads();
        if (PROPRIO > 0) __builtin_amdgcn_s_setprio(PROPRIO);
    }
    // What a pack's prologue derives from the kernel arguments and the thread index alone is the
    // same for every pack, and hoisted over the pack loop it would be held in registers through
    // the T loop (the first build did: 104 VGPRs and 127 SGPRs spilled on wman).  So each pack
    // reads the arguments through an opaque copy of the kernel-argument pointer (`a` below: the
    // pack's view of them, in the constant address space) and computes its thread index again,
    // from the wave index and mbcnt through an operand that cannot be hoisted (the launch's v0 is
    // then dead after the entry loads): its prologue is redone, as one pack per workgroup did.
    typedef __attribute__((address_space(4))) const BsArgs PackArgs;
    PackArgs* kap = (PackArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kap));
    PackArgs& a = *kap;
    const int tid = wave * 64 + lane_now(), lane = tid & 63;
    BS_PACK_SETUP(pack)
    // (the frozen builds read the counted bits once per pack, not at every variable phase: with the
    // geometry out of the registers there is room to hold it)
    [[maybe_unused]] const int pack_tbits = FZ ? a.target_bits : 0;
#define BS_TBITS (FZ ? pack_tbits : a.target_bits)
#define BS_PK pack
#define BS_NEXT_PACK continue
#define BS_LANE_IS0 (lane_now() == 0)
#else
#define BS_TBITS a.target_bits
#define BS_PK blockIdx.x
#define BS_NEXT_PACK return
#define BS_LANE_IS0 (lane == 0)
#endif
    // PAD slot (all ones: V->C negative, magnitude 15), ZERO slot (a zero C->V), the zero hard
    // decision word of UCN padding edges, the counters and the off-grid flag RED[7]; iteration
    // 0's tables are copied global -> LDS asynchronously (global_load_lds) behind the channel
    // loads, retired by the channel barrier (through registers, each thread's loads waited in
    // turn: three L2 round trips and a barrier of their own per pack)
    if (tid < SLOT_W) {
        reinterpret_cast<uint32_t*>(smem + (FZ ? W::off_pad : a.off_pad))[tid] = 0xFFFFFFFFu;
        reinterpret_cast<uint32_t*>(smem + (FZ ? W::off_zero : a.off_zero))[tid] = 0u;
    }
    if (UCN && tid == 0) lds_put(a.off_hdz, 0u);
    if (tid < 8) RED[tid] = (tid == 1) ? 0xFFFFFFFFu : 0u;
#ifdef BS_STAMP
    if (tid == 0) {
        uint32_t hw0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw0));
        RED[12] = (hw0 >> 4) & 3u;
    }
#endif
    if (tid < FLORW) RED[flor + tid] = 0u;
    // early stop: the done word (wave-uniform, every wave keeps its own copy: a codeword's bit is
    // set once an iteration's hard decisions had a zero syndrome; the bits past the pack's
    // codewords start set, so a ragged pack's padding never holds the pack back) and the T
    // syndrome words, zeroed
    [[maybe_unused]] uint32_t es_done = ~valid;
    if constexpr (ES) {
        for (int w = tid; w < a.T; w += NT) RED[flor + FLORW + w] = 0u;
    }
    // (EW: the lane's variable's hard decisions, each codeword's bit taken at its stop iteration;
    // one register through the loop, stored once after it)
    [[maybe_unused]] uint32_t es_hd = 0u;
    // (the barrier that orders these writes before the channel's flag updates: here when the
    // channel is generated from the sampler's tables; else after the first variable's LLR loads
    // are issued, so that it waits beside their HBM round trip, EBR)
#if BS_LOOP_TU
    // (the generator's parameters, a copy: the pack's view of the arguments is in the constant
    // address space)
    BsGen gen{};
    if constexpr (Q8) {
        gen.tab = a.gen.tab;
        gen.k0 = a.gen.k0;
        gen.k1 = a.gen.k1;
        gen.offset = a.gen.offset;
        gen.nb = a.gen.nb;
        gen.kmin = a.gen.kmin;
        gen.ps = a.gen.ps;
        gen.pe = a.gen.pe;
        gen.ss = a.gen.ss;
        gen.se = a.gen.se;
        gen.lds = a.gen.lds;
    }
#define BS_GEN gen
#else
#define BS_GEN a.gen
#endif
#if BS_LOOP_TU
    // the next pack of this workgroup (lane 0 of the workgroup alone; BS_RED_NEXT)
    unsigned next_pack = pack + gridDim.x;
    auto take_ticket = [&]() __attribute__((always_inline)) {
        typedef __attribute__((address_space(1))) uint32_t GlobalW;
        GlobalW* tk = (GlobalW*)(uintptr_t)a.cn_hd;
        if (tid == 0 && tk)
            next_pack = gridDim.x + __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    if constexpr (Q8) take_ticket();
#endif
    if constexpr (Q8) gen_tables(BS_GEN, tid, NT);
    if (Q8 || !EBR) __syncthreads();
#if BS_LOOP_TU
    if constexpr (Q8) {
        if (tid == 0) RED[BS_RED_NEXT] = next_pack;
    }
#endif
    BS_ST(8);
    uint32_t cs[VPL], cm[VPL][4], bg[VPL];
    int off = 0;
    if (T0A && !WF) {                    // (retired by the channel barrier's vmcnt(0); WF: no table words)
        copy_async((FZ ? W::off_alut : a.off_alut), a.alut, AL, wave, NT);
        copy_async((FZ ? W::off_blut : a.off_blut), a.blut, BL, wave, NT);
    }
    // all 32 loads of a variable issued before any use: one HBM round trip per workgroup
    // prologue (with batches of 8 the LLR fetch cost 0.75 ms of a 6.5 ms C2 decode, with this
    // 0.44 ms: the workgroups stay in step, so every pack boundary is a chip-wide HBM burst; a
    // persistent grid prefetching the next pack during the check phases needed 6 more
    // loop-carried registers and spilled: 7.56 ms).
    // the pack's LLR rows through a buffer descriptor (wave-uniform base and size): each load is
    // buffer_load_dword with the lane's 4 v in voffset and the row's 4 r nv in soffset, so no
    // load needs a 64-bit VGPR address (with them the multi-variable lanes spilled the loaded
    // values and waited for each load in turn); rows past the batch read 0
    const __amdgpu_buffer_rsrc_t llr_rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.llr + b0 * nv), 0, nvalid * nv * 4, 0x00020000);
    auto llr_at = [&](int r, int v) __attribute__((always_inline)) -> float {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(llr_rs, 4 * v, 4 * r * nv, 0));
    };
    auto var_of = [&](int u) __attribute__((always_inline)) -> int {
        return (UCN && vv[u] >= 0) ? (vv[u] & 0xFFFF) : vv[u];
    };
    // lanes with several variables (VPL > 1) issue variable u + 1's loads after converting
    // variable u's, so no lane holds every variable's 32 values at once
    float xv[VPL][PACK];
    // (pack loop: defined on every path -- assigned only under [the lane has a variable], the 32
    // values were carried from one pack to the next, live through the T loop: 100 VGPRs spilled)
#if BS_LOOP_TU
#pragma unroll
    for (int r = 0; r < PACK; ++r) xv[0][r] = 0.f;
#endif
    if constexpr (Q8) {
        // generated channel (ldpc_decode_awgn): the grid bytes of the lane's variables from the
        // Philox stream, packed into planes as pack_channel's; never off the grid
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
            cs[u] = 0u;
            bg[u] = 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p) cm[u][p] = 0u;
            const int v = var_of(u);
            if (v >= 0 && !ABL(32)) {
                uint32_t Dq[8];
                gen_bytes(BS_GEN, BS_PK, v, a.qmax, Dq);
                pack_bytes<BIG>(Dq, valid, cs[u], cm[u], bg[u]);
            }
        }
    } else if constexpr (L8) {
        // int8 LLRs (ldpc_decode_q8): the float path's steps on bytes -- the same descriptor over the
        // pack's valid rows (one byte per LLR), the lane's v in voffset and the row's r nv in soffset
        // -- a row past the batch takes the last valid row's offset, a scalar min, so no load leaves
        // the pack's rows whatever the range check does with soffset, and pack_bytes masks its bits
        // as it masks the zeros the float path reads there; four rows per word, converted to the
        // bytes pack_bytes takes (ldpc_bitplane.h, l8_bytes).  An invalid byte in a row of the pack
        // raises the flag that sends a float pack to the fixup; here the pack is marked instead.
#if BS_LOOP_TU
        take_ticket();
#endif
        const __amdgpu_buffer_rsrc_t l8_rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(reinterpret_cast<const uint8_t*>(a.llr) + b0 * nv), 0, nvalid * nv, 0x00020000);
        auto l8_load = [&](uint32_t (&Dw)[8], int v) __attribute__((always_inline)) {
            uint32_t by[PACK];
#pragma unroll
            for (int r = 0; r < PACK; ++r)
                by[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(l8_rs, v, min(r, nvalid - 1) * nv, 0);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                Dw[i] = by[4 * i] | by[4 * i + 1] << 8 | by[4 * i + 2] << 16 | by[4 * i + 3] << 24;
        };
        // (pack loop: defined on every path, as xv is)
        uint32_t Dw[VPL][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) Dw[0][i] = 0u;
        if (var_of(0) >= 0 && !ABL(32)) l8_load(Dw[0], var_of(0));
        if (EBR) {
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0), vmcnt / expcnt untouched
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        const bool l8_big = BIG && a.cu > 0.f;
        uint32_t l8_bad = 0u;
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
            cs[u] = 0u;
            bg[u] = 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p) cm[u][p] = 0u;
            const int v = var_of(u);
            const int u1 = u + 1 < VPL ? u + 1 : u;
            const int vn = (u + 1 < VPL && !ABL(32)) ? var_of(u1) : -1;
            if (v >= 0 && !ABL(32)) {
                uint32_t Dk[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    uint32_t iv;
                    Dk[i] = l8_bytes(Dw[u][i], a.qmax, l8_big, iv);
                    l8_bad |= l8_invalid(iv, valid >> (4 * i));
                }
                pack_bytes<BIG>(Dk, valid, cs[u], cm[u], bg[u]);
            }
            if (vn >= 0) l8_load(Dw[u1], vn);
        }
        off = l8_bad != 0u;
#if BS_LOOP_TU
        if (tid == 0) RED[BS_RED_NEXT] = next_pack;
#endif
    } else {
#if BS_LOOP_TU
    take_ticket();
#endif
    if (var_of(0) >= 0 && !ABL(32)) {
#pragma unroll
        for (int r = 0; r < PACK; ++r) xv[0][r] = llr_at(r, var_of(0));
    }
    if (EBR) {
        // (a workgroup barrier without __syncthreads' fence, whose vmcnt(0) would wait for the
        // loads just issued: the LDS writes above complete (lgkmcnt(0)) and the compiler keeps
        // every memory access on its side)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0), vmcnt / expcnt untouched
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
        cs[u] = 0u;
        bg[u] = 0u;
#pragma unroll
        for (int p = 0; p < 4; ++p) cm[u][p] = 0u;
        const int v = var_of(u);
        const int u1 = u + 1 < VPL ? u + 1 : u;
        const int vn = (u + 1 < VPL && !ABL(32)) ? var_of(u1) : -1;
        if (v >= 0 && !ABL(32))
            off |= pack_channel<BIG>(xv[u], a.inv, a.qmax, a.cu, valid, cs[u], cm[u], bg[u]);
        if (vn >= 0) {
#pragma unroll
            for (int r = 0; r < PACK; ++r) xv[u1][r] = llr_at(r, vn);
        }
    }
#if BS_LOOP_TU
    // (after the channel's packing: the LLRs' round trip and their conversion cover the ticket's)
    if (tid == 0) RED[BS_RED_NEXT] = next_pack;
#endif
    }
    if (off) atomicOr(&RED[7], 1u);
    BS_ST(9);
    __syncthreads();
    BS_ST(10);
    if (RED[7]) {                              // off the grid: the v5 fixup decodes this pack
        if constexpr (ES) {
            // early stop: no fixup (v5 has no stop rule); the pack's frames are marked undecoded
            // and enter neither the counters nor the histogram
            if (tid < nvalid) {
                if (a.flags) a.flags[b0 + tid] = 0x80;
                if (kern_args<KArgs>().n_iter) kern_args<KArgs>().n_iter[b0 + tid] = 0;
            }
        }
        if constexpr (L8 && !ES) {
            // int8 LLRs: an invalid byte has no float decode to fall back to; marked the same way
            // (the early-stop int8 builds: by the block above, once)
            if (tid < nvalid && a.flags) a.flags[b0 + tid] = 0x80;
        }
        if (tid == 0) a.bad[BS_PK] = 1u;
        BS_NEXT_PACK;                          // (wave-uniform: every thread read the same word)
    }
    if (tid == 0) a.bad[BS_PK] = 0u;
    if (!T0A) {
        for (int w = tid; w < AL; w += NT) ALUT[w] = a.alut[w];
        for (int w = tid; w < BL; w += NT) BLUT[w] = a.blut[w];
        __syncthreads();
    }
    BS_ST(11);

    // ---- variable phase -------------------------------------------------------------------------
    //   first: lw_0 as every edge's V->C (no C->V yet);
    //   else:  S = sum of the C->V, APP_t = Q(ch) + S (hard decision, counters); unless last,
    //          Tv = clamp(Q(beta_{t+1} ch) + S) and V->C_e = clamp(Tv - C->V_e, +-15) per edge
    //   UCN:   the hard decision (APP_t >= 0; first: lw_0 >= 0) to HD[v] for the next check phase
    int bkp[VPL];                        // (BKPF) the ids of iteration tb's tables, loaded early
#pragma unroll
    for (int u = 0; u < VPL; ++u) bkp[u] = -1;
    // (WF) the code of the channel table the next variable phase takes (BS_WF_IDENT: the identity),
    // wave-uniform: iteration 0's from the arguments here, in the prologue; iteration t + 1's from
    // check phase t's id word
    [[maybe_unused]] int wf_bk = 0;
    if constexpr (WF) {
        wf_bk = (a.beta_id & 1) ? BS_WF_IDENT
                                : __builtin_amdgcn_readfirstlane((int)((const ConstW*)a.btid)[0]);
    }
    // |Q(beta_tb ch)| (4 planes) of the lane's variable u: the identity table, one of the fixed
    // set (wave-uniform id: a jump into immediate truth tables), the iteration's table in
    // constant memory (one beta per iteration) or the LDS table words (bslice)
    auto beta_lw = [&](const int u, const uint32_t bslice, const int tb, const uint32_t (&cmu)[4],
                       uint32_t (&lw)[4], const bool use_bk) __attribute__((always_inline)) {
        if constexpr (WF) {
            // the table's code (wave-uniform, wf_bk): the identity, or a table of the fixed set
            if (ABL(2) || wf_bk >= BS_WF_IDENT) {
                PH("vn_beta_id", u);
#pragma unroll
                for (int i = 0; i < 4; ++i) lw[i] = cmu[i];
            } else {
                PH("vn_beta_fix", u);
                beta_asm(lw, cmu, wf_bk);
            }
            return;
        }
        int bk = -1;
        if constexpr (!XP) {
            if (use_bk && a.btid) {
                const int col = ((FZ ? W::bcols : a.bcols) == 1) ? 0 : pcol[u];
                if (BKPF) bk = __builtin_amdgcn_readfirstlane(bkp[u]);
                else if (col >= 0)   // (a scalar load, through the constant address space)
                    bk = __builtin_amdgcn_readfirstlane((int)((const ConstW*)a.btid)[(size_t)tb * (FZ ? W::btid_n : a.btid_n) + col]);
            }
        }
        // identity table: |Q(beta ch)| = |ch| (the mask covers iterations 0..63)
        if (ABL(2) || (tb < 64 && ((a.beta_id >> tb) & 1))) {
            PH("vn_beta_id", u);
#pragma unroll
            for (int i = 0; i < 4; ++i) lw[i] = cmu[i];
        } else if (bk >= 0 && bk < kNBetaTab) {   // a table of the fixed set
            PH("vn_beta_fix", u);
            beta_asm(lw, cmu, bk);
            if constexpr (BIG) {            // shortened bits: |Q(beta cu)| from the table words
                if ((FZ ? W::bcols : a.bcols) == 1) {
                    const ConstW* tg = (const ConstW*)(a.blut) + (size_t)tb * BLUT_W;
#pragma unroll
                    for (int i = 0; i < 4; ++i) lw[i] = mux(bg[u], tg[LUT_W + i], lw[i]);
                } else {
                    const v4u gb = lds_q(bslice + tab_b[u] + LUT_W * 4);
                    lw[0] = mux(bg[u], gb.x, lw[0]);
                    lw[1] = mux(bg[u], gb.y, lw[1]);
                    lw[2] = mux(bg[u], gb.z, lw[2]);
                    lw[3] = mux(bg[u], gb.w, lw[3]);
                }
            }
        } else if ((FZ ? W::bcols : a.bcols) == 1) {      // one beta per iteration: table in SGPRs
            PH("vn_beta_sg", u);
            const ConstW* tg = (const ConstW*)(a.blut) + (size_t)tb * BLUT_W;
            lut_s(lw, cmu, tg);
            if constexpr (BIG) {
#pragma unroll
                for (int i = 0; i < 4; ++i) lw[i] = mux(bg[u], tg[LUT_W + i], lw[i]);
            }
        } else {
            PH("vn_beta_lds", u);
            const uint32_t btab = bslice + tab_b[u];
            const uint32_t cmi[1][4] = {{cmu[0], cmu[1], cmu[2], cmu[3]}};
            uint32_t lo[1][4];
            lut<1>(lo, cmi, btab);
#pragma unroll
            for (int i = 0; i < 4; ++i) lw[i] = lo[0][i];
            if constexpr (BIG) {
                const v4u gb = lds_q(btab + LUT_W * 4);
                lw[0] = mux(bg[u], gb.x, lw[0]);
                lw[1] = mux(bg[u], gb.y, lw[1]);
                lw[2] = mux(bg[u], gb.z, lw[2]);
                lw[3] = mux(bg[u], gb.w, lw[3]);
            }
        }
    };
    auto vn_phase = [&](const bool first, const bool last, const uint32_t bslice, const int tb)
                        __attribute__((always_inline)) {
        // (names `tid` so that the closure captures it: the phase does not read it, but without
        // the capture the compiler allocates the one-pack-per-workgroup instances' registers
        // differently, and those builds are tuned as they stand)
        (void)tid;
        uint32_t wr = 0u, apos = 0u, nb = 0u;
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
            // a (wave, u) place without a variable chunk (dw = -1, wave-uniform): nothing to do
            // (5G BG2: 20 chunks on 32 places; their beta table and Tv work used to run anyway)
            if (VPL > 1 && dw[u] < 0) continue;
            PH("vn_setup", (last ? 100 : 0) + u);
            // (the addresses made opaque per use: PK unpacked per use, not hoisted as twice the
            // registers; without it the multi-chunk build ran slower for fewer v_mov)
#pragma unroll
            for (int p = 0; p < VNA; ++p) asm volatile("" : "+v"(va[u][p]));
            auto vaddr = [&](int f) __attribute__((always_inline)) -> uint32_t {
                if constexpr (PK) return (f & 1) ? (va[u][f >> 1] >> 16) : (va[u][f >> 1] & 0xFFFFu);
                else return va[u][f];
            };
            const int v = (UCN && vv[u] >= 0) ? (vv[u] & 0xFFFF) : vv[u];
            const uint32_t hda = UCN ? 4u * ((uint32_t)vv[u] >> 16) : 0u;     // HD slot (rotated)
            const uint32_t cmu[4] = {cm[u][0], cm[u][1], cm[u][2], cm[u][3]};
            const bool counted = v >= 0 && v < BS_TBITS;
            uint32_t lw[1][4];                   // |Q(beta_{t+1} ch)| (before the C->V: fewer live registers)
            PH("vn_beta", (last ? 100 : 0) + u);
            if (!last) beta_lw(u, bslice, tb, cmu, lw[0], !first);
            // (C->V of the first KEEP edges stay in registers for the V->C pass, the others are
            // read from their slots again)
            const int dwu = dw[u];
            // the rest at SBX planes of S: the fewest that hold 15 dw + 15 for the place's largest
            // degree dw (wave-uniform): 7 where 15 dw + 15 <= 63, 8 where <= 127, else 9 (one
            // copy of the phase per plane count, SBSET)
            auto vbody = [&](auto sbc) __attribute__((always_inline)) {
                constexpr int SB = decltype(sbc)::value;
                uint32_t mn[KEEP > 0 ? KEEP : 1], mb[KEEP > 0 ? KEEP : 1][4];
                uint32_t S[SB];
#pragma unroll
                for (int i = 0; i < SB; ++i) S[i] = 0u;
                if (!first) {
#pragma unroll
                    for (int f = 0; f < DV; ++f) {
                        if (f < dwu) {
                            PH("vn_sum", 1000 * (SB - 6) + (last ? 100 : 0) + 10 * u + f);
                            uint32_t M[4], n, b[4];
                            read_slot(n, M, vaddr(f));
#pragma unroll
                            for (int i = 0; i < 4; ++i) b[i] = M[i] ^ n;
                            if (f == 0) set_b<SB>(S, b, n);
                            else add_b<SB>(S, b, n);
                            if (f < KEEP) {
                                mn[f < KEEP ? f : 0] = n;
#pragma unroll
                                for (int i = 0; i < 4; ++i) mb[f < KEEP ? f : 0][i] = b[i];
                            }
                        }
                    }
                    if constexpr (SB == 8) PH8("vn_app", 1000 * (SB - 6) + (last ? 100 : 0) + u, S, (S + 4));
                    else PH("vn_app", 1000 * (SB - 6) + (last ? 100 : 0) + u);
                    // APP_t = Q(ch) + S: the sign (hard decision) from the carry chain alone, the full
                    // sum only in the last iteration (APP > 0 for the loss counter)
                    uint32_t hd, nz = 0u;
                    const uint32_t c_s = cs[u];
                    if (last) {
                        uint32_t A[SB];
#pragma unroll
                        for (int i = 0; i < SB; ++i) A[i] = S[i];
                        const uint32_t cb[4] = {cmu[0] ^ c_s, cmu[1] ^ c_s, cmu[2] ^ c_s, cmu[3] ^ c_s};
                        add_b<SB>(A, cb, c_s);
                        hd = ~A[SB - 1];
#pragma unroll
                        for (int i = 0; i < SB; ++i) nz |= A[i];
                    } else {
                        uint32_t c = c_s;
#pragma unroll
                        for (int i = 0; i < SB - 1; ++i) c = B3(T_MAJ, S[i], i < 4 ? (cmu[i] ^ c_s) : c_s, c);
                        hd = B3(T_XNOR3, S[SB - 1], c_s, c);
                    }
                    // (early stop: at every iteration, for the next check phase's syndromes)
                    if (UCN && !last && v >= 0 && (ES || ucn_on(tb))) lds_put(hda, hd);   // HD[v] (Main_Functions.py:184-188)
                    hd &= valid;                                     // APP >= 0 -> hard decision 1
                    if constexpr (XP) {                              // iteration tb - 1's hard decisions
                        // (word mode, wave-uniform: the last iteration's alone, one row per pack)
                        const bool word = kern_args<KArgs>().word != 0;
                        const size_t row = word ? (size_t)BS_PK : (size_t)(tb - 1) * (size_t)((a.B + 31) >> 5) + BS_PK;
                        if (v >= 0 && (last || !word)) a.hdx[row * nv + v] = hd;
                    }
                    if (ABL(8)) hd = 0u;
                    if (counted) {
                        wr |= hd;
                        if (last) {
                            apos |= hd & nz;
                            // (early stop: the codewords not done before count at T - 1)
                            if constexpr (ES) nb += (uint32_t)__popc(hd & ~es_done);
                            else
                            nb += (uint32_t)__popc(hd);
                        }
                    }
                    // (the codewords that never stopped keep iteration T - 1's decisions)
                    if constexpr (EW) {
                        if (last) es_hd |= hd & ~es_done;
                    }
                }
                if (last) return;
                if constexpr (SB == 8) PH8("vn_tv", 1000 * (SB - 6) + (last ? 100 : 0) + u, S, (S + 4));
                else PH("vn_tv", 1000 * (SB - 6) + (last ? 100 : 0) + u);
                // Tv = clamp(Q(beta ch) + S): the table gives |Q(beta ch)|, the channel the sign
                uint32_t lb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) lb[i] = lw[0][i] ^ cs[u];
                add_b<SB>(S, lb, cs[u]);
                uint32_t Tv[6];
                clamp6<SB>(Tv, S);
                const int dwm = dwmin[u];
                if (first) {
                    // UCN at t = 0: the hard decision of x~ = Q(beta_0 ch) (Main_Functions.py:181-182)
                    if (UCN && v >= 0 && ucn_on(0)) lds_put(hda, ~Tv[5]);
                    uint32_t x[7], X[4];
#pragma unroll
                    for (int i = 0; i < 7; ++i) x[i] = Tv[i < 6 ? i : 5];
                    abs_sat(X, x);
#pragma unroll
                    for (int f = 0; f < DV; ++f)
                        if (f < dwu && (f < dwm || vaddr(f) != (FZ ? W::off_zero : a.off_zero))) write_slot(vaddr(f), x[6], X);
                } else {
#pragma unroll
                    for (int f = 0; f < DV; ++f) {
                        if (f < dwu) {
                            if (ABL(4)) continue;
                            PH("vn_vc", 1000 * (SB - 6) + (last ? 100 : 0) + 10 * u + f);
                            uint32_t x[7], X[4], n, b[4];
                            if (f < KEEP) {
                                n = mn[f < KEEP ? f : 0];
#pragma unroll
                                for (int i = 0; i < 4; ++i) b[i] = mb[f < KEEP ? f : 0][i];
                            } else {
                                uint32_t M[4];
                                read_slot(n, M, vaddr(f));
#pragma unroll
                                for (int i = 0; i < 4; ++i) b[i] = M[i] ^ n;
                            }
                            sub_tv(x, Tv, b, n);
                            abs_sat(X, x);
                            if (f < dwm || vaddr(f) != (FZ ? W::off_zero : a.off_zero)) write_slot(vaddr(f), x[6], X);
                        }
                    }
                }
            };
            if constexpr (SB >= 8) {
                if ((SBSET & 1) && dwu * QMAX + QMAX <= 63) vbody(std::integral_constant<int, 7>{});
                else if ((SBSET & 2) && SB == 9 && dwu * QMAX + QMAX <= 127) vbody(std::integral_constant<int, (SB == 9 ? 8 : SB)>{});
                else vbody(std::integral_constant<int, SB>{});
            } else {
                vbody(std::integral_constant<int, SB>{});
            }
        }
        // the frame-error words: every lane ORs its word into one of the FLORW LDS words, which
        // one wave folds in the next iteration; the last iteration reduces over the wave
        // (with its APP and bit counts) and lane 0 adds the results
        if (!first && !last) {
            PH("vn_flags", 0);
            if (!ABL(8)) {
                const uint32_t la = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 31u;
                __hip_atomic_fetch_or(RED + flor + la, wr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else if (!first) {
            PH("vn_flags", last ? 100 : 0);
            if (!ABL(8)) wr = wave_or(wr);
            if (last) {
                apos = wave_or(apos);
                nb = wave_add(nb);
            }
            if (BS_LANE_IS0) {
                if (wr) atomicOr(&RED[0], wr);
                if (last) {
                    if (apos) atomicOr(&RED[2], apos);
                    if (nb) atomicAdd(&RED[3], nb);
                }
            }
        }
    };

    vn_phase(true, false, (FZ ? W::off_blut : a.off_blut), 0);
    BS_ST(12);
    // (WF) the pack's id words (BS_WF_IDENT above), one per lane of the first T: loaded here, beside
    // the check setup's own global loads, and stored with its per-lane words ahead of the T loop's
    // barrier.  The region is written nowhere else.  The pack before read its last id word in check
    // phase T - 1, and the barriers after that check phase and its variable phase, and the one at
    // this pack's top, lie between that read and this store; besides, every pack of a launch
    // writes the same words.  Words that differed from pack to pack would rest on those barriers
    // alone.
    [[maybe_unused]] uint32_t wf_idw = 0u;
    if constexpr (WF) {
        if (tid < a.T) {
            wf_idw = (uint32_t)kern_args<BsArgsAf<KArgs>>().atid[tid];
            if (tid + 1 < a.T)
                wf_idw |= (((a.beta_id >> (tid + 1)) & 1) ? (uint32_t)BS_WF_IDENT
                                                          : (uint32_t)a.btid[(size_t)(tid + 1) * W::btid_n]) << 16;
        }
    }
    // check groups: chunk k of 64 check lanes; lane LPC c + j of it (check c = row i, index h)
    // takes edges k = LPC m + j, at slots first_i + j A_i + m z + h (a.row_lay); edges past the
    // degree read the all-ones PAD slot and are not written; idle lanes (c >= n_checks) read PAD
    // only.  (Lane j of a check's group evaluates alpha-table output bits OB j .. OB j + OB - 1:
    // 16 words per bit, at 64 B per bit.)
    const int cj = lane % LPC;
    int gchunk[CPL], gdeg[CPL], gm[CPL];
    uint32_t gbase[CPL], gtab[CPL], ghd[CPL][UCN ? HDW : 1];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        gchunk[c] = (CPL == 1) ? wave : __builtin_amdgcn_readfirstlane(a.cn_chunk[wave * CPL + c]);
        const int ql = max(gchunk[c], 0) * 64 + lane;
        const int cc = ql / LPC;
        const int ci = min(cc / (FZ ? W::z : a.z), (FZ ? W::n_checks : a.n_checks) / (FZ ? W::z : a.z) - 1);
        gdeg[c] = (cc < (FZ ? W::n_checks : a.n_checks)) ? a.row_ptr[ci + 1] - a.row_ptr[ci] : 0;
        // edge positions m holding a real edge for some lane of the chunk (wave-uniform): the
        // positions past them are padding for every lane and skipped (LPC, an even count, lanes
        // of each group skip together, so the group's [V->C >= 0] parity is unchanged)
        // (the instances with several check chunks per lane: 5G-type graphs, whose rows differ
        // in degree; the one-chunk instances serve near-regular rows and keep their registers)
        gm[c] = SKIPM ? (int)__popc(wave_or((1u << ((gdeg[c] + LPC - 1) / LPC)) - 1u)) : EPL;
        gbase[c] = (FZ ? W::off_slots : a.off_slots) + (uint32_t)((a.row_lay[2 * ci] + cj * a.row_lay[2 * ci + 1] + (cc - ci * (FZ ? W::z : a.z))) * SLOT_B);
        gtab[c] = (FZ ? W::off_alut : a.off_alut) + (uint32_t)(((FZ ? W::arows : a.arows) > 1 ? ci : 0) * LUT_W * 4) + (uint32_t)(cj * OB * 64);
        // (16-bit LDS addresses: the slot base and the alpha-table address share one register
        // through the T loop, unpacked per iteration)
        if constexpr (PKG) gbase[c] |= gtab[c] << 16;
        if constexpr (UCN) {
#pragma unroll
            // (the table holds the cn_lanes check lanes: a one-chunk instance's waves past them
            // read nothing -- their reads ran off the end of the allocation)
            for (int p = 0; p < HDW; ++p) ghd[c][p] = ((ES || ucn) && gchunk[c] >= 0 && ql < (FZ ? W::cn_lanes : a.cn_lanes)) ? a.cn_hd[(size_t)ql * HDW + p] : 0u;
        }
    }
    // the lane's real edge positions, one word for all its chunks (bit RB c + m: position m of
    // chunk c holds an edge of the lane's check), read through an opaque copy per iteration so
    // [LPC m + j < degree] is not hoisted out of the T loop as CPL x EPL 64-bit lane masks whose
    // SGPR pairs the loop spilled (bsc: 166 v_readlane reloads in the loop body before).  The
    // multi-chunk instances only: the one-chunk builds spill VGPRs with it (C2 3 -> 9, C3 7 -> 10)
    constexpr bool RPW = CPL > 1;
    constexpr int RB = EPL;
    static_assert(CPL * RB <= 32, "real-position word");
    static_assert(!SKIPM || EPL <= 8, "BS_MIN2_CASE covers 1..8");
    uint32_t rpk = 0u;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int m = 0; m < EPL; ++m)
            if (RPW && (LPC * m + LPC - 1 < cn_dmin || LPC * m + cj < gdeg[c])) rpk |= 1u << (RB * c + m);
    const uint32_t cstride = (uint32_t)((FZ ? W::z : a.z) * SLOT_B);
    const uint32_t tabu = (uint32_t)((FZ ? W::arows : a.arows) * LUT_W * 4);        // alpha' tables after the alpha ones
    // the one-chunk instances' check-lane slot base (packed with the alpha-table address) kept in
    // one LDS word per lane and read at each check phase, not in a register held through the T loop
    constexpr bool GBL = CPL == 1;
    if constexpr (GBL) lds_put((FZ ? W::off_ch : a.off_ch) + 4u * (uint32_t)tid, gbase[0]);
    if constexpr (WF) {
        if (tid < a.T) lds_put(W::off_alut + 4u * (uint32_t)tid, wf_idw);
    }
    // the one-chunk UCN instances' packed hard-decision addresses (HDW words per check lane)
    // likewise in LDS, read at each check phase
    constexpr bool HDL = UCN && CPL == 1;
    if constexpr (HDL) {
#pragma unroll
        for (int p = 0; p < HDW; ++p) lds_put(a.off_hdl + 4u * (uint32_t)(p * NT + tid), ghd[0][p]);
    }
    __syncthreads();

    BS_ST(4);
    for (int t = 0; t < (ABL(16) ? 0 : a.T); ++t) {
        PH("top", 0);
        // (the one-chunk instances fold after the check phase, on a wave with slack at its barrier)
        if (!ONE && wave == 0 && t > 0) {     // fold iteration t-1's frame flags
            // (every lane of wave 0 writes the same words: a wave-uniform branch, no thread
            // index kept live through the loop; kept in LDS for the iter_wrong export after the
            // loop: a global pointer held through it cost the 64-VGPR build 17 SGPR spill moves)
            // (the FLORW words of iteration t - 1, zeroed again)
            const uint32_t ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            uint32_t x = ln < 32u ? RED[flor + ln] : 0u;
            if (ln < 32u) RED[flor + ln] = 0u;
            const uint32_t w0 = wave_or(x);
            RED[16 + t - 1] = w0;
            RED[1] &= w0;
        }
        const int nx = (t + 1) & 1;
        // the fixed-set id of this iteration's check table (AFX builds, ids given): one scalar
        // load through the constant address space, used after the minima search.  The ids'
        // address comes from the kernel arguments again each iteration, behind an opaque pointer:
        // it is not held through the loop, and the loop is not duplicated over the
        // launch-uniform choice.
        int ak = 0;
        bool afx = false;
        // (WF: no scalar load in the loop -- the check phase reads the id word from LDS)
        if constexpr (AFX && !WF) {
            typedef __attribute__((address_space(4))) const BsArgsAf<KArgs> ConstAf;
            ConstAf* kq = (ConstAf*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(kq));
            const ConstW* at = (const ConstW*)kq->atid;
            afx = at != nullptr;
            if (afx) ak = (int)at[t];
        }
#pragma unroll
        for (int u = 0; u < VPL; ++u) asm volatile("" : "+s"(dw[u]), "+s"(dwmin[u]));   // compared per use, not hoisted as masks
        if (!RPW) asm volatile("" : "+s"(cn_dmin));
        const int cdm = FZ ? W::cn_dmin : FOLDB ? (cn_dmin & (FOLDB - 1)) : cn_dmin;    // (without the fold mark)
        // (the lane's variable made opaque per iteration on the multi-chunk instances: [v >= 0]
        // and [v < target bits] are compared per use, not held through the loop as spilled
        // 64-bit lane masks)
        if (RPW) {
#pragma unroll
            for (int u = 0; u < VPL; ++u) asm volatile("" : "+v"(vv[u]));
        }
        // next iteration's tables (their slots were last read two phases ago), copied global ->
        // LDS asynchronously: no wave waits for the loads, the barrier after the check phase
        // retires them
        // (WF: no table words at all, so neither copy nor the tables' pointers)
        if constexpr (!WF) {
            if (t + 1 < a.T) {
                // the copies' wave-uniform bounds made opaque per iteration, so their compares are
                // redone here instead of held through the loop as 64-bit lane masks (not in wman's
                // in-prologue channel build, which ran slower with it)
                int cw = wave, al = AL, bl = BL, bcl = (FZ ? W::bcols : a.bcols);
                // (the frozen builds: the bounds are literals.  The copy loop itself stays: a one-trip
                // form of it, or the wave count given to the compiler, each brought a VGPR spill back)
                if (!FZ && !(Q8 && VPL == 1 && CPL == 1 && !UCN))
                    asm volatile("" : "+s"(cw), "+s"(al), "+s"(bl), "+s"(bcl));
                // the tables' addresses loaded again from the kernel arguments each iteration (scalar
                // loads) instead of held through the loop, where they were spilled to VGPR lanes: the
                // one-chunk instances but wman's in-prologue channel build
                const uint32_t* alut_p = a.alut;
                const uint32_t* blut_p = a.blut;
                uint32_t off_al = (FZ ? W::off_alut : a.off_alut), off_bl = (FZ ? W::off_blut : a.off_blut);
                if constexpr (VPL == 1 && CPL == 1 && !(Q8 && !UCN)) {
                    typedef __attribute__((address_space(4))) const BsArgs ConstArgs;
                    ConstArgs* ka = (ConstArgs*)__builtin_amdgcn_kernarg_segment_ptr();
                    asm volatile("" : "+s"(ka));
                    alut_p = ka->alut;
                    blut_p = ka->blut;
                    if constexpr (!FZ) {
                        off_al = ka->off_alut;
                        off_bl = ka->off_blut;
                    }
                }
                // (no alpha table where the check phase takes the fixed set's: its LDS region stays unused)
                if (!(AFX && afx))
                    copy_async(off_al + 4u * (uint32_t)(nx * al), alut_p + (size_t)(t + 1) * al, al, cw, NT);
                if (bcl > 1)
                    copy_async(off_bl + 4u * (uint32_t)(nx * bl), blut_p + (size_t)(t + 1) * bl, bl, cw, NT);
            }
        }
        if constexpr (BKPF) {                // this iteration's variable phase: ids of row t + 1
            if (t + 1 < a.T && a.btid) {     // (the last variable phase takes no table)
#pragma unroll
                for (int u = 0; u < VPL; ++u) {
                    const int col = ((FZ ? W::bcols : a.bcols) == 1) ? 0 : pcol[u];
                    bkp[u] = col >= 0 ? a.btid[(size_t)(t + 1) * (FZ ? W::btid_n : a.btid_n) + col] : -1;
                }
            }
        }
        // ======== check nodes ===================================================================
        if (PRIO == 2) __builtin_amdgcn_s_setprio(1);
        if (PRIO == 4) __builtin_amdgcn_s_setprio(2);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const bool active = (CPL == 1) ? (FZ && W::cn_lanes >= W::NT) || wave * 64 < (FZ ? W::cn_lanes : a.cn_lanes) : (gchunk[c] >= 0);   // (cn_lanes: 64 k)
            if (!active || ABL(1)) continue;
            PH("ck_addr", c);
            uint32_t cbase;
            if constexpr (GBL) {
                // (the lane index from an operand the loop cannot hoist: a hoisted address was
                // itself held through the loop and spilled)
                uint32_t all = ~0u;
                asm volatile("" : "+s"(all));
                const uint32_t ln = __builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
                cbase = lds_w((FZ ? W::off_ch : a.off_ch) + ((uint32_t)wave << 8) + 4u * ln);
            } else {
                cbase = gbase[c];
                asm volatile("" : "+v"(cbase));
            }
            // (WF) iteration t's id word: every lane the same address, a broadcast read issued with
            // the slot base's, made wave-uniform after the minima search
            [[maybe_unused]] uint32_t idw = 0u;
            if constexpr (WF) idw = lds_w(W::off_alut + 4u * (uint32_t)t);
            uint32_t ctab = PKG ? (cbase >> 16) : gtab[c];
            if constexpr (PKG) cbase &= 0xFFFFu;
            int gmc = gm[c];
            asm volatile("" : "+s"(gmc));
            uint32_t rp = rpk;
            if (RPW) asm volatile("" : "+v"(rp));
            const int cdeg = gdeg[c];
            // slot m of the lane: a real edge (always while LPC m + LPC - 1 < cn_dmin)
            auto real = [&](int m) __attribute__((always_inline)) -> bool {
                if constexpr (RPW) return ((rp >> (RB * c + m)) & 1u) != 0u;
                else return LPC * m + LPC - 1 < cdm || LPC * m + cj < cdeg;
            };
            auto caddr = [&](int m) __attribute__((always_inline)) -> uint32_t {
                return real(m) ? cbase + m * cstride : (FZ ? W::off_pad : a.off_pad);
            };
            // pass 1: two minima of |V->C| and the parity of [V->C >= 0] over the lane's edges
            // (padding edges: negative, magnitude 15), then merged across the lane group
            // (the lane's EPL slots are read once, all loads issued before any use, and kept
            // in registers for pass 2)
            uint32_t Xs[EPL][4], ns[EPL];
            PH("ck_read", c);
#pragma unroll
            // (positions that are padding for the whole chunk are read like the others: the PAD
            // slot, every lane the same address, a broadcast)
            for (int m = 0; m < EPL; ++m) read_slot(ns[m], Xs[m], caddr(m));
            // UCN: syndrome of the previous hard decisions over the check (padding edges read a
            // zero word): odd -> the check is unsatisfied, its messages weighted by alpha'
            uint32_t syn = 0u;
            PH("ck_syn", c);
            const bool ucn_t = ucn_on(t);
            if constexpr (UCN) {
                // (early stop: check phase t > 0 takes the syndrome of iteration t - 1's hard
                // decisions whether or not alpha' needs it)
                if (ucn_t || (ES && t > 0)) {
                    // (the packed addresses made opaque per iteration: unpacked per use, not
                    // hoisted out of the T loop as EPL registers that the loop then spilled;
                    // HDL: read from LDS, through a lane index the loop cannot hoist)
                    uint32_t hwv[HDW];
                    if constexpr (HDL) {
                        uint32_t all = ~0u;
                        asm volatile("" : "+s"(all));
                        const uint32_t ln = __builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
#pragma unroll
                        for (int p = 0; p < HDW; ++p)
                            hwv[p] = lds_w(a.off_hdl + 4u * (uint32_t)(p * NT) + ((uint32_t)wave << 8) + 4u * ln);
                    } else {
#pragma unroll
                        for (int p = 0; p < HDW; ++p) {
                            asm volatile("" : "+v"(ghd[c][p]));
                            hwv[p] = ghd[c][p];
                        }
                    }
#pragma unroll
                    for (int m = 0; m < EPL; ++m) {
                        if (SKIPM && m >= gmc) continue;
                        const uint32_t hw = hwv[m >> 1];
                        syn ^= lds_w((m & 1) ? (hw >> 16) : (hw & 0xFFFFu));
                    }
                    syn ^= qperm<QP_X1>(syn);
                    if (LPC == 4) syn ^= qperm<QP_X2>(syn);
                    if constexpr (ES) {
                        // the codewords with an unsatisfied check, ORed into syndrome word t - 1
                        if (t > 0) {
                            const uint32_t wu = wave_or(syn);
                            if (wu && BS_LANE_IS0)
                                __hip_atomic_fetch_or(RED + flor + FLORW + (t - 1), wu,
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            }
            PH4("ck_min", c, Xs[EPL - 1]);
            uint32_t m1[4] = {Xs[0][0], Xs[0][1], Xs[0][2], Xs[0][3]}, m2[4] = {~0u, ~0u, ~0u, ~0u};
            uint32_t par = ns[0];
            // the bit-serial search over the whole lane group (min2_bits); cand[m] = [|V->C| of
            // slot m = m1] for pass 2
            uint32_t cand[EPL];
            // (padding positions: ~0, an even count of them over the LPC lanes of a group)
#pragma unroll
            for (int m = 1; m < EPL; ++m) par ^= ns[m];
            if constexpr (SKIPM) {
                // 1 <= gmc <= EPL for every active chunk, by construction (ceil(degree / lanes
                // per check) of its widest check): every other count is marked unreachable, so
                // the search's values are not kept alive through empty cases; the tie words of
                // the positions past gmc are zeroed
                switch (gmc) {                   // wave-uniform: the chunk's real positions
#define BS_MIN2_CASE(k)                                                                            \
    case k:                                                                                        \
        if constexpr (k <= EPL) {                                                                  \
            PH("ck_mink", 16 * c + k);                                                             \
            min2_bits<k, LPC>(m1, m2, cand, Xs);                                                   \
            _Pragma("unroll") for (int m = k; m < EPL; ++m) cand[m] = 0u;                          \
        } else {                                                                                   \
            __builtin_unreachable();                                                               \
        }                                                                                          \
        break;
                    BS_MIN2_CASE(1) BS_MIN2_CASE(2) BS_MIN2_CASE(3) BS_MIN2_CASE(4) BS_MIN2_CASE(5)
                    BS_MIN2_CASE(6) BS_MIN2_CASE(7) BS_MIN2_CASE(8)
#undef BS_MIN2_CASE
                    default:
                        __builtin_unreachable();
                }
            } else {
                min2_bits<EPL, LPC>(m1, m2, cand, Xs);
            }
            PH9("ck_merge", c, m1, m2, par);
            par ^= qperm<QP_X1>(par);
            if (LPC == 4) par ^= qperm<QP_X2>(par);
            // message k is negative iff an even number of the OTHER edges have V->C >= 0
            // (Main_Functions.py:251-254): par ^ n_k, par the parity of [V->C >= 0] over the
            // LPC EPL slots (an even count, padding included)
            // weighted, quantized minima: each lane evaluates OB output bits, the group shares them
            uint32_t q1[4], q2[4];
            PH9("ck_tab", c, m1, m2, par);
            if constexpr (WF) {
                // both minima through the immediate truth tables of the id word's check table; its
                // upper half is the code of the channel table this iteration's variable phase takes
                const uint32_t iw = (uint32_t)__builtin_amdgcn_readfirstlane((int)idw);
                wf_bk = (int)(iw >> 16);
                beta_asm(q1, m1, (int)(iw & 0xFFFFu));
                beta_asm(q2, m2, (int)(iw & 0xFFFFu));
            } else
            if (AFX && afx) {
                // alpha_t's table is table ak of the fixed set: both minima of the group, which
                // every lane of it holds, through the immediate truth tables -- all four planes in
                // each lane, no table words from LDS and no exchange over the lane group
                beta_asm(q1, m1, ak);
                beta_asm(q2, m2, ak);
            } else {
                const uint32_t mm[2][4] = {{m1[0], m1[1], m1[2], m1[3]}, {m2[0], m2[1], m2[2], m2[3]}};
                const uint32_t tab = ctab + (uint32_t)((t & 1) * AL * 4);
                uint32_t qb[OB][2];
                // alpha' is needed only where a check is unsatisfied for some codeword: a wave
                // whose checks are all satisfied in all 32 codewords (most waves once the
                // frames have converged) skips its table (the same messages, exactly)
                bool any_unsat = false;
                // (the multi-chunk instances only: the one-chunk UCN build ran slower with the test)
                if constexpr (UCN) any_unsat = ucn_t && (CPL == 1 || __builtin_amdgcn_ballot_w64(syn != 0u) != 0ull);
#pragma unroll
                for (int b = 0; b < OB; ++b) {
                    uint32_t o[2];
                    lut_bit<2>(o, mm, tab + (uint32_t)(b * 64));
                    if constexpr (UCN) {
                        if (any_unsat) {              // alpha' where the check is unsatisfied
                            uint32_t ou[2];
                            lut_bit<2>(ou, mm, tab + tabu + (uint32_t)(b * 64));
                            o[0] = mux(syn, ou[0], o[0]);
                            o[1] = mux(syn, ou[1], o[1]);
                        }
                    }
                    qb[b][0] = o[0];
                    qb[b][1] = o[1];
                }
                if (LPC == 4) {
                    q1[0] = qperm<0x00>(qb[0][0]); q1[1] = qperm<0x55>(qb[0][0]);
                    q1[2] = qperm<0xAA>(qb[0][0]); q1[3] = qperm<0xFF>(qb[0][0]);
                    q2[0] = qperm<0x00>(qb[0][1]); q2[1] = qperm<0x55>(qb[0][1]);
                    q2[2] = qperm<0xAA>(qb[0][1]); q2[3] = qperm<0xFF>(qb[0][1]);
                } else {                // lane 0 of a pair holds bits 0, 1; lane 1 bits 2, 3
                    q1[0] = qperm<0xA0>(qb[0][0]); q1[1] = qperm<0xA0>(qb[OB - 1][0]);
                    q1[2] = qperm<0xF5>(qb[0][0]); q1[3] = qperm<0xF5>(qb[OB - 1][0]);
                    q2[0] = qperm<0xA0>(qb[0][1]); q2[1] = qperm<0xA0>(qb[OB - 1][1]);
                    q2[2] = qperm<0xF5>(qb[0][1]); q2[3] = qperm<0xF5>(qb[OB - 1][1]);
                }
            }
            // pass 2: an edge whose |V->C| equals the minimum gets the weighted second minimum
            // (if it is not the only one, the two minima are equal), the others the minimum
#pragma unroll
            for (int m = 0; m < EPL; ++m) {
                if (m == 0) PH8("ck_pass2", 16 * c, q1, q2);
                if (real(m)) {
                    if (m > 0) PH("ck_pass2", 16 * c + m);
                    uint32_t Mg[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) Mg[i] = mux(cand[m], q2[i], q1[i]);
                    write_slot(cbase + m * cstride, par ^ ns[m], Mg);
                }
            }
        }
        if constexpr (ONE) {
            // fold iteration t-1's frame flags, off the check phase's critical wave: at the loop's
            // top wave 0 ran the fold (two LDS round trips and a wave_or) before its check work,
            // still at the variable phase's priority, and the check barrier waited for it (wman:
            // 83 K clocks per pack against 61-74 K on the two waves sharing its SIMD).  Here one
            // wave with slack at the check barrier folds after its own check work: the last wave
            // where it holds no check lanes (802.11n), else wave 1 (wman: waves 1-3 share their
            // SIMD with one other check wave, not two).
            // The words of t-1 are complete (the variable barrier of t-1) and are zero again
            // before any variable phase t ORs into them (the check barrier below).  RED[16 + t - 1]
            // and RED[1] have no reader inside the loop: the early-stop block below reads the
            // syndrome words and HD only, and both epilogues come after a barrier that follows
            // this one.
            const bool folds = FOLDB ? (cn_dmin & FOLDB) != 0 : (uint32_t)wave == a.fold_wave;
            if (folds && t > 0) {
                // (every lane writes the same words: a wave-uniform branch, no thread index kept
                // live through the loop; kept in LDS for the iter_wrong export after the loop)
                const uint32_t ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                uint32_t x = ln < 32u ? RED[flor + ln] : 0u;
                if (ln < 32u) RED[flor + ln] = 0u;
                const uint32_t w0 = wave_or(x);
                RED[16 + t - 1] = w0;
                RED[1] &= w0;
            }
        }
        BS_ST(0);
        __syncthreads();
        BS_ST(1);
        if constexpr (ES) {
            // ======== early stop ================================================================
            // syndrome word t - 1 is complete (the barrier): the codewords newly done at iteration
            // t - 1 are those with no unsatisfied check that were not done before.  Their bit
            // errors are counted from HD, which still holds iteration t - 1's hard decisions; once
            // every codeword is done the workgroup leaves the loop (every wave reads the same
            // word: a workgroup-uniform branch; the barrier retired the async table copies).
            if (t > 0) {
                const uint32_t un = (uint32_t)__builtin_amdgcn_readfirstlane((int)RED[flor + FLORW + t - 1]);
                const uint32_t nn = ~un & ~es_done;
                es_done |= nn;
                if (nn) {
                    const int v = vv[0] >= 0 ? (vv[0] & 0xFFFF) : -1;
                    uint32_t nb = 0u;
                    if constexpr (EW) {
                        // (every real variable's decisions, not the target bits' alone)
                        if (v >= 0) {
                            const uint32_t h = lds_w(4u * ((uint32_t)vv[0] >> 16)) & nn;
                            es_hd |= h;
                            if (v < a.target_bits) nb = (uint32_t)__popc(h);
                        }
                    } else
                    if (v >= 0 && v < a.target_bits)
                        nb = (uint32_t)__popc(lds_w(4u * ((uint32_t)vv[0] >> 16)) & nn);
                    nb = wave_add(nb);
                    if (nb && BS_LANE_IS0) atomicAdd(&RED[3], nb);
                }
                if (es_done == 0xFFFFFFFFu) break;
            }
        }
        // ======== variable nodes ================================================================
        if (PRIO == 2) __builtin_amdgcn_s_setprio(0);
        if (PRIO == 4) {                             // the waves of the heaviest variables first
            if (dw[0] >= DV - 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        const uint32_t bslice = (FZ ? W::off_blut : a.off_blut) + (uint32_t)(nx * BL * 4);
        if (t == a.T - 1) vn_phase(false, true, bslice, t + 1);
        else vn_phase(false, false, bslice, t + 1);
        BS_ST(2);
        __syncthreads();
        BS_ST(3);
    }
    // the epilogue's output pointers, loaded from the kernel arguments here, not held through
    // the T loop from the kernel's entry
    int64_t* e_counters = a.counters;
    uint8_t* e_flags = a.flags;
    uint32_t* e_iter_wrong = a.iter_wrong;
    int64_t e_B = a.B;
    // (not C4's decode build: more loop spills; not wman's decode build: 0.5 % slower)
    if constexpr (Q8 || (VPL == 1 && CPL == 1 && UCN)) {
        typedef __attribute__((address_space(4))) const BsArgs ConstArgs;
        ConstArgs* ka = (ConstArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        e_counters = ka->counters;
        e_flags = ka->flags;
        e_iter_wrong = ka->iter_wrong;
        e_B = ka->B;
    }
#if BS_LOOP_TU
    const int te = wave * 64 + lane_now();   // (`tid` is not held through the T loop)
#else
    const int te = tid;
#endif
    if constexpr (EW) {
        // the pack's row of the stop-iteration hard decisions: every word from the lane that owns
        // the variable, one store (a pack off the grid never gets here: word_out zeroes its rows)
        uint32_t* hdw = kern_args<KArgs>().hdw;
        const int v = vv[0] >= 0 ? (vv[0] & 0xFFFF) : -1;
        if (hdw && v >= 0) hdw[(size_t)BS_PK * nv + v] = es_hd;
    }
    if constexpr (ES) {
        // early stop: each codeword's outputs at its own stop iteration -- the first t whose
        // syndrome word has its bit clear, else T - 1 -- from the syndrome words and the
        // per-iteration frame-error words (RED[16 + t]; iteration T - 1's is RED[0]); one lane of
        // wave 0 per codeword.  (The words past the iteration the pack left the loop at are not
        // used: every codeword has stopped by then.)
        __syncthreads();                 // the bit counts of the waves that left the loop
        if (wave == 0) {
            const uint32_t* ESU = RED + flor + FLORW;
            const int r = te & 31;
            const bool on = te < nvalid;
            int stop = a.T - 1;
            uint32_t all = 1u, wl = 0u;
            bool open = true;
            for (int t = 0; t < a.T; ++t) {
                const bool lastt = t == a.T - 1;
                const uint32_t w = lastt ? RED[0] : RED[16 + t];
                const uint32_t u = lastt ? 0u : ESU[t];
                if (open) {
                    wl = (w >> r) & 1u;
                    all &= wl;
                    if (!((u >> r) & 1u)) {
                        stop = t;
                        open = false;
                    }
                }
            }
            const unsigned long long mw = __builtin_amdgcn_ballot_w64(on && wl != 0u);
            const unsigned long long ma = __builtin_amdgcn_ballot_w64(on && all != 0u);
            if (on) {
                if (e_flags) e_flags[b0 + te] = (uint8_t)(all | (wl << 1));
                if (kern_args<KArgs>().n_iter) kern_args<KArgs>().n_iter[b0 + te] = (uint8_t)(stop + 1);
            }
            if (te == 0 && e_counters) {
                unsigned long long* cc = reinterpret_cast<unsigned long long*>(e_counters);
                const unsigned long long c0 = RED[3], c1 = __popcll(mw), c2 = __popcll(ma);
                if (c0) atomicAdd(cc + 0, c0);
                if (c1) atomicAdd(cc + 1, c1);
                if (c2) atomicAdd(cc + 2, c2);
            }
            if (kern_args<KArgs>().iter_hist) {           // one atomic per distinct stop iteration of the pack
                unsigned long long rem = __builtin_amdgcn_ballot_w64(on);
                while (rem) {
                    const int l = __builtin_ctzll(rem);
                    const int ts = __builtin_amdgcn_readlane(stop, l);
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(on && stop == ts);
                    if (te == l)
                        atomicAdd(reinterpret_cast<unsigned long long*>(kern_args<KArgs>().iter_hist) + ts,
                                  (unsigned long long)__popcll(m));
                    rem &= ~m;
                }
            }
        }
    }
    if constexpr (!ES) {
    // (the body keeps the indentation it had before the early-stop builds)
    if (te == 0) {
        const uint32_t wl = RED[0] & valid;
        const uint32_t all = RED[1] & RED[0] & valid;
        const uint32_t ap = RED[2] & valid;
        RED[16 + a.T - 1] = RED[0];
        if (e_counters) {
            unsigned long long* cc = reinterpret_cast<unsigned long long*>(e_counters);
            const unsigned long long c0 = RED[3], c1 = __popc(wl), c2 = __popc(all),
                                     c3 = 2ull * __popc(ap) + __popc(wl & ~ap);
            if (c0) atomicAdd(cc + 0, c0);
            if (c1) atomicAdd(cc + 1, c1);
            if (c2) atomicAdd(cc + 2, c2);
            if (c3) atomicAdd(cc + 3, c3);
        }
        RED[5] = all;
        RED[6] = wl;
    }
    if (e_flags || e_iter_wrong) {
        __syncthreads();
        if (e_flags && te < nvalid)
            e_flags[b0 + te] = (uint8_t)(((RED[5] >> te) & 1) | (((RED[6] >> te) & 1) << 1));
        if (e_iter_wrong)                   // [T][packs]: iteration t's frame-error word
            for (int t = te; t < a.T; t += NT)
                e_iter_wrong[(size_t)t * (size_t)((e_B + 31) >> 5) + BS_PK] = RED[16 + t] & valid;
    }
    }
    BS_ST(5);
#if BS_LOOP_TU
#ifdef BS_STAMP
    ++npk;
#endif
    } while ((pack = (unsigned)__builtin_amdgcn_readfirstlane(
                  (int)reinterpret_cast<volatile uint32_t*>(smem + (FZ ? W::off_red : a.off_red))[BS_RED_NEXT])) <
             (unsigned)((a.B + PACK - 1) / PACK));
#elif defined(BS_STAMP)
    const unsigned long long npk = 1ull;
#endif
#undef BS_TBITS
#undef BS_PK
#undef BS_NEXT_PACK
#undef BS_LANE_IS0
#undef BS_GEN
#ifdef BS_STAMP
    if (a.stamps && lane == 0 && wave < 16) {
#pragma unroll
        for (int i = 0; i < 13; ++i) atomicAdd(a.stamps + 16 * wave + i, (unsigned long long)sacc[i]);
        atomicAdd(a.stamps + 16 * wave + 15, npk);
        // the SIMD this wave ran on (HW_ID bits 5:4) relative to wave 0's (RED[12]): counts in
        // 32-bit fields, offsets 0-1 in word 13, 2-3 in word 14
        uint32_t hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const uint32_t simd = (((hw >> 4) & 3u) - reinterpret_cast<uint32_t*>(smem + (FZ ? W::off_red : a.off_red))[12]) & 3u;
        atomicAdd(a.stamps + 16 * wave + 13 + (simd >> 1), npk << (32 * (simd & 1)));
        if (wave == 0) {
            uint32_t xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* rec = a.stamps + BS_WG_BASE + (size_t)BS_WG_REC * blockIdx.x;
            rec[0] = npk;
            rec[2] = __builtin_amdgcn_s_memrealtime();
            rec[4] = __builtin_amdgcn_s_memtime();
            rec[5] = (unsigned long long)xcc << 32 | hw;
        }
    }
#endif
#undef BS_ST
}

// ---- launch ---------------------------------------------------------------------------------
// What the host fills for one launch (bs_run): the arguments of every build of an instance -- BsArgs,
// the early-stop builds' additions and the export builds' word switch.  A launcher hands its kernel
// the argument struct that kernel takes, built from this one (bs_launch_kernel).
struct BsLaunch : BsArgsEw {
    int word;                    // BsArgsXp::word
    const int32_t* atid;         // BsArgsAf::atid (the pack-loop units' builds; null elsewhere)
    bool frozen;                 // host only: the plan equals BsFrozenWman (bs_frozen_fit) and the
                                 // request is a plain decode: launch the geometry-frozen build
    bool wf;                     // host only: of the frozen builds, the one with the weights frozen in
                                 // kind (k_bs, WF): atid and btid hold all T ids (bs_weight_path)
    uint32_t* ticket;            // host only: the pack loop's ticket word (launch_bs_x), or null:
                                 // fixed stride (LDPC_BS_TICKETS=0)
};

template <class K>
K kernel_arg_of(void (*)(K));    // (the argument struct of a kernel, for decltype)
// the kernel-argument struct K from the host's struct: that base of it (BsArgs, BsArgsEs,
// BsArgsEw) or, for the export builds' K, the BsArgs base and the word switch; bsc's alike
template <class K>
struct BsAfBase { using type = void; };
template <class K>
struct BsAfBase<BsArgsAf<K>> { using type = K; };
template <class K, class L>
K bs_kernel_args(const L& a) {
    if constexpr (std::is_base_of_v<K, L>) return a;
    else if constexpr (!std::is_void_v<typename BsAfBase<K>::type>)
        return K{bs_kernel_args<typename BsAfBase<K>::type>(a), a.atid};
    else return K{a, a.word};
}
// every build may ask for all of BS_LDS_MAX as dynamic LDS: set once per kernel
template <auto Fn>
void bs_max_lds() {
    static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(Fn),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)BS_LDS_MAX);
    (void)once;
}
// one launch of the build Fn (of either bit-sliced kernel) with nw waves per workgroup
template <auto Fn, class L>
int bs_launch_kernel(const L& a, int nblocks, int nw, size_t lds, hipStream_t s) {
    bs_max_lds<Fn>();
    hipLaunchKernelGGL(Fn, dim3(nblocks), dim3(64 * nw), lds, s, bs_kernel_args<decltype(kernel_arg_of(Fn))>(a));
    return hipGetLastError() == hipSuccess ? LDPC_OK : LDPC_ERR_HIP;
}

// grid: the workgroups launched; the instances with the pack loop (bs_loops) take any count from 1
// to the packs, the others exactly one per pack.  *resident (ldpc_bs.hip: one word per context and
// build): the workgroups of this instance, workgroup size and LDS size that fit the device at
// once, asked from the runtime when it is 0.
template <int I, bool XP, bool Q8, bool FZ = false, bool L8 = false, bool WF = false>
int launch_bs_x(const BsLaunch& a, int npacks, int nw, size_t lds, hipStream_t s, int grid, int* resident) {
    constexpr BsInst k = kBsInst[I];
    static_assert(bs_loops(k) == (BS_LOOP_TU != 0), "BS_LOOP_TU lists the instances of bs_loops");
    constexpr auto fn = &k_bs<k.D, k.DV, k.LPC, k.VPL, k.CPL, k.UCN, k.BIG, k.PK, k.WPE, XP, 1024, Q8, false, false, FZ, L8, WF>;
    int nblocks = npacks;
    if constexpr (bs_loops(k)) {
        if (grid < 0) {                      // (no LDPC_BS_GRID: the resident workgroups)
            if (*resident <= 0) {
                bs_max_lds<fn>();
                int dev = 0, ncu = 0, per_cu = 0;
                if (hipGetDevice(&dev) != hipSuccess ||
                    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn),
                                                                 64 * nw, lds) != hipSuccess ||
                    ncu <= 0 || per_cu <= 0) {
                    (void)hipGetLastError();
                    return LDPC_ERR_HIP;
                }
                *resident = ncu * per_cu;
            }
            grid = *resident;
        }
        if (grid > 0 && grid < npacks) nblocks = grid;
        // the packs past the first of each workgroup go by ticket (BS_RED_NEXT): the word is zeroed
        // on the stream before every launch that loops back -- not left at zero by the kernel, so
        // that a launch that died cannot make the next one skip packs
        BsLaunch t = a;
        t.cn_hd = nblocks < npacks ? a.ticket : nullptr;
        if (t.cn_hd && hipMemsetAsync(a.ticket, 0, sizeof(uint32_t), s) != hipSuccess) return LDPC_ERR_HIP;
        return bs_launch_kernel<fn>(t, nblocks, nw, lds, s);
    }
    return bs_launch_kernel<fn>(a, nblocks, nw, lds, s);
}

// the early-stop builds of an ES instance (float LLRs, or the in-prologue channel): one workgroup
// per pack, no pack loop (packs end at different times) and no export build
// (L8: the int8-LLR builds of the two; launched the same way)
template <int I, bool Q8, bool EW, bool L8 = false>
int launch_bs_es_x(const BsLaunch& a, int npacks, int nw, size_t lds, hipStream_t s) {
    constexpr BsInst k = kBsInst[I];
    static_assert(k.ES && !bs_loops(k), "an early-stop instance");
    return bs_launch_kernel<&k_bs<k.D, k.DV, k.LPC, k.VPL, k.CPL, k.UCN, k.BIG, k.PK, k.WPE, false, 1024, Q8, true, EW, false, L8>>(
        a, npacks, nw, lds, s);
}
// instance I's launch: an ES instance has the early-stop builds alone (with a plane buffer for the
// stop-iteration words, the EW build: DESIGN 3.9); the others never see the early-stop arguments
// The instances with the int8-LLR builds (L8): every one a plan takes by default for a decode
// without early stop; the A/B-only entries (2, 6) have none.  The early-stop entries (7, 8) have the
// int8 builds of their ES and EW kernels instead (launch_bs_any; ldpc_bs.hip, bs_l8_ok).
constexpr bool bs_l8_inst(int i) { return i == 0 || i == 1 || i == 3 || i == 4 || i == 5 || i == kBsInstUcn1; }
// the channel a launch decodes: float LLRs, the in-prologue generator (Q8 builds) or int8 LLRs (L8)
enum BsSrc { BS_SRC_LLR = 0, BS_SRC_GEN = 1, BS_SRC_L8 = 2 };
template <int I>
int launch_bs_any(const BsLaunch& a, int npacks, int nw, size_t lds, hipStream_t s, int src, int grid, int* resident) {
    const bool q8 = src == BS_SRC_GEN;
    if (src == BS_SRC_L8) {
        // (an early-stop instance: the int8 early-stop build, or with a plane buffer for the
        // stop-iteration words the int8 EW build)
        if constexpr (kBsInst[I].ES) {
            if (a.hdx) return LDPC_ERR_UNSUPPORTED;
            return a.hdw ? launch_bs_es_x<I, false, true, true>(a, npacks, nw, lds, s)
                         : launch_bs_es_x<I, false, false, true>(a, npacks, nw, lds, s);
        }
        // (resident[5 / 6]: the int8 decode and word builds; the word mode alone exports: hdx with word)
        if constexpr (bs_l8_inst(I)) {
            if (a.hdw || (a.hdx && !a.word)) return LDPC_ERR_UNSUPPORTED;
            return a.hdx ? launch_bs_x<I, true, false, false, true>(a, npacks, nw, lds, s, grid, resident + 6)
                         : launch_bs_x<I, false, false, false, true>(a, npacks, nw, lds, s, grid, resident + 5);
        }
        return LDPC_ERR_UNSUPPORTED;
    }
    if constexpr (kBsInst[I].ES) {
        if (a.hdx) return LDPC_ERR_UNSUPPORTED;
        if (a.hdw)
            return q8 ? launch_bs_es_x<I, true, true>(a, npacks, nw, lds, s)
                      : launch_bs_es_x<I, false, true>(a, npacks, nw, lds, s);
        return q8 ? launch_bs_es_x<I, true, false>(a, npacks, nw, lds, s)
                  : launch_bs_es_x<I, false, false>(a, npacks, nw, lds, s);
    } else {
        // (the generated channel comes from ldpc_decode_awgn, which exports no hard bits)
        // (resident[0 / 1 / 2]: the decode, the hard-bit export and the in-prologue channel build;
        // [3 / 4]: the geometry-frozen decode and in-prologue channel builds; [7 / 8]: the same two
        // with the weights frozen in kind)
        if constexpr (I == BsFrozenWman::inst) {
            if (a.frozen && a.wf && !a.hdx)
                return q8 ? launch_bs_x<I, false, true, true, false, true>(a, npacks, nw, lds, s, grid, resident + 8)
                          : launch_bs_x<I, false, false, true, false, true>(a, npacks, nw, lds, s, grid, resident + 7);
            if (a.frozen && !a.hdx)
                return q8 ? launch_bs_x<I, false, true, true>(a, npacks, nw, lds, s, grid, resident + 4)
                          : launch_bs_x<I, false, false, true>(a, npacks, nw, lds, s, grid, resident + 3);
        }
        if (a.hdx) return q8 ? LDPC_ERR_UNSUPPORTED : launch_bs_x<I, true, false>(a, npacks, nw, lds, s, grid, resident + 1);
        return q8 ? launch_bs_x<I, false, true>(a, npacks, nw, lds, s, grid, resident + 2)
                  : launch_bs_x<I, false, false>(a, npacks, nw, lds, s, grid, resident);
    }
}

// per-instance translation units (ldpc_bs_inst.hip, -DBS_INST=i)
template <int I>
int bs_launch(const BsLaunch& a, int npacks, int nw, size_t lds, hipStream_t s, int src, int grid, int* resident);

}  // namespace bs
}  // namespace ldpc
