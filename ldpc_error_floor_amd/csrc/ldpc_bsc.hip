// ldpc_bsc.hip — bit-sliced fused QMS decoder with COMPRESSED check messages ("bsc"), for the
// graphs whose one-slot-per-edge state (ldpc_bs_kernel.h: 20 B per lifted edge and pack) does
// not fit the 160 KB of LDS — 5G NR BG1 n2112 (C5: 8,784 edges = 176 KB).
//
// Same arithmetic and semantics as the bsl kernel (32 codewords per 32-bit word, one pack per
// workgroup, Main_Functions.py:157-335 in units of the q-bit grid) with a different state
// split (LDS per pack, BG1: 151 KB):
//   TV[v][6]      Tv = clamp(Q(beta ch) + S, [-32, 31]) per variable (6 two's-complement planes)
//   REC[c][8]     the check's two possible C->V magnitudes: q1 (every edge whose |V->C| is not
//                 the minimum) and q2 (those that are), 4 planes each
//   SGN[e], ARG[e] per edge: the C->V sign (parity ^ own V->C sign) and [|V->C| == minimum]
// so the check phase recomputes V->C = clamp(Tv - C->V_old, +-15) from Tv and its own previous
// message (instead of the variable phase writing it per edge), and the variable phase reads
// each edge's C->V as (SGN, ARG ? q2 : q1) from the check's record.  The check side keeps the
// bsl structure (LPC lanes per check, quad DPP merges, alpha table by mux tree); the variable
// side needs no per-edge write-back.  Variable lanes hold several variables (VPL) and check
// lanes several 64-lane chunks (CPL), one 16-wave workgroup per CU.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ldpc_bs_host.h"

namespace ldpc {
namespace bs {

// instances: D = check-degree bound, DVH / DVL = variable-degree bound of a lane's first /
// other variables, LPC lanes per check, VPL variables and CPL check chunks per lane
// (a wman-sized instance — one variable and one check chunk per lane, 64 VGPRs — was measured
// against bsl on C2: 61 spills, and the BG1 instance there ran 68 M cw/s against bsl's 176 M)
// MIX: rows of degree <= LPC / 2 * EPL take LPC / 2 lanes per check (their own 64-lane chunks,
// after the LPC-lane ones): one lane merge and one more table bit per lane instead of two
// merges and twice the lanes, for the low-degree rows
struct BscInst { int D, DVH, DVL, LPC, VPL, CPL; int WPE; int NW = 16; bool MIX = false; };
constexpr BscInst kBscInst[] = {
    {20, 10, 5, 4, 3, 3, 4},          // 5G BG1 (C5): degree 19 rows, degree 10 / 8 columns, 16 waves
    {20, 10, 5, 2, 3, 2, 4},          // the same with 2 lanes per check (LDPC_BS_LPC A/B)
    // 12 waves: 36 variable chunks on 36 places, 45 check chunks on 48, up to 168 VGPRs (the
    // 16-wave build spills 25 VGPRs at 128): LDPC_BSC_INST=2 A/B
    {20, 10, 5, 4, 3, 4, 3, 12},
    // mixed lanes per check (5G BG1: four degree-19 rows at 4 lanes, six of degree 3-10 at 2)
    {20, 10, 5, 4, 3, 3, 4, 16, true},
    {20, 10, 5, 4, 3, 2, 4, 16, true},
};

struct BscArgs {
    const float* llr;            // (Q8 builds: unused, the channel is generated, as bsl's)
    int64_t B;
    int n_vars, n_checks, T, target_bits, cn_dmin, z;
    float inv, cu;
    int qmax;                    // the grid's largest magnitude in grid units (15, 7 or 3)
    int beta_id;                 // every beta is 1: Q(beta ch) = ch, no table
    const int32_t* row_ptr;
    const int32_t* row_lay;      // [M][2] slot layout (as bsl): first slot, j-block stride
    const uint32_t* vn_tab;      // [VPL][64 nw][DVH + 1]: per edge slot | (record offset / 16) << 16, variable
    const int32_t* vn_wdeg;      // [VPL][nw][2]
    const int32_t* cn_chunk;     // [nw][CPL]
    const uint32_t* cn_var;      // [chunks * 64][CVW] variables of the lane's edges (16-bit packed)
    const int32_t* cn_lane;      // MIX: [chunks * 64] check | lane << 16 | lanes per check << 20, -1 idle
    const uint32_t* alut;        // [T][arows][LUT_W]
    const uint32_t* blut;        // [T][bcols][BLUT_W]
    int arows, bcols;
    int64_t* counters;
    uint8_t* flags;
    uint32_t* bad;
    uint32_t* iter_wrong;        // [T][packs] per-iteration frame-error words, or null
    int stagger, stagger_n;      // start offsets of workgroups 0 .. stagger_n - 1 (the first
                                 // generation, one per CU), spread over 0 .. stagger x 512 clocks
    uint32_t* hdx;               // XP builds: [T][packs][n_vars] hard decisions (as bsl's)
    uint32_t off_a, off_rec, off_tv, off_red, off_alut, off_blut;   // SGN at LDS byte 0
                                 // (RED: 16 words, then T words: iteration t's frame-error word)
    BsGen gen;                   // Q8 builds: the in-prologue channel (bsl's; tables at SGN)
};

// The export builds' arguments (XP): BscArgs and the word mode's switch (as bsl's
// BsArgsXp).
struct BscArgsXp : BscArgs {
    int word;                    // 1: hdx is [packs][n_vars], the last iteration's hard decisions alone
};

// The early-stop builds' arguments: BscArgs and what the mode adds, so the other
// builds' kernel arguments stay as they are.
struct BscArgsEs : BscArgs {
    uint8_t* n_iter;             // [B] iterations run per codeword (0: pack off the grid), or null
    int64_t* iter_hist;          // [T] += codewords with n_iter = t + 1, or null
    uint32_t off_u;              // LDS: the T syndrome words, after the FLORW words of RED: word t
                                 // = OR over the checks of the syndrome of iteration t's hard decisions
};

// The arguments of the early-stop builds that keep the decoded word (EW; as bsl's
// BsArgsEw): the ES builds' kernel arguments stay as they are.
struct BscArgsEw : BscArgsEs {
    uint32_t* hdw;               // [packs][n_vars] each codeword's hard decisions at its stop
                                 // iteration, or null: off
};

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

// Check records in blocks of 16: the q1 words of records 16 b .. 16 b + 15 (256 B), then their q2
// words (256 B), so q2 is q1 + 256 (an instruction offset) and a ds_read_b128 group of 16 lanes
// on consecutive records covers 64 distinct banks (with 32-B records side by side it covered 32,
// two-way).  Byte offset of record r inside REC:
__host__ __device__ constexpr uint32_t rec_off(uint32_t r) { return ((r >> 4) << 9) + ((r & 15u) << 4); }
constexpr uint32_t REC_Q2 = 256;
typedef __attribute__((address_space(3))) v2u LdsD;
__device__ __forceinline__ v2u lds_d(uint32_t addr) { return *reinterpret_cast<const LdsD*>(addr); }
__device__ __forceinline__ void lds_dput(uint32_t addr, uint32_t x, uint32_t y) {
    v2u v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<LdsD*>(addr) = v;
}

// B1: every beta is 1 and one column table (a.beta_id, bcols 1: C5's flat weights), so the
// channel term is Q(ch) itself and neither the beta table's operands nor the shortened-bit
// planes are live (C5's instance: 124 VGPRs, no spills, against 128 and 10 spilled)
// ES: the early-stop build, on top of B1 only.  There the Tv that the variable phase
// stores is clamp6(Q(ch) + S), whose sign is the sign of APP_t bit for bit (the same planes into
// the same adder), so iteration t's hard decisions are ~TV[v] plane 5 and need no table of their
// own: check phase t + 1 XORs them over each check's real edges into syndrome word U[t].
// EW: the early-stop build that also keeps each codeword's hard decisions at its stop iteration
// (DESIGN 3.9), a build of its own beside the ES build.  A lane holds up to VPL variables and the
// C5 build has no register to carry a word for each through the loop, so the lane that owns a
// variable ORs into the pack's row in global memory: zero at the start, hd_t & nn on the few
// iterations where codewords stop, hd_{T-1} & ~done in the last variable phase.  The ORs are
// atomics without a return value, so no wave waits for memory inside the loop.
// L8: the LLRs read as int8 grid values (a.llr points at bytes; as bsl's L8 build);
// with ES / EW the int8 builds of the early-stop kernels
template <int D, int DVH, int DVL, int LPC, int VPL, int CPL, int WPE, bool XP, int LB, bool MIX, bool B1, bool Q8,
          bool ES = false, bool EW = false, bool L8 = false>
__global__ void __launch_bounds__(LB) __attribute__((amdgpu_waves_per_eu(WPE)))
k_bsc(std::conditional_t<ES, std::conditional_t<EW, BscArgsEw, BscArgsEs>, std::conditional_t<XP, BscArgsXp, BscArgs>> a) {
    static_assert(!ES || (B1 && !XP), "early stop: the beta = 1 build, no export");
    static_assert(!EW || ES, "the stop-iteration word: early-stop builds");
    static_assert(!L8 || !Q8, "int8 LLRs: the decode, export and early-stop builds");
    constexpr int SB = (DVH * QMAX + QMAX <= 127) ? 8 : 9;
    constexpr int EPL = (D + LPC - 1) / LPC;
    constexpr int VNW = DVH + 1;
    constexpr int CVW = (EPL + 1) / 2;
    // plane counts below the place's that get a copy of the variable phase (1 seven, 2 eight):
    // both, on every instance
    constexpr int SBSET = 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if ((uint32_t)(uintptr_t)smem != 0u) __builtin_trap();          // LDS-absolute addresses
    const int tid = threadIdx.x;
    const int NT = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwv = NT >> 6;
    const int nv = a.n_vars;
    const int64_t b0 = (int64_t)blockIdx.x * PACK;
    const int nvalid = (int)min<int64_t>(PACK, a.B - b0);
    const uint32_t valid = (nvalid >= 32) ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);
    uint32_t* RED = reinterpret_cast<uint32_t*>(smem + a.off_red);
    const int flor = 16 + ((a.T + 3) & ~3);                         // the FLORW OR words
    const int AL = a.arows * LUT_W, BL = a.bcols * BLUT_W;
    uint32_t* ALUT = reinterpret_cast<uint32_t*>(smem + a.off_alut);
    uint32_t* BLUT = reinterpret_cast<uint32_t*>(smem + a.off_blut);

    // ---- per-lane variables ------------------------------------------------------------------
    uint32_t va[VPL][DVH];
    int vv[VPL], dw[VPL], dwmin[VPL];
    uint32_t tab_b[VPL];
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
        const int dvu = u == 0 ? DVH : DVL;
        const uint32_t* vt = a.vn_tab + ((size_t)u * NT + tid) * VNW;
#pragma unroll
        for (int p = 0; p < DVH; ++p) va[u][p] = (p < dvu) ? vt[p] : 0u;
        vv[u] = (int)vt[DVH];                                // v | Tv index << 16, or -1
        dw[u] = __builtin_amdgcn_readfirstlane(a.vn_wdeg[2 * (u * nwv + wave)]);
        dwmin[u] = __builtin_amdgcn_readfirstlane(a.vn_wdeg[2 * (u * nwv + wave) + 1]);
        tab_b[u] = (!B1 && a.bcols > 1 && vv[u] >= 0) ? (uint32_t)(((vv[u] & 0xFFFF) / (nv / a.bcols)) * BLUT_W * 4) : 0u;
    }
    (void)dwmin;

    // ---- channel planes (as bsl: shortened bits = +-cu decoded here, other off-grid packs
    // flagged for the v5 fixup) --------------------------------------------------------------
    // one workgroup per CU: the first generation starts in lockstep, and with every pack taking
    // the same time, each later generation again fetches its LLR blocks in one chip-wide burst
    // while HBM idles the rest of the pack.  Spreading the first starts over a pack's duration
    // keeps the fetches apart for the whole grid (later workgroups inherit the offsets).
    if (a.stagger > 0 && (int)blockIdx.x < a.stagger_n) {
        const int n = (int)(((uint32_t)blockIdx.x * 97u % (uint32_t)a.stagger_n) * (uint32_t)a.stagger /
                            (uint32_t)a.stagger_n);
        for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(8);
    }
    if (tid == 0) RED[7] = 0u;
    if constexpr (Q8) gen_tables(a.gen, tid, NT);
    __syncthreads();
    uint32_t cs[VPL], cm[VPL][4], bg[VPL];
    int off = 0;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
        cs[u] = 0u;
        bg[u] = 0u;
#pragma unroll
        for (int p = 0; p < 4; ++p) cm[u][p] = 0u;
        const int v = vv[u] < 0 ? -1 : (vv[u] & 0xFFFF);
        if (Q8 && v >= 0) {                        // generated channel (ldpc_decode_awgn), a build of its own
            uint32_t Dq[8];
            gen_bytes(a.gen, blockIdx.x, v, a.qmax, Dq);
            pack_bytes<true>(Dq, valid, cs[u], cm[u], bg[u]);
        } else if (L8 && v >= 0) {
            // int8 LLRs (ldpc_decode_q8): a descriptor over the pack's valid rows, one byte per LLR
            // (a row past the batch takes the last valid row's offset: masked by pack_bytes, and no
            // load leaves the pack's rows); four rows per word, converted by
            // l8_bytes (ldpc_bitplane.h); an invalid byte in a row of the pack marks the pack
            const __amdgpu_buffer_rsrc_t l8_rs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(reinterpret_cast<const uint8_t*>(a.llr) + b0 * nv), 0, nvalid * nv, 0x00020000);
            uint32_t by[PACK], Dk[8];
#pragma unroll
            for (int r = 0; r < PACK; ++r)
                by[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(l8_rs, v, min(r, nvalid - 1) * nv, 0);
            uint32_t l8_bad = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                uint32_t iv;
                Dk[i] = l8_bytes(by[4 * i] | by[4 * i + 1] << 8 | by[4 * i + 2] << 16 | by[4 * i + 3] << 24, a.qmax,
                                 a.cu > 0.f, iv);
                l8_bad |= l8_invalid(iv, valid >> (4 * i));
            }
            off |= l8_bad != 0u;
            pack_bytes<true>(Dk, valid, cs[u], cm[u], bg[u]);
        } else if (v >= 0) {
            // (buffer loads: a wave-uniform descriptor over the pack's rows, the lane's 4 v in
            // voffset, the row's 4 r nv in soffset: no 64-bit VGPR address per load, as bsl)
            const __amdgpu_buffer_rsrc_t llr_rs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(a.llr + b0 * nv), 0, nvalid * nv * 4, 0x00020000);
            float xv[PACK];
#pragma unroll
            for (int r = 0; r < PACK; ++r)
                xv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(llr_rs, 4 * v, 4 * r * nv, 0));
            off |= pack_channel<true>(xv, a.inv, a.qmax, a.cu, valid, cs[u], cm[u], bg[u]);
        }
    }
    if (off) atomicOr(&RED[7], 1u);
    __syncthreads();
    if (RED[7]) {
        if constexpr (ES) {
            // early stop: no fixup; the pack's frames are marked undecoded and enter neither the
            // counters nor the histogram
            if (tid < nvalid) {
                if (a.flags) a.flags[b0 + tid] = 0x80;
                if (a.n_iter) a.n_iter[b0 + tid] = 0;
            }
        }
        if constexpr (L8 && !ES) {
            // int8 LLRs: an invalid byte has no float decode to fall back to; marked the same way
            // (the early-stop int8 builds: by the block above, once)
            if (tid < nvalid && a.flags) a.flags[b0 + tid] = 0x80;
        }
        if (tid == 0) a.bad[blockIdx.x] = 1u;
        return;
    }
    if (tid == 0) a.bad[blockIdx.x] = 0u;
    // (EW: the pack's row of stop-iteration hard decisions starts from zero; the barriers before
    // the loop retire these stores)
    // (the row's address is taken from the kernel arguments at each use, scalar loads, not held
    // through the loop)
    [[maybe_unused]] auto hdw_row = [&]() __attribute__((always_inline)) -> uint32_t* {
        uint32_t* h = kern_args<BscArgsEw>().hdw;
        return h ? h + (size_t)blockIdx.x * (size_t)kern_args<BscArgsEw>().n_vars : nullptr;
    };
    if constexpr (EW) {
        if (uint32_t* row = hdw_row()) {
#pragma unroll
            for (int u = 0; u < VPL; ++u)
                if (vv[u] >= 0) row[vv[u] & 0xFFFF] = 0u;
        }
    }
    // the zero edge / zero record (padding edges of the variable lanes), counters, tables
    if (tid < 8)
        reinterpret_cast<uint32_t*>(smem + a.off_rec + rec_off((uint32_t)a.n_checks) + (tid >> 2) * REC_Q2)[tid & 3] = 0u;
    if (tid < 8) RED[tid] = (tid == 1) ? 0xFFFFFFFFu : 0u;
    if (tid < FLORW) RED[flor + tid] = 0u;
    // early stop: the done word (wave-uniform, every wave its own copy: a codeword's bit is set once
    // an iteration's hard decisions had a zero syndrome; the bits past the pack's codewords start
    // set, so a ragged pack's padding never holds the pack back) and the T syndrome words, zeroed
    [[maybe_unused]] uint32_t es_done = ~valid;
    if constexpr (ES) {
        for (int w = tid; w < a.T; w += NT) (RED + ((a.off_u - a.off_red) >> 2))[w] = 0u;
    }
    for (int w = tid; w < AL; w += NT) ALUT[w] = a.alut[w];
    for (int w = tid; w < BL; w += NT) BLUT[w] = a.blut[w];
    __syncthreads();

    // ---- variable phase --------------------------------------------------------------------
    //   S = sum of the C->V (SGN, ARG ? q2 : q1), APP_t = Q(ch) + S (hard decision, counters);
    //   unless last, TV[v] = clamp(Q(beta_{t+1} ch) + S)
    auto vn_phase = [&](const bool first, const bool last, const uint32_t bslice, const int tb)
                        __attribute__((always_inline)) {
        uint32_t wr = 0u, apos = 0u, nb = 0u;
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
            const int dvu = u == 0 ? DVH : DVL;
            if (dw[u] < 0) continue;   // no variable chunk at this (wave, u) place
            // (the edge words made opaque per use, as bsl: without it the build spills more)
#pragma unroll
            for (int p = 0; p < DVH; ++p)
                if (p < dvu) asm volatile("" : "+v"(va[u][p]));
            const int v = vv[u] < 0 ? -1 : (vv[u] & 0xFFFF);
            const bool counted = v >= 0 && v < a.target_bits;
            uint32_t lw[1][4];
            if (!last) {
                if (B1 || a.beta_id) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) lw[0][i] = cm[u][i];
                } else if (a.bcols == 1) {
                    const ConstW* tg = (const ConstW*)(a.blut) + (size_t)tb * BLUT_W;
                    lut_s(lw[0], cm[u], tg);
#pragma unroll
                    for (int i = 0; i < 4; ++i) lw[0][i] = mux(bg[u], tg[LUT_W + i], lw[0][i]);
                } else {
                    const uint32_t btab = bslice + tab_b[u];
                    const uint32_t cmi[1][4] = {{cm[u][0], cm[u][1], cm[u][2], cm[u][3]}};
                    lut<1>(lw, cmi, btab);
                    const v4u gb = lds_q(btab + LUT_W * 4);
                    lw[0][0] = mux(bg[u], gb.x, lw[0][0]);
                    lw[0][1] = mux(bg[u], gb.y, lw[0][1]);
                    lw[0][2] = mux(bg[u], gb.z, lw[0][2]);
                    lw[0][3] = mux(bg[u], gb.w, lw[0][3]);
                }
            }
            const int dwu = dw[u];
            [[maybe_unused]] uint32_t hl = 0u;    // (EW: the variable's hard decisions, for the merge below)
            // the rest at SBX planes of S: the fewest that hold 15 dw + 15 for the place's largest
            // degree (as bsl; the places past the first hold at most DVL edges)
            auto vbody = [&](auto sbc) __attribute__((always_inline)) {
                constexpr int SB = decltype(sbc)::value;
                uint32_t S[SB];
#pragma unroll
                for (int i = 0; i < SB; ++i) S[i] = 0u;
                if (!first) {
#pragma unroll
                    for (int f = 0; f < DVH; ++f) {
                        if (f < dvu && f < dwu) {
                            const uint32_t wd = va[u][f];
                            const uint32_t sa = (wd & 0xFFFFu) << 2;
                            const uint32_t ra = a.off_rec + ((wd >> 16) << 4);
                            const uint32_t n = lds_w(sa), am = lds_w(sa + a.off_a);
                            const v4u q1 = lds_q(ra), q2 = lds_q(ra + REC_Q2);
                            uint32_t b[4];
                            b[0] = mux(am, q2.x, q1.x) ^ n;
                            b[1] = mux(am, q2.y, q1.y) ^ n;
                            b[2] = mux(am, q2.z, q1.z) ^ n;
                            b[3] = mux(am, q2.w, q1.w) ^ n;
                            if (f == 0) set_b<SB>(S, b, n);
                            else add_b<SB>(S, b, n);
                        }
                    }
                    uint32_t hd, nz = 0u;
                    const uint32_t c_s = cs[u];
                    if (last) {
                        uint32_t A[SB];
#pragma unroll
                        for (int i = 0; i < SB; ++i) A[i] = S[i];
                        const uint32_t cb[4] = {cm[u][0] ^ c_s, cm[u][1] ^ c_s, cm[u][2] ^ c_s, cm[u][3] ^ c_s};
                        add_b<SB>(A, cb, c_s);
                        hd = ~A[SB - 1];
#pragma unroll
                        for (int i = 0; i < SB; ++i) nz |= A[i];
                    } else {
                        uint32_t c = c_s;
#pragma unroll
                        for (int i = 0; i < SB - 1; ++i) c = B3(T_MAJ, S[i], i < 4 ? (cm[u][i] ^ c_s) : c_s, c);
                        hd = B3(T_XNOR3, S[SB - 1], c_s, c);
                    }
                    hd &= valid;
                    if constexpr (XP) {                              // iteration tb - 1's hard decisions
                        // (word mode, wave-uniform: the last iteration's alone, one row per pack)
                        const size_t row = a.word ? (size_t)blockIdx.x : (size_t)(tb - 1) * (size_t)((a.B + 31) >> 5) + blockIdx.x;
                        if (v >= 0 && (last || !a.word)) a.hdx[row * nv + v] = hd;
                    }
                    if (counted) {
                        wr |= hd;
                        if (last) {
                            apos |= hd & nz;
                            // (early stop: the codewords not done before count from iteration T - 1)
                            if constexpr (ES) nb += (uint32_t)__popc(hd & ~es_done);
                            else nb += (uint32_t)__popc(hd);
                        }
                    }
                    if constexpr (EW) hl = hd;
                }
                if (last || v < 0) return;
                uint32_t lb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) lb[i] = lw[0][i] ^ cs[u];
                add_b<SB>(S, lb, cs[u]);
                uint32_t Tv[6];
                clamp6<SB>(Tv, S);
                const uint32_t ta = a.off_tv + 24u * ((uint32_t)vv[u] >> 16);     // the Tv index
                lds_dput(ta, Tv[0], Tv[1]);
                lds_dput(ta + 8, Tv[2], Tv[3]);
                lds_dput(ta + 16, Tv[4], Tv[5]);
            };
            auto dispatch = [&](auto smax) __attribute__((always_inline)) {
                constexpr int SM = decltype(smax)::value;
                if ((SBSET & 1) && dwu * QMAX + QMAX <= 63) vbody(std::integral_constant<int, 7>{});
                else if ((SBSET & 2) && SM == 9 && dwu * QMAX + QMAX <= 127)
                    vbody(std::integral_constant<int, (SM == 9 ? 8 : SM)>{});
                else vbody(std::integral_constant<int, SM>{});
            };
            constexpr int SBL = (DVL * QMAX + QMAX <= 127) ? 8 : 9;    // places past the first
            if (u == 0) dispatch(std::integral_constant<int, SB>{});
            else dispatch(std::integral_constant<int, SBL>{});
            // (EW: the codewords that never stopped keep iteration T - 1's decisions)
            if constexpr (EW) {
                if (last && v >= 0 && (hl & ~es_done)) {
                    if (uint32_t* row = hdw_row())
                        __hip_atomic_fetch_or(row + v, hl & ~es_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (!first && !last) {               // (as bsl: one ds_or per lane into the FLORW words)
            const uint32_t la = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 31u;
            __hip_atomic_fetch_or(RED + flor + la, wr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (!first) {
            wr = wave_or(wr);
            if (last) {
                apos = wave_or(apos);
                nb = wave_add(nb);
            }
            if (lane == 0) {
                if (wr) atomicOr(&RED[0], wr);
                if (last) {
                    if (apos) atomicOr(&RED[2], apos);
                    if (nb) atomicAdd(&RED[3], nb);
                }
            }
        }
    };

    vn_phase(true, false, a.off_blut, 0);
    // check groups (as bsl): lane LPC c + j of a chunk takes edges k = LPC m + j of check c
    // (MIX: each chunk's lanes per check from its lane map; lane 0 of a chunk always holds a check)
    int gchunk[CPL], gdeg[CPL], gm[CPL], gl4[CPL];
    uint32_t gslot[CPL], grec[CPL], gtab[CPL], gvar[CPL][CVW];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        gchunk[c] = __builtin_amdgcn_readfirstlane(a.cn_chunk[wave * CPL + c]);
        const int ql = max(gchunk[c], 0) * 64 + lane;
        int cc, cjc, Lc = LPC;
        gl4[c] = 1;
        if constexpr (MIX) {
            const int32_t d = gchunk[c] >= 0 ? a.cn_lane[ql] : -1;
            cc = d < 0 ? a.n_checks : (d & 0xFFFF);
            cjc = d < 0 ? 0 : ((d >> 16) & 15);
            gl4[c] = __builtin_amdgcn_readfirstlane(d < 0 ? LPC : ((d >> 20) & 15)) == LPC ? 1 : 0;
            Lc = gl4[c] ? LPC : LPC / 2;
        } else {
            cc = ql / LPC;
            cjc = lane % LPC;
        }
        const int ci = min(cc / a.z, a.n_checks / a.z - 1);
        gdeg[c] = (cc < a.n_checks) ? a.row_ptr[ci + 1] - a.row_ptr[ci] : 0;
        // edge positions m holding a real edge for some lane of the chunk (wave-uniform): the
        // positions past them are padding for every lane and skipped (LPC, an even count, lanes
        // of each group skip together, so the group's [V->C >= 0] parity is unchanged)
        gm[c] = __popc(wave_or((1u << ((gdeg[c] + Lc - 1) / Lc)) - 1u));
        (void)nwv;
        gslot[c] = (uint32_t)(4 * (a.row_lay[2 * ci] + cjc * a.row_lay[2 * ci + 1] + (cc - ci * a.z)));
        grec[c] = a.off_rec + rec_off((uint32_t)min(cc, a.n_checks - 1));
        gtab[c] = a.off_alut + (uint32_t)((a.arows > 1 ? ci : 0) * LUT_W * 4) + (uint32_t)(cjc * (4 / Lc) * 64);
#pragma unroll
        for (int p = 0; p < CVW; ++p) gvar[c][p] = gchunk[c] >= 0 ? a.cn_var[(size_t)ql * CVW + p] : 0u;
    }
    const uint32_t sstride = (uint32_t)(4 * a.z);
    // the lane's real edge positions, one word for all its chunks: bit RB c + m = position m of
    // chunk c holds an edge of the lane's check, bit RB c + EPL = the lane holds a check.  Read
    // through an opaque copy per iteration, so [L m + j < degree] is not hoisted out of the T
    // loop as CPL x EPL x 2 64-bit lane masks, whose SGPR pairs the loop spilled and reloaded by
    // v_readlane (C5: 166 reloads in the loop body)
    constexpr int RB = EPL + 1;                  // bits per chunk
    static_assert(CPL * RB <= 32, "real-position word");
    uint32_t rpk = 0u;
    {
        const int cn_dmin = a.cn_dmin;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int L = (!MIX || gl4[c]) ? LPC : LPC / 2;
            const int cjl = lane & (L - 1);
#pragma unroll
            for (int m = 0; m < EPL; ++m)
                if (L * m + L - 1 < cn_dmin || L * m + cjl < gdeg[c]) rpk |= 1u << (RB * c + m);
            if (gdeg[c] > 0) rpk |= 1u << (RB * c + EPL);
        }
    }
    __syncthreads();

    for (int t = 0; t < a.T; ++t) {
        if (wave == 0 && t > 0) {               // (all lanes of wave 0, the same words: bsl)
            // (the FLORW words of iteration t - 1, zeroed again)
            const uint32_t ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const uint32_t x = ln < 32u ? RED[flor + ln] : 0u;
            if (ln < 32u) RED[flor + ln] = 0u;
            const uint32_t w0 = wave_or(x);
            RED[16 + t - 1] = w0;                    // (exported after the loop)
            RED[1] &= w0;
        }
        const int nx = (t + 1) & 1;
#pragma unroll
        for (int u = 0; u < VPL; ++u) asm volatile("" : "+s"(dw[u]));
        // (the lane's variables opaque per iteration: [v >= 0], [v < target bits] compared per
        // use, not held through the loop as spilled lane masks; as bsl)
#pragma unroll
        for (int u = 0; u < VPL; ++u) asm volatile("" : "+v"(vv[u]));
        uint32_t rp = rpk;
        asm volatile("" : "+v"(rp));
        if (t + 1 < a.T) {            // (async global -> LDS, retired by the next barrier: bsl)
            copy_async(a.off_alut + 4u * (uint32_t)(nx * AL), a.alut + (size_t)(t + 1) * AL, AL, wave, NT);
            if (a.bcols > 1)
                copy_async(a.off_blut + 4u * (uint32_t)(nx * BL), a.blut + (size_t)(t + 1) * BL, BL, wave, NT);
        }
        // ======== check nodes ===================================================================
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            if (gchunk[c] < 0) continue;
            // the chunk's check work at L lanes per check (MIX: L = LPC / 2 for the low-degree rows)
            auto chunk = [&](auto LC) __attribute__((always_inline)) {
            constexpr int L = decltype(LC)::value;
            constexpr int OBL = 4 / L;
            const int cjl = lane & (L - 1);
            int gmc = gm[c];
            asm volatile("" : "+s"(gmc));
            uint32_t sbase = gslot[c];
            asm volatile("" : "+v"(sbase));
            auto real = [&](int m) __attribute__((always_inline)) -> bool {
                return ((rp >> (RB * c + m)) & 1u) != 0u;
            };
            const bool has_check = ((rp >> (RB * c + EPL)) & 1u) != 0u;
            // V->C = clamp(Tv - C->V_old, +-15) of the lane's edges (padding: negative, 15)
            v4u q1o = {0u, 0u, 0u, 0u}, q2o = {0u, 0u, 0u, 0u};
            if (t > 0) {
                q1o = lds_q(grec[c]);
                q2o = lds_q(grec[c] + REC_Q2);
            }
            uint32_t Xs[EPL][4], ns[EPL];
            // early stop: the lane's share of its check's syndrome of iteration t - 1's hard
            // decisions (~Tv plane 5), over its real edge positions only
            [[maybe_unused]] uint32_t syn = 0u;
#pragma unroll
            for (int m = 0; m < EPL; ++m) {
                if (m >= gmc) {                      // padding for the whole chunk
#pragma unroll
                    for (int i = 0; i < 4; ++i) Xs[m][i] = ~0u;
                    ns[m] = ~0u;
                    continue;
                }
                const uint32_t vw = gvar[c][m >> 1];
                const uint32_t vi = (m & 1) ? (vw >> 16) : (vw & 0xFFFFu);
                const uint32_t ta = a.off_tv + 24u * vi;
                const v2u t01 = lds_d(ta), t23 = lds_d(ta + 8), t45 = lds_d(ta + 16);
                const uint32_t Tv[6] = {t01.x, t01.y, t23.x, t23.y, t45.x, t45.y};
                uint32_t x[7];
                if (t == 0) {
#pragma unroll
                    for (int i = 0; i < 7; ++i) x[i] = Tv[i < 6 ? i : 5];
                } else {
                    const uint32_t sa = sbase + m * sstride;
                    const uint32_t so = lds_w(sa), ao = lds_w(sa + a.off_a);
                    uint32_t bo[4];
                    bo[0] = mux(ao, q2o.x, q1o.x) ^ so;
                    bo[1] = mux(ao, q2o.y, q1o.y) ^ so;
                    bo[2] = mux(ao, q2o.z, q1o.z) ^ so;
                    bo[3] = mux(ao, q2o.w, q1o.w) ^ so;
                    sub_tv(x, Tv, bo, so);
                }
                abs_sat(Xs[m], x);
                ns[m] = x[6];
                if constexpr (ES) {
                    if (t > 0 && real(m)) syn ^= ~Tv[5];
                }
                if (!real(m)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) Xs[m][i] = ~0u;
                    ns[m] = ~0u;
                }
            }
            if constexpr (ES) {
                // merged over the check's lanes as par; the lanes that hold a check OR theirs into
                // syndrome word t - 1 (one LDS atomic per wave and chunk)
                if (t > 0) {
                    syn ^= qperm<QP_X1>(syn);
                    if (L == 4) syn ^= qperm<QP_X2>(syn);
                    const uint32_t wu = wave_or(has_check ? syn : 0u);
                    if (wu && lane == 0)
                        __hip_atomic_fetch_or((RED + ((a.off_u - a.off_red) >> 2)) + (t - 1), wu,
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            // two minima by the bit-serial search of bsl (min2_bits) over the chunk's real positions
            // (1 <= gmc <= EPL for an active chunk: the other counts are marked unreachable);
            // positions past the chunk's bound hold the all-ones padding, whose sign word, XORed
            // by all L lanes of the group, leaves the parity unchanged
            uint32_t m1[4], m2[4];
            uint32_t cand[EPL];
            uint32_t par = ns[0] ^ ns[1];
#pragma unroll
            for (int m = 2; m < EPL; ++m) par ^= ns[m];
            switch (gmc) {
#define BSC_MIN2_CASE(k)                                                                           \
    case k:                                                                                        \
        if constexpr (k <= EPL) {                                                                  \
            min2_bits<k, L>(m1, m2, cand, Xs);                                                     \
            _Pragma("unroll") for (int m = k; m < EPL; ++m) cand[m] = 0u;                          \
        } else {                                                                                   \
            __builtin_unreachable();                                                               \
        }                                                                                          \
        break;
                BSC_MIN2_CASE(1) BSC_MIN2_CASE(2) BSC_MIN2_CASE(3) BSC_MIN2_CASE(4) BSC_MIN2_CASE(5)
                BSC_MIN2_CASE(6) BSC_MIN2_CASE(7) BSC_MIN2_CASE(8) BSC_MIN2_CASE(9) BSC_MIN2_CASE(10)
#undef BSC_MIN2_CASE
                default:
                    __builtin_unreachable();
            }
            par ^= qperm<QP_X1>(par);
            if (L == 4) par ^= qperm<QP_X2>(par);
            // weighted, quantized minima (Main_Functions.py:266-316)
            uint32_t qb[OBL][2];
            {
                const uint32_t mm[2][4] = {{m1[0], m1[1], m1[2], m1[3]}, {m2[0], m2[1], m2[2], m2[3]}};
                const uint32_t tab = gtab[c] + (uint32_t)((t & 1) * AL * 4);
#pragma unroll
                for (int b = 0; b < OBL; ++b) {
                    uint32_t o[2];
                    lut_bit<2>(o, mm, tab + (uint32_t)(b * 64));
                    qb[b][0] = o[0];
                    qb[b][1] = o[1];
                }
            }
            // the record: lane j writes planes OBL j .. of q1 and q2 (the whole group has read the
            // old record above: same wave, LDS operations in program order); idle lanes past
            // the last check (degree 0) share its clamped record address and must not write
            if (has_check) {
#pragma unroll
                for (int b = 0; b < OBL; ++b) {
                    lds_put(grec[c] + 4u * (uint32_t)(OBL * cjl + b), qb[b][0]);
                    lds_put(grec[c] + REC_Q2 + 4u * (uint32_t)(OBL * cjl + b), qb[b][1]);
                }
            }
            // per edge: the C->V sign (par ^ own V->C sign, :251-254) and [|V->C| == min]
#pragma unroll
            for (int m = 0; m < EPL; ++m) {
                if (real(m)) {
                    const uint32_t sa = sbase + m * sstride;
                    lds_put(sa, par ^ ns[m]);
                    lds_put(sa + a.off_a, cand[m]);
                }
            }
                    };
            if (!MIX || gl4[c]) chunk(std::integral_constant<int, LPC>{});
            else if constexpr (MIX) chunk(std::integral_constant<int, LPC / 2>{});
        }
        __syncthreads();
        if constexpr (ES) {
            // ======== early stop ================================================================
            // syndrome word t - 1 is complete (the barrier): the codewords newly done at iteration
            // t - 1 are those with no unsatisfied check that were not done before.  Their bit
            // errors are counted from TV, which still holds iteration t - 1's value; once every
            // codeword is done the workgroup leaves the loop (every wave reads the same word: a
            // workgroup-uniform branch; the barrier retired the async table copies).
            if (t > 0) {
                const uint32_t un = (uint32_t)__builtin_amdgcn_readfirstlane(
                    (int)(RED + ((a.off_u - a.off_red) >> 2))[t - 1]);
                const uint32_t nn = ~un & ~es_done;
                es_done |= nn;
                if (nn) {
                    uint32_t nb = 0u;
#pragma unroll
                    for (int u = 0; u < VPL; ++u) {
                        const int v = vv[u] < 0 ? -1 : (vv[u] & 0xFFFF);
                        if constexpr (EW) {
                            // (every real variable's decisions, not the target bits' alone)
                            if (v >= 0) {
                                const uint32_t h = ~lds_w(a.off_tv + 24u * ((uint32_t)vv[u] >> 16) + 20u) & nn;
                                if (h) {
                                    if (uint32_t* row = hdw_row())
                                        __hip_atomic_fetch_or(row + v, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                }
                                if (v < a.target_bits) nb += (uint32_t)__popc(h);
                            }
                        } else
                        if (v >= 0 && v < a.target_bits)
                            nb += (uint32_t)__popc(~lds_w(a.off_tv + 24u * ((uint32_t)vv[u] >> 16) + 20u) & nn);
                    }
                    nb = wave_add(nb);
                    if (nb && lane == 0) atomicAdd(&RED[3], nb);
                }
                if (es_done == 0xFFFFFFFFu) break;
            }
        }
        // ======== variable nodes ================================================================
        const uint32_t bslice = a.off_blut + (uint32_t)(nx * BL * 4);
        if (t == a.T - 1) vn_phase(false, true, bslice, t + 1);
        else vn_phase(false, false, bslice, t + 1);
        __syncthreads();
    }
    if constexpr (ES) {
        // early stop: each codeword's outputs at its own stop iteration -- the first t whose
        // syndrome word has its bit clear, else T - 1 -- from the syndrome words and the
        // per-iteration frame-error words (RED[16 + t]; iteration T - 1's is RED[0]); one lane of
        // wave 0 per codeword, as the bsl build.  (The words past the iteration the pack left the
        // loop at are not used: every codeword has stopped by then.)
        __syncthreads();                 // the bit counts of the waves that left the loop
        if (wave == 0) {
            const uint32_t* U = (RED + ((a.off_u - a.off_red) >> 2));
            const int r = tid & 31;
            const bool on = tid < nvalid;
            int stop = a.T - 1;
            uint32_t all = 1u, wl = 0u;
            bool open = true;
            for (int t = 0; t < a.T; ++t) {
                const bool lastt = t == a.T - 1;
                const uint32_t w = lastt ? RED[0] : RED[16 + t];
                const uint32_t u = lastt ? 0u : U[t];
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
                if (a.flags) a.flags[b0 + tid] = (uint8_t)(all | (wl << 1));
                if (a.n_iter) a.n_iter[b0 + tid] = (uint8_t)(stop + 1);
            }
            if (tid == 0 && a.counters) {
                unsigned long long* cc = reinterpret_cast<unsigned long long*>(a.counters);
                const unsigned long long c0 = RED[3], c1 = __popcll(mw), c2 = __popcll(ma);
                if (c0) atomicAdd(cc + 0, c0);
                if (c1) atomicAdd(cc + 1, c1);
                if (c2) atomicAdd(cc + 2, c2);
            }
            if (a.iter_hist) {                  // one atomic per distinct stop iteration of the pack
                unsigned long long rem = __builtin_amdgcn_ballot_w64(on);
                while (rem) {
                    const int l = __builtin_ctzll(rem);
                    const int ts = __builtin_amdgcn_readlane(stop, l);
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(on && stop == ts);
                    if (tid == l)
                        atomicAdd(reinterpret_cast<unsigned long long*>(a.iter_hist) + ts,
                                  (unsigned long long)__popcll(m));
                    rem &= ~m;
                }
            }
        }
    }
    if constexpr (!ES) {
    // (the body keeps the indentation it had before the early-stop builds)
    if (tid == 0) {
        const uint32_t wl = RED[0] & valid;
        const uint32_t all = RED[1] & RED[0] & valid;
        const uint32_t ap = RED[2] & valid;
        RED[16 + a.T - 1] = RED[0];
        if (a.counters) {
            unsigned long long* cc = reinterpret_cast<unsigned long long*>(a.counters);
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
    if (a.flags || a.iter_wrong) {
        __syncthreads();
        if (a.flags && tid < nvalid)
            a.flags[b0 + tid] = (uint8_t)(((RED[5] >> tid) & 1) | (((RED[6] >> tid) & 1) << 1));
        if (a.iter_wrong)
            for (int t = tid; t < a.T; t += NT)
                a.iter_wrong[(size_t)t * (size_t)((a.B + 31) >> 5) + blockIdx.x] = RED[16 + t] & valid;
    }
    }
}

}  // namespace bs
}  // namespace ldpc

// ---- host: planning, graph tables, launch -------------------------------------------------
namespace ldpc {
namespace bs {

constexpr int kBscNInst = sizeof(kBscInst) / sizeof(kBscInst[0]);
constexpr int BSC_NW = 16;
constexpr int BSC_TAG = 100;     // ws.bs_graph_inst of the bsc tables: BSC_TAG + instance

struct BscPlan {
    bool ok = false;
    int inst = -1, nw = BSC_NW, cn_lanes = 0, arows = 1, bcols = 1, cn_dmin = 0;
    float cu = -1.f;
    size_t nslot = 0;
    uint32_t off_a = 0, off_rec = 0, off_tv = 0, off_red = 0, off_alut = 0, off_blut = 0;
    bool es = false;               // an early-stop plan:
    uint32_t off_u = 0;            // its T syndrome words (in the RED region, after the FLORW words)
    size_t lds = 0;
    std::vector<int32_t> lay;
    std::vector<int> vorder, vslot;      // variables by degree; chunk of each (wave, u) place
    std::vector<int> rl;                 // lanes per check of each row
    std::vector<int32_t> lanes;          // check lane -> check | lane << 16 | lanes per check << 20, -1 idle
};

// The in-prologue channel (Q8 builds) copies the sampler's tables, 4 AWGN_TAB_W bytes, to LDS
// byte 0, into the SGN region: where the launch puts them (gen.lds) and the test of bsc_q8_ok
// that they fit.  bsc_debug_bounds holds both against the plan.
static uint32_t q8_tab_lds(const BscPlan&) { return 0u; }
static bool q8_tab_fits(const BscPlan& p) { return (size_t)p.off_a >= sizeof(uint32_t) * AWGN_TAB_W; }

// (LDPC_BSC_B1=0: the general channel path for a B1 decode too, an A/B switch)
static bool bsc_b1_on() {
    static const bool on = [] { const char* e = getenv("LDPC_BSC_B1"); return !(e && atoi(e) == 0); }();
    return on;
}
// the early-stop builds exist for these instances (on top of their B1 build)
static constexpr bool bsc_es_inst(int i) { return i == 3 || i == 4; }
// the instances with the int8-LLR builds: those the planner takes by default -- the
// mixed-lane ones where every beta is 1, the first entry otherwise; not the A/B-only entries 1, 2
static constexpr bool bsc_l8_inst(int i) { return i == 0 || i == 3 || i == 4; }

// es: the plan of an early-stop request.  Only a decode that takes the B1 build
// (every beta 1, one column table) on the instance the planner picks for it has such a build; the
// plan is that decode's with the T syndrome words added.  Every other request has no plan.
static BscPlan bsc_plan(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T,
                        bool es = false) {
    BscPlan p;
    const char* e = getenv("LDPC_BS");
    if (e && atoi(e) == 0) return p;
    if (!bs_mode(mode)) return p;
    if (ucn || per_edge_w || !g.host || !g.w_beta_nonneg) return p;
    if (es && !(g.w_beta_one && g.w_beta_uniform && bsc_b1_on())) return p;
    const host::GraphTables& h = *g.host;
    int min_cdeg = 1 << 30;
    for (int i = 0; i < h.M; ++i) min_cdeg = std::min(min_cdeg, h.row_ptr[i + 1] - h.row_ptr[i]);
    if (min_cdeg < 2) return p;
    const int nv = g.n_vars, nc = g.n_checks, z = h.z;
    const char* el = getenv("LDPC_BS_LPC");          // A/B: force 2 or 4 lanes per check
    const int want_lpc = el ? atoi(el) : 0;
    const char* ei = getenv("LDPC_BSC_INST");        // A/B: force one instance (if it fits)
    const int want_inst = ei ? atoi(ei) : -1;
    // the mixed-lane instances first (fewest check chunks per wave first) when the decode takes
    // the beta = 1 build (every beta 1, one column table: bsc_launch's B1), where they run without
    // spills: C5 53.86 -> 52.44 ms (r3zd).  With a beta table they spill 11-19 VGPRs and issue 7 %
    // fewer VALU instructions in the same time as the uniform ones (56.24-56.43 against 56.34 ms,
    // r3w; PMC r3 mixprof): the uniform instances stay the default there.  LDPC_BSC_MIX=0/1
    // forces either.
    const char* em = getenv("LDPC_BSC_MIX");
    const bool mix = em ? atoi(em) != 0 : (g.w_beta_one && g.w_beta_uniform);
    std::vector<int> order(kBscNInst);
    for (int i = 0; i < kBscNInst; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const int kx = kBscInst[x].MIX == mix ? 0 : 1, ky = kBscInst[y].MIX == mix ? 0 : 1;
        if (kx != ky) return kx < ky;
        return kBscInst[x].MIX && kBscInst[x].CPL < kBscInst[y].CPL;
    });
    for (const int i : order) {
        const BscInst& k = kBscInst[i];
        if (h.max_cdeg > k.D || h.max_vdeg > k.DVH) continue;
        if (want_lpc != 0 && want_lpc != k.LPC) continue;
        if (want_inst >= 0 && want_inst != i) continue;
        if (want_inst < 0 && k.NW != BSC_NW) continue;          // A/B-only instances
        BscPlan q;
        q.inst = i;
        q.nw = k.NW;
        // rows and check lanes: MIX instances give the rows of degree <= LPC / 2 * EPL half the
        // lanes, in 64-lane chunks of their own after the full-width rows' chunks
        const int EPLk = (k.D + k.LPC - 1) / k.LPC;
        q.rl.assign((size_t)h.M, k.LPC);
        if (k.MIX)
            for (int i = 0; i < h.M; ++i)
                if (h.row_ptr[i + 1] - h.row_ptr[i] <= k.LPC / 2 * EPLk) q.rl[(size_t)i] = k.LPC / 2;
        if (k.MIX) {
            for (const int L : {k.LPC, k.LPC / 2}) {
                for (int i = 0; i < h.M; ++i) {
                    if (q.rl[(size_t)i] != L) continue;
                    for (int hc = 0; hc < z; ++hc)
                        for (int j = 0; j < L; ++j) q.lanes.push_back((i * z + hc) | (j << 16) | (L << 20));
                }
                while (q.lanes.size() % 64) q.lanes.push_back(-1);
            }
            q.cn_lanes = (int)q.lanes.size();
        } else {
            q.cn_lanes = 64 * ((k.LPC * nc + 63) / 64);
            q.lanes = uniform_lanes(h, k.LPC, q.cn_lanes);
        }
        const int vch = (nv + 63) / 64, cch = q.cn_lanes / 64;
        if (k.VPL == 1 && k.CPL == 1) q.nw = std::max(vch, cch);
        if (q.nw > 16 || vch > k.VPL * q.nw || cch > k.CPL * q.nw) continue;
        if (nv > 65535 || nc >= 65535) continue;
        // variables by descending degree in 64-chunks, dealt to (wave, u) places (the first
        // chunk of each wave, u = 0, takes the heaviest: only there may a degree exceed DVL)
        q.vorder.resize(nv);
        for (int v = 0; v < nv; ++v) q.vorder[v] = v;
        auto vdeg = [&](int v) { const int j = v / z; return h.col_ptr[j + 1] - h.col_ptr[j]; };
        std::stable_sort(q.vorder.begin(), q.vorder.end(), [&](int x, int y) { return vdeg(x) > vdeg(y); });
        std::vector<int> cost(vch);
        for (int ch = 0; ch < vch; ++ch) cost[ch] = 3 + vdeg(q.vorder[64 * ch]);
        q.vslot = deal_chunks(cost, q.nw, k.VPL);
        bool fits = true;
        for (int w = 0; w < q.nw; ++w)
            for (int u = 1; u < k.VPL; ++u) {
                const int ch = q.vslot[(size_t)w * k.VPL + u];
                if (ch >= 0 && vdeg(q.vorder[64 * ch]) > k.DVL) fits = false;
            }
        if (!fits) continue;
        q.arows = g.w_alpha_uniform ? 1 : h.M;
        q.bcols = g.w_beta_uniform ? 1 : h.N;
        q.cn_dmin = (!k.MIX && q.cn_lanes == k.LPC * nc) ? min_cdeg : 0;
        const float cu = clip / bs_step(mode);
        q.cu = cu > (float)bs_qmax(mode) ? cu : -1.f;
        q.lay = slot_layout_rows(h, q.rl, &q.nslot);
        // LDS: SGN [nslot + 1] | ARG [nslot + 1] | REC [(nc + 1) / 16 blocks][2][16][4] | TV [nv][6] |
        // RED | ALUT | BLUT
        const size_t sgn = ((q.nslot + 1) * 4 + 127) & ~(size_t)127;
        if (q.nslot + 1 > 65535) continue;
        if (nv > 32767) continue;                // v | Tv index << 16 as a non-negative int
        q.off_a = (uint32_t)sgn;
        size_t o = 2 * sgn;
        q.off_rec = (uint32_t)o;
        o += (size_t)((nc + 1 + 15) / 16) * 512;
        q.off_tv = (uint32_t)o;
        if ((rec_off((uint32_t)nc) >> 4) > 65535) continue;     // 16-bit record field
        o += (size_t)nv * 24;
        o = (o + 15) & ~(size_t)15;
        q.off_red = (uint32_t)o;
        o += 64 + (((size_t)4 * T + 15) & ~(size_t)15) + 4 * FLORW;      // + the frame-error words
                                                                       // (16 B aligned), the OR words
        if (es) {                  // + the T syndrome words of the early-stop builds, rounded alike
            q.es = true;
            q.off_u = (uint32_t)o;
            o += ((size_t)4 * T + 15) & ~(size_t)15;
        }
        q.off_alut = (uint32_t)o;
        o += (size_t)2 * q.arows * LUT_W * 4;
        q.off_blut = (uint32_t)o;
        o += (size_t)2 * q.bcols * BLUT_W * 4;
        q.lds = (o + 15) & ~(size_t)15;
        if (q.lds > BS_LDS_MAX) continue;
        // (early stop: the instance the full-T decode would take, or none -- a forced instance
        // without the build is not replaced by another)
        if (es && (!bsc_es_inst(i) || q.bcols != 1)) return p;
        q.ok = true;
        return q;
    }
    return p;
}

static int bsc_tables(const DevGraph& g, const BscPlan& p, FusedWorkspace& ws, hipStream_t s) {
    if (ws.bs_graph && ws.bs_graph_inst == BSC_TAG + p.inst) return LDPC_OK;
    if (ws.bs_graph) {
        (void)hipFree(ws.bs_graph);
        ws.bs_graph = nullptr;
    }
    const host::GraphTables& h = *g.host;
    const BscInst& k = kBscInst[p.inst];
    const int nv = g.n_vars, nc = g.n_checks, z = h.z, LPC = k.LPC;
    const int VNW = k.DVH + 1, EPL = (k.D + LPC - 1) / LPC, CVW = (EPL + 1) / 2;
    const int NWp = p.nw, nl = 64 * NWp;
    auto slot_of = [&](int i, int kk, int hc) {
        const int L = p.rl[(size_t)i];
        return (uint32_t)((size_t)p.lay[2 * i] + (size_t)(kk % L) * p.lay[2 * i + 1] + (size_t)(kk / L) * z + hc);
    };
    // Tv slots: variable (column j, index hh) keeps its Tv at j z + (hh + toff_j) mod z.  The
    // check phase reads the Tv of each lane's edge m (ds_read_b64, bank = dword mod 64, 6 dwords
    // per variable: 32 lanes are conflict-free when their Tv indices differ mod 32); a half-wave
    // holds 8 consecutive checks of 4 edges, i.e. 4 runs of 8 consecutive indices from 4
    // columns, which overlap mod 32 for most column offsets.  A hill climb over the per-column
    // rotations toff_j spreads them (BG1: 695 -> ~514 LDS cycles per Tv read round of a
    // check pass in tools/bank_model's terms); the variable phase writes the same slot.
    const char* etv = getenv("LDPC_BSC_TVPERM");
    const std::vector<int> toff = (etv && atoi(etv) == 0) ? std::vector<int>(h.N, 0)
                                                           : column_rotation_lanes(h, EPL, p.lanes);
    auto tv_index = [&](int v) -> uint32_t {
        const int j = v / z, hh = v - j * z;
        return (uint32_t)(j * z + (hh + toff[j]) % z);
    };
    const uint32_t pad_word = (uint32_t)p.nslot | ((rec_off((uint32_t)nc) >> 4) << 16);    // zero slot, zero record
    std::vector<uint32_t> vn((size_t)k.VPL * nl * VNW, 0u);
    std::vector<int32_t> wdeg((size_t)2 * k.VPL * NWp, 0);
    for (int u = 0; u < k.VPL; ++u)
        for (int l = 0; l < nl; ++l) {
            uint32_t* q = &vn[((size_t)u * nl + l) * VNW];
            for (int f = 0; f < k.DVH; ++f) q[f] = pad_word;
            q[k.DVH] = 0xFFFFFFFFu;
        }
    for (int w = 0; w < NWp; ++w)
        for (int u = 0; u < k.VPL; ++u) {
            const int ch = p.vslot[(size_t)w * k.VPL + u];
            int dmax = ch < 0 ? -1 : 0, dmin = ch < 0 ? 0 : 1 << 30;     // -1: no chunk (skipped)
            for (int l = 0; ch >= 0 && l < 64; ++l) {
                const int o = 64 * ch + l;
                if (o >= nv) { dmin = 0; continue; }
                uint32_t* q = &vn[((size_t)u * nl + 64 * w + l) * VNW];
                const int v = p.vorder[o], j = v / z, hh = v - j * z;
                const int c0 = h.col_ptr[j], dv = h.col_ptr[j + 1] - c0;
                for (int f = 0; f < dv; ++f) {
                    const int pe = h.col_pe[c0 + f], i = h.pe_row[pe];
                    int hc = hh - h.pe_shift[pe];
                    hc = hc < 0 ? hc + z : hc;
                    q[f] = slot_of(i, pe - h.row_ptr[i], hc) | ((rec_off((uint32_t)(i * z + hc)) >> 4) << 16);
                }
                q[k.DVH] = (uint32_t)v | (tv_index(v) << 16);
                dmax = std::max(dmax, dv);
                dmin = std::min(dmin, dv);
            }
            wdeg[2 * ((size_t)u * NWp + w)] = dmax;
            wdeg[2 * ((size_t)u * NWp + w) + 1] = dmin;
        }
    const int cch = p.cn_lanes / 64;
    std::vector<int32_t> cchunk((size_t)NWp * k.CPL, -1);
    if (k.CPL == 1 && k.VPL == 1) {
        for (int w = 0; w < NWp; ++w) cchunk[w] = w < cch ? w : -1;
    } else {
        const std::vector<int> cs = deal_chunks(check_chunk_cost_lanes(h, p.lanes), NWp, k.CPL);
        for (size_t x = 0; x < cs.size(); ++x) cchunk[x] = cs[x];
    }
    std::vector<uint32_t> cvar((size_t)p.cn_lanes * CVW, 0u);
    for (int ql = 0; ql < p.cn_lanes; ++ql) {
        const int32_t dl = p.lanes[(size_t)ql];
        if (dl < 0) continue;
        const int cc = dl & 0xFFFF, cj = (dl >> 16) & 15, L = (dl >> 20) & 15;
        const int i = cc / z, hc = cc - i * z;
        for (int m = 0; m < EPL; ++m) {
            const int kk = L * m + cj;
            if (kk >= h.row_ptr[i + 1] - h.row_ptr[i]) continue;
            const int pe = h.row_ptr[i] + kk;
            const uint32_t v = tv_index(h.pe_col[pe] * z + (hc + h.pe_shift[pe]) % z);
            cvar[(size_t)ql * CVW + (m >> 1)] |= v << (16 * (m & 1));
        }
    }
    const size_t nwords = vn.size() + wdeg.size() + p.lay.size() + cchunk.size() + cvar.size() + p.lanes.size();
    void* d = nullptr;
    if (hipMalloc(&d, nwords * 4) != hipSuccess) { (void)hipGetLastError(); return LDPC_ERR_OOM; }
    uint32_t* dp = reinterpret_cast<uint32_t*>(d);
    size_t at = 0;
    bool ok = true;
    auto up = [&](const void* src, size_t n) {
        if (n) ok = ok && hipMemcpyAsync(dp + at, src, n * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        at += n;
    };
    up(vn.data(), vn.size());
    up(wdeg.data(), wdeg.size());
    up(p.lay.data(), p.lay.size());
    up(cchunk.data(), cchunk.size());
    up(cvar.data(), cvar.size());
    up(p.lanes.data(), p.lanes.size());
    if (!ok || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipFree(d);
        return LDPC_ERR_HIP;
    }
    ws.bs_graph = d;
    ws.bs_graph_inst = BSC_TAG + p.inst;
    return LDPC_OK;
}

// What bsc_run fills for one launch: the arguments of every build of an instance (as bsl's
// BsLaunch); bs_launch_kernel hands each kernel the struct it takes.
struct BscLaunch : BscArgsEw {
    int word;                    // BscArgsXp::word
};

template <int I, bool XP, bool B1, bool Q8, bool ES = false, bool EW = false, bool L8 = false>
static int bsc_launch1(const BscLaunch& a, int nblocks, int nw, size_t lds, hipStream_t s) {
    constexpr BscInst k = kBscInst[I];
    return bs_launch_kernel<&k_bsc<k.D, k.DVH, k.DVL, k.LPC, k.VPL, k.CPL, k.WPE, XP, 64 * k.NW, k.MIX, B1, Q8, ES, EW, L8>>(
        a, nblocks, nw, lds, s);
}
// instance I's launch: the build this decode takes
template <int I>
static int bsc_launch(const BscLaunch& a, int nblocks, int nw, size_t lds, hipStream_t s, int src, bool es) {
    const bool b1 = bsc_b1_on() && a.beta_id && a.bcols == 1;
    const bool q8 = src == BS_SRC_GEN;
    if (src == BS_SRC_L8) {
        // int8 LLRs, early stop: the int8 builds of the early-stop kernels below (ES, and EW with a
        // plane buffer for the stop-iteration words), on the same terms
        if (es) {
            if constexpr (bsc_es_inst(I)) {
                if (a.hdx || !a.beta_id || a.bcols != 1) return LDPC_ERR_UNSUPPORTED;
                return a.hdw ? bsc_launch1<I, false, true, false, true, true, true>(a, nblocks, nw, lds, s)
                             : bsc_launch1<I, false, true, false, true, false, true>(a, nblocks, nw, lds, s);
            }
            return LDPC_ERR_UNSUPPORTED;
        }
        // int8 LLRs: the decode and the word build (hdx with word) of the instances a plan takes
        if constexpr (bsc_l8_inst(I)) {
            if (a.hdw || (a.hdx && !a.word)) return LDPC_ERR_UNSUPPORTED;
            if (a.hdx) return b1 ? bsc_launch1<I, true, true, false, false, false, true>(a, nblocks, nw, lds, s)
                                 : bsc_launch1<I, true, false, false, false, false, true>(a, nblocks, nw, lds, s);
            return b1 ? bsc_launch1<I, false, true, false, false, false, true>(a, nblocks, nw, lds, s)
                      : bsc_launch1<I, false, false, false, false, false, true>(a, nblocks, nw, lds, s);
        }
        return LDPC_ERR_UNSUPPORTED;
    }
    if (es) {
        // the early-stop builds (float LLRs, or the in-prologue channel): on the B1 build of the
        // instances that have them, one workgroup per pack, no export build; with a plane buffer
        // for the stop-iteration words, the EW build
        if constexpr (bsc_es_inst(I)) {
            static_assert(kBscInst[I].MIX, "an early-stop instance");
            if (a.hdx || !a.beta_id || a.bcols != 1) return LDPC_ERR_UNSUPPORTED;
            if (a.hdw)
                return q8 ? bsc_launch1<I, false, true, true, true, true>(a, nblocks, nw, lds, s)
                          : bsc_launch1<I, false, true, false, true, true>(a, nblocks, nw, lds, s);
            return q8 ? bsc_launch1<I, false, true, true, true>(a, nblocks, nw, lds, s)
                      : bsc_launch1<I, false, true, false, true>(a, nblocks, nw, lds, s);
        }
        return LDPC_ERR_UNSUPPORTED;
    }
    if (a.hdx) {
        // (the generated channel comes from ldpc_decode_awgn, which exports no hard bits)
        if (q8) return LDPC_ERR_UNSUPPORTED;
        return b1 ? bsc_launch1<I, true, true, false>(a, nblocks, nw, lds, s)
                  : bsc_launch1<I, true, false, false>(a, nblocks, nw, lds, s);
    }
    if (q8) return b1 ? bsc_launch1<I, false, true, true>(a, nblocks, nw, lds, s)
                      : bsc_launch1<I, false, false, true>(a, nblocks, nw, lds, s);
    return b1 ? bsc_launch1<I, false, true, false>(a, nblocks, nw, lds, s)
              : bsc_launch1<I, false, false, false>(a, nblocks, nw, lds, s);
}
typedef int (*BscLaunchFn)(const BscLaunch&, int, int, size_t, hipStream_t, int, bool);
template <int... I>
constexpr std::array<BscLaunchFn, sizeof...(I)> bsc_launch_table(std::integer_sequence<int, I...>) {
    return {&bsc_launch<I>...};
}

}  // namespace bs

using namespace bs;

// Host-side bounds check of the bsc plan for this graph (test infrastructure, through
// ldpc_debug_bs_bounds): wherever bsc_q8_ok's test lets the Q8 build run, the in-prologue
// channel's tables lie inside the SGN region they borrow and clear of every region after it
// (LDPC_BOUNDS_BIG_TABLES: taken 4 bytes longer than that region, so a test can see the check
// fail), and every check chunk's count of real edge positions -- the kernel's
// wave_or / popc over its lanes, restated -- is in 1 .. EPL, the range the min2 switch covers
// (its other cases are marked unreachable).  Returns 1 if a plan was checked, 0 if
// none serves the graph; violations / first as BoundsReport.
// es: the early-stop plan of the graph instead (LDPC_BOUNDS_ES_BSC): the same checks, and its T
// syndrome words lie inside the RED region, after the FLORW words and before ALUT, with the
// dynamic LDS size inside BS_LDS_MAX.
int bsc_debug_bounds(const DevGraph& g, int mode, float clip, int T, int flags, int& violations,
                     std::string& first, bool es) {
    const BscPlan p = bsc_plan(g, mode, false, false, clip, T, es);
    if (!p.ok) return 0;
    auto fail = [&](const char* what, long long idx, long long lo, long long hi) {
        if (violations++ == 0) {
            char buf[160];
            snprintf(buf, sizeof(buf), "%s: %lld outside [%lld, %lld)", what, idx, lo, hi);
            first = buf;
        }
    };
    const host::GraphTables& h = *g.host;
    const BscInst& k = kBscInst[p.inst];
    const int LPC = k.LPC, EPL = (k.D + LPC - 1) / LPC, z = h.z, nc = g.n_checks;
    if (es) {
        // RED: 16 words, the frame-error words (T rounded to 4), the FLORW words, then U[0 .. T)
        const long long u0 = p.off_u, un = 4LL * T;
        const long long red_used = (long long)p.off_red + 4LL * (16 + ((T + 3) & ~3) + FLORW);
        if (!p.es || u0 < red_used || u0 + un > (long long)p.off_alut)
            fail("syndrome words", u0 + un, red_used, p.off_alut);
        if (u0 & 15) fail("syndrome words' alignment", u0 & 15, 0, 1);
        if (p.lds > BS_LDS_MAX) fail("LDS size", (long long)p.lds, 0, (long long)BS_LDS_MAX + 1);
    }
    if (q8_tab_fits(p)) {
        const long long tb = q8_tab_lds(p);
        const long long tn = (flags & LDPC_BOUNDS_BIG_TABLES) ? (long long)p.off_a + 4 : 4LL * AWGN_TAB_W;
        if (tb < 0 || tb + tn > (long long)p.off_a) fail("channel tables", tb + tn, 0, p.off_a);
        // (ARG, REC, TV, RED, ALUT and BLUT, in this order, up to the dynamic LDS size)
        const long long reg[] = {p.off_a, p.off_rec, p.off_tv, p.off_red, p.off_alut, p.off_blut, (long long)p.lds};
        static const char* const name[] = {"channel tables / ARG", "channel tables / REC", "channel tables / TV",
                                           "channel tables / RED", "channel tables / ALUT", "channel tables / BLUT"};
        for (int i = 0; i < 6; ++i)
            if (tb < reg[i + 1] && reg[i] < tb + tn) fail(name[i], tb + tn, reg[i], reg[i + 1]);
    }
    for (int ch = 0; ch < p.cn_lanes / 64; ++ch) {
        const int32_t d0 = p.lanes[(size_t)ch * 64];
        const int Lc = (!k.MIX || d0 < 0 || ((d0 >> 20) & 15) == LPC) ? LPC : LPC / 2;
        uint32_t any = 0u;
        for (int l = 0; l < 64; ++l) {
            const int32_t d = p.lanes[(size_t)ch * 64 + l];
            const int cc = d < 0 ? nc : (d & 0xFFFF);
            const int ci = std::min(cc / z, nc / z - 1);
            const int gdeg = cc < nc ? h.row_ptr[ci + 1] - h.row_ptr[ci] : 0;
            const int npos = (gdeg + Lc - 1) / Lc;
            if (npos > 31) { fail("real positions of a lane", npos, 0, 32); continue; }
            any |= (1u << npos) - 1u;
        }
        const int gm = __builtin_popcount(any);
        if (gm < 1 || gm > EPL) fail("real positions of a chunk (the min2 switch)", gm, 1, EPL + 1);
    }
    return 1;
}

// ---- requests (ldpc_fused.h); early stop: DESIGN 3.7 -------------------------------------------
static BscPlan bsc_plan(const DevGraph& g, const BsReq& r) {
    return bsc_plan(g, r.mode, r.ucn, r.per_edge_w, r.clip, r.T, r.es);
}

bool bsc_supported(const DevGraph& g, const BsReq& r) { return bsc_plan(g, r).ok; }

bool bsc_q8_ok(const DevGraph& g, const BsReq& r, bool has_short) {
    const BscPlan p = bsc_plan(g, r);
    // (the in-prologue channel's tables borrow the SGN region at LDS byte 0)
    return p.ok && (!has_short || p.cu > 0.f) && q8_tab_fits(p);
}

bool bsc_l8_ok(const DevGraph& g, const BsReq& r, bool has_short) {
    const BscPlan p = bsc_plan(g, r);
    // (an early-stop plan is on an instance with early-stop builds, each with its int8 build)
    return p.ok && (r.es ? bsc_es_inst(p.inst) : bsc_l8_inst(p.inst)) && (!has_short || p.cu > 0.f);
}

const char* bsc_kernel_name(const DevGraph& g, const BsReq& r) {
    static thread_local char buf[64];
    const BscPlan p = bsc_plan(g, r);
    if (!p.ok) return "";
    const BscInst& k = kBscInst[p.inst];
    snprintf(buf, sizeof(buf), "bsc[p32,w%d,d%d,v%d/%d,l%d%s,x%d/%d%s]", p.nw, k.D, k.DVH, k.DVL, k.LPC,
             k.MIX ? "/2" : "", k.VPL, k.CPL, r.es ? ",es" : "");
    return buf;
}

// one launch of plan p (an early-stop plan for an early-stop request)
static int bsc_run(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const BscPlan& p, const float* llr,
                   const BsReq& r, const BsOut& o, hipStream_t s) {
    // (the graph tables do not depend on the mode: both kinds of decode share them)
    int st = bsc_tables(g, p, ws, s);
    if (st != LDPC_OK) return st;
    const BscInst& k = kBscInst[p.inst];
    const float step = bs_step(r.mode);
    uint32_t *alut = nullptr, *blut = nullptr;
    st = bs_make_tables(b, g, p.arows, p.arows, p.bcols, step, bs_qmax(r.mode), p.cu, false, ws, &alut, &blut, s);
    if (st != LDPC_OK) return st;
    const uint32_t* gt = reinterpret_cast<const uint32_t*>(ws.bs_graph);
    const int VNW = k.DVH + 1;
    BscLaunch a{};
    a.n_iter = o.n_iter;
    a.iter_hist = o.iter_hist;
    a.off_u = p.off_u;
    a.hdw = o.hdw;
    a.word = o.word ? 1 : 0;
    // (int8 LLRs: the L8 builds read the bytes behind the same argument)
    a.llr = r.l8 ? reinterpret_cast<const float*>(r.l8) : llr;
    a.gen = bs_gen(b, q8_tab_lds(p));    // the in-prologue channel (ldpc_decode_awgn)
    a.B = b.B;
    a.n_vars = g.n_vars;
    a.n_checks = g.n_checks;
    a.T = b.T;
    a.target_bits = b.target_bits;
    a.cn_dmin = p.cn_dmin;
    a.z = g.z;
    a.inv = 1.0f / step;
    a.cu = p.cu;
    a.qmax = bs_qmax(r.mode);
    a.beta_id = g.w_beta_one ? 1 : 0;
    a.row_ptr = g.row_ptr;
    a.vn_tab = gt;
    const size_t nvt = (size_t)k.VPL * 64 * p.nw * VNW;
    a.vn_wdeg = reinterpret_cast<const int32_t*>(gt + nvt);
    a.row_lay = a.vn_wdeg + 2 * (size_t)k.VPL * p.nw;
    a.cn_chunk = a.row_lay + 2 * (size_t)g.M;
    a.cn_var = reinterpret_cast<const uint32_t*>(a.cn_chunk + (size_t)p.nw * k.CPL);
    a.cn_lane = reinterpret_cast<const int32_t*>(a.cn_var + (size_t)p.cn_lanes * ((((k.D + k.LPC - 1) / k.LPC) + 1) / 2));
    // (LDPC_BS_STAGGER still applies; C5: no gain.  Early stop: none, the packs end at different times)
    if (!r.es) bs_stagger(false, &a.stagger, &a.stagger_n);
    a.alut = alut;
    a.blut = blut;
    a.arows = p.arows;
    a.bcols = p.bcols;
    a.counters = o.counters;
    a.flags = o.flags;
    a.bad = o.bad;
    a.iter_wrong = r.es ? nullptr : b.iter_wrong;
    a.hdx = o.hdx;
    a.off_a = p.off_a;
    a.off_rec = p.off_rec;
    a.off_tv = p.off_tv;
    a.off_red = p.off_red;
    a.off_alut = p.off_alut;
    a.off_blut = p.off_blut;
    const int nblocks = (int)((b.B + PACK - 1) / PACK);
    static constexpr auto kLaunch = bsc_launch_table(std::make_integer_sequence<int, kBscNInst>{});
    return kLaunch[p.inst](a, nblocks, p.nw, p.lds, s, r.l8 ? BS_SRC_L8 : b.q8 ? BS_SRC_GEN : BS_SRC_LLR, r.es);
}

// (bs_decode falls through to it; LDPC_ERR_UNSUPPORTED with nothing launched when no build serves
// the request)
int bsc_decode(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, const BsReq& r,
               const BsOut& o, hipStream_t s) {
    const BscPlan p = bsc_plan(g, r);
    if (!p.ok) return LDPC_ERR_UNSUPPORTED;
    return bsc_run(g, b, ws, p, llr, r, o, s);
}

}  // namespace ldpc
