// ldpc_fused.h — fused (all iterations in one launch, LDS/register-resident) decoder.
#pragma once
#include <string>

#include "ldpc_internal.h"

namespace ldpc {

struct FusedWorkspace {
    uint64_t* hd = nullptr;        // [T][tiles][n_vars][4] hard decisions (only for bit export)
    int64_t hd_elems = 0;
    void* tables = nullptr;        // per-decode tables shared by all workgroups (v5)
    size_t tables_bytes = 0;
    void* bs_graph = nullptr;      // bit-sliced kernel: graph tables (built once per context)
    int bs_graph_inst = -1;        // the kernel instance they were built for
    void* bs_es_graph = nullptr;   // the same for the early-stop instances (a pair of their own:
    int bs_es_graph_inst = -1;     // alternating decodes of both kinds rebuild neither)
    void* bs_lut = nullptr;        // bit-sliced kernel: per-decode weight tables
    size_t bs_lut_bytes = 0;
    uint32_t* bs_bad = nullptr;    // [packs] 1: pack decoded by the v5 fixup
    int64_t bs_bad_n = 0;
    int bs_resident[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // bit-sliced kernel with the pack loop: the workgroups resident
    uint64_t bs_resident_key = ~0ull; // at once (decode / export / channel build, the frozen decode /
                                      // channel build, the int8 decode / word build, the frozen
                                      // decode / channel build with the weights frozen in kind), and
                                      // what for
    uint32_t* bs_ticket = nullptr; // the pack loop's ticket word (ldpc_bs_kernel.h, BS_RED_NEXT): allocated
                                   // at the first launch that wants it, zeroed before each one
    bool bs_frozen = false;        // the last bit-sliced decode ran a geometry-frozen build
    bool bs_afix = false;          // the last bit-sliced decode weighed its check minima through the
                                   // fixed-set tables (BsLaunch::atid set)
    bool bs_wf = false;            // the last bit-sliced decode ran a build with the weights frozen in
                                   // kind (BsLaunch::wf)
    uint32_t* hdx = nullptr;       // [T][packs][n_vars] bit-sliced hard decisions (bit export of
    int64_t hdx_elems = 0;         // the bit-sliced kernels; fixup packs are in `hd` instead)
    bool bits_packed = false;      // the last bit-exporting decode wrote hdx (+ hd for bad packs)
    uint32_t* hdw = nullptr;       // [ceil(B_max / 32)][n_vars] the word modes' hard decisions (last
    int64_t hdw_elems = 0;         // iteration's; stop iteration's, 3.9), bit-sliced;
                                   // allocated on first use
    uint8_t* ev_niter = nullptr;   // [B_max] the events mode's n_iter when the caller asks for none
    int64_t ev_niter_n = 0;        // (early stop)
    const char* last_kernel = "";  // the kernel that served the last decode (ldpc_ctx_last_kernel)
    // what the per-decode table kernels last wrote (they depend only on the graph, the weights
    // and T): a decode with the same key skips them
    uint64_t key_gad[4] = {~0ull, 0, 0, 0}, key_qtab[4] = {~0ull, 0, 0, 0}, key_bslut[4] = {~0ull, 0, 0, 0};
};

// a grow-on-demand device buffer: at least n elements behind p afterwards (have: its size in
// elements, of elem bytes each; the contents are not kept)
template <class T, class N>
int dev_grow(T*& p, N& have, size_t n, size_t elem) {
    if ((size_t)have >= n) return LDPC_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    have = 0;
    if (hipMalloc(reinterpret_cast<void**>(&p), n * elem) != hipSuccess) {
        (void)hipGetLastError();
        return LDPC_ERR_OOM;
    }
    have = (N)n;
    return LDPC_OK;
}
template <class T, class N>
int dev_grow(T*& p, N& have, size_t n) { return dev_grow(p, have, n, sizeof(T)); }

// fused v5 serves this request (QMS q in {5,-5,4,3}, clip_llr on the grid, a shape fits)
bool fused_supported(const DevGraph& g, int mode, int T, float clip_llr);
int64_t fused_bytes_per_cw(const DevGraph& g, int T);
int fused_decode(const DevGraph& g, Bufs& b, FusedWorkspace& ws, const float* llr, int mode,
                 bool ucn, bool want_bits, int ntiles_max, int T_max, int per_edge_w,
                 int64_t* counters, uint8_t* flags, hipStream_t s);
// where the last bit-exporting fused decode left its hard decisions (ldpc_capi.hip's HdSrc)
struct HdView {
    const uint64_t* tile;      // [T+1][tiles][n_vars][4] (Bufs::hd layout, slot t + 1), or null
    const uint32_t* pack;      // [T][packs][n_vars] bit-sliced, or null
    const uint32_t* bad;       // [packs] 1: this pack's bits are in `tile` (v5 fixup)
};
HdView fused_bits_view(const FusedWorkspace& ws);
const char* fused_kernel_name(const DevGraph& g, int mode, int T, float clip_llr, bool ucn,
                              bool per_edge_w);

// v5 (ldpc_fused5.hip): byte-packed check state, default when a shape fits
bool fused5_supported(const DevGraph& g, int T);
const char* fused5_shape_name(const DevGraph& g, int T);
// only: null, or per-32-codeword pack flags: decode just the blocks of flagged packs (the
// bit-sliced kernel's fixup; needs a shape with CW <= 32, fused5_cw)
int fused5_decode(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr,
                  int qmax, float step, int clip_u, bool per_edge_w, uint64_t* hd_out,
                  int64_t* counters, uint8_t* flags, hipStream_t s, const uint32_t* only = nullptr);
int fused5_cw(const DevGraph& g, int T);

// ---- the bit-sliced kernels: bsl (ldpc_bs.hip, 32 codewords per word, QMS q = 5 / -5 / 4 / 3)
// and bsc (ldpc_bsc.hip, compressed check messages: the graphs whose per-edge slots exceed the LDS)
// One request: the QMS grid, UCN weights set, per-edge CN weights (never served), clip_LLR (the
// LLR of shortened bits), the iteration count (whose per-iteration frame words take 4 T bytes of
// LDS), and es: syndrome-based early stop, which has kernel builds of its own.
struct BsReq {
    int mode;
    bool ucn, per_edge_w;
    float clip;
    int T;
    bool es;
    const int8_t* l8 = nullptr;    // the LLRs as int8 grid values [B][n_vars] (device; ldpc_decode_q8,
                                   // DESIGN 3.11) instead of the float LLRs, or null; no part of the plan
};
// What one decode writes; null: off.
struct BsOut {
    int64_t* counters;         // [0..2]
    uint8_t* flags;            // [B] frame flags
    uint32_t* bad;             // [packs] 1: an LLR of the pack is off the quantizer grid (not decoded)
    uint32_t* hdx;             // the export build: [T][packs][n_vars] every iteration's hard decisions
                               // (bit r of word (t, pack, v) = codeword 32 pack + r)
    bool word;                 // hdx is [packs][n_vars] and takes the last iteration's alone
    uint8_t* n_iter;           // early stop: [B] iterations run (0: pack off the grid)
    int64_t* iter_hist;        // early stop: [T] += codewords that ran t + 1 iterations
    uint32_t* hdw;             // early stop: [packs][n_vars] each codeword's hard decisions at its
                               // stop iteration (the EW builds)
};
// bs_*: bsl, or where no bsl plan serves the request, bsc (the fall-through).  An early-stop
// request falls through only for a graph that no bsl plan at all serves (ldpc_bs.hip, bs_route).
// q8_ok: the in-prologue channel (Bufs::q8 / gen8) serves the request's counters-only decode: the
// kernel has room for the sampler's tables and, with shortened bits in the channel, the
// shortened-bit marker; a caller checks it before it hands a decode b.q8.
// kernel_name: "bsl[...]" / "bsc[...]", with ",es" inside the brackets for early stop; "" if unserved.
bool bs_supported(const DevGraph& g, const BsReq& r);
bool bs_q8_ok(const DevGraph& g, const BsReq& r, bool has_short);
// l8_ok: the int8-LLR builds (BsReq::l8) serve the request: its plan's instance has
// them and, with has_short (the +-clip markers in the input), decodes shortened bits; for an
// early-stop request, its early-stop plan's instance
bool bs_l8_ok(const DevGraph& g, const BsReq& r, bool has_short);
bool bsc_l8_ok(const DevGraph& g, const BsReq& r, bool has_short);
const char* bs_kernel_name(const DevGraph& g, const BsReq& r);
bool bsc_supported(const DevGraph& g, const BsReq& r);
bool bsc_q8_ok(const DevGraph& g, const BsReq& r, bool has_short);
const char* bsc_kernel_name(const DevGraph& g, const BsReq& r);
// the decode of b.B codewords (LLRs at llr, the in-prologue channel b.q8 / b.gen8, or int8 LLRs at
// r.l8).  Packs with an LLR off the grid are marked in o.bad (early stop and int8 LLRs: also flags
// 0x80; early stop: n_iter 0), not decoded.
// LDPC_ERR_UNSUPPORTED: no build serves the request; nothing was launched.
int bs_decode(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, const BsReq& r,
              const BsOut& o, hipStream_t s);
int bsc_decode(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, const BsReq& r,
               const BsOut& o, hipStream_t s);
// host-side bounds check of the bsc plan (test infrastructure, ldpc_debug_bs_bounds), and the
// flags of that check (include/ldpc_nms_debug.h): no kernel or launch path reads them
enum { LDPC_BOUNDS_PRE_GUARD = 1, LDPC_BOUNDS_BIG_TABLES = 2, LDPC_BOUNDS_ES = 4, LDPC_BOUNDS_ES_BSC = 8,
       LDPC_BOUNDS_UCN1 = 16 };
// (es: the graph's early-stop plan instead, LDPC_BOUNDS_ES_BSC)
int bsc_debug_bounds(const DevGraph& g, int mode, float clip, int T, int flags, int& violations,
                     std::string& first, bool es = false);
// (fused_decode with it: the bit-sliced kernel or LDPC_ERR_UNSUPPORTED)
bool fused_q8_ok(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w, bool has_short);
// a decode with an in-kernel generator (Bufs::awgn) runs the v5 kernel's prologue channel
bool fused_awgn_v5(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w, bool app);
// The bit-sliced decodes without the v5 fixup: the word mode (ldpc_decode_word), early
// stop (ldpc_decode_es; 3.7) and early stop with the word (ldpc_decode_es_word; 3.9).
// fused_bs_supported: the request is one they decode: an early-stop request that bs_decode serves;
// without early stop (the word mode), one fused_decode would take bs_decode for, of a graph with
// at most WORD_MAX_VARS variables (word_out's bound).
// fused_decode_bs: o takes counters, flags, n_iter and iter_hist; ws.bs_bad and, with rows, ws.hdw
// are sized here.  rows: null, or [B][ceil(n_vars / 32)]: the export build (early stop: the EW
// build) stores the last (the stop) iteration's hard decisions into ws.hdw, and the output kernel
// word_out (ldpc_word.hip) writes the rows, word_flags [B] or null (bit 0: syndrome nonzero) and,
// for the packs the decode marked off the grid, zero rows and 0x80 in word_flags and o.flags.
// ev: null, or the events mode's sink (ldpc_decode_events), instead of rows: the same
// decode step into ws.hdw, then events_out (ldpc_events.hip) in word_out's place: one record per
// frame whose word is nonzero, appended at *count (accumulated, never zeroed here): slots < cap
// take the frame's index frame_base + b, {n_iter, a, a_target, b} and, with word, its row packed
// as a row of `rows` is; slots >= cap are counted only.  target_bits: a_target's range.
// Nothing is allocated or launched for a request that is not served.
constexpr int WORD_MAX_VARS = 4096;      // (the bit-sliced plans' bound: 4 variables on 1024 lanes)
struct EventSink {
    int64_t frame_base, cap;
    int64_t* count;            // [1]
    int64_t* frame;            // [cap]
    int32_t* info;             // [cap][4]
    uint32_t* word;            // [cap][ceil(n_vars / 32)] or null
    int target_bits;
};
bool fused_bs_supported(const DevGraph& g, const BsReq& r);
int fused_decode_bs(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, const BsReq& r,
                    int64_t B_max, int ntiles_max, BsOut o, uint32_t* rows, uint8_t* word_flags, hipStream_t s,
                    const EventSink* ev = nullptr);
// n_iter: [B] the early-stop decode's, or null: every record takes T
int events_out(const DevGraph& g, const uint32_t* planes, const uint32_t* bad, int64_t B, const uint8_t* n_iter,
               int T, const EventSink& ev, uint8_t* frame_flags, hipStream_t s);
int word_out(const DevGraph& g, const uint32_t* planes, const uint32_t* bad, int64_t B, uint32_t* hard_last,
             uint8_t* word_flags, uint8_t* frame_flags, hipStream_t s);
void fused_free(FusedWorkspace& ws);

// float-mode fused decoder (ldpc_ffl.hip): MS, MS without nudge, QMS q = 6, sum-product; counters / flags
// only, row-uniform CN weights
bool ffl_mode(int mode);
bool ffl_supported(const DevGraph& g, int mode, bool ucn, bool per_edge_w);
const char* ffl_kernel_name(const DevGraph& g, int mode, bool ucn, bool per_edge_w);
int ffl_decode(const DevGraph& g, const Bufs& b, const float* llr, int mode, bool ucn, bool per_edge_w,
               int64_t* counters, uint8_t* flags, hipStream_t s);

}  // namespace ldpc
