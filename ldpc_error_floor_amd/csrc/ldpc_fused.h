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
    int bs_resident[3] = {0, 0, 0};   // bit-sliced kernel with the pack loop: the workgroups resident
    uint64_t bs_resident_key = ~0ull; // at once (decode / export / channel build), and what for
    uint32_t* hdx = nullptr;       // [T][packs][n_vars] bit-sliced hard decisions (bit export of
    int64_t hdx_elems = 0;         // the bit-sliced kernels; fixup packs are in `hd` instead)
    bool bits_packed = false;      // the last bit-exporting decode wrote hdx (+ hd for bad packs)
    uint32_t* hdw = nullptr;       // [ceil(B_max / 32)][n_vars] the word modes' hard decisions (last
    int64_t hdw_elems = 0;         // iteration's; stop iteration's, 3.9), bit-sliced;
                                   // allocated on first use
    const char* last_kernel = "";  // the kernel that served the last decode (ldpc_ctx_last_kernel)
    // what the per-decode table kernels last wrote (they depend only on the graph, the weights
    // and T): a decode with the same key skips them
    uint64_t key_gad[4] = {~0ull, 0, 0, 0}, key_qtab[4] = {~0ull, 0, 0, 0}, key_bslut[4] = {~0ull, 0, 0, 0};
};

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

// bit-sliced (ldpc_bs.hip): 32 codewords per word, counters / flags only, QMS q = 5 / -5
// (clip: clip_LLR, the LLR of shortened bits)
// (T: the iteration count, whose per-iteration frame words take 4 T bytes of LDS)
bool bs_supported(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
const char* bs_kernel_name(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
// hdx: null, or [T][packs][n_vars] u32: also store every iteration's hard decisions (bit r of
// word (t, pack, v) = codeword 32 pack + r; the export build of the kernel).  word:
// hdx is [packs][n_vars] and takes the last iteration's hard decisions alone
int bs_decode(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, int mode,
              bool ucn, int64_t* counters, uint8_t* flags, uint32_t* bad, uint32_t* hdx, bool word,
              hipStream_t s);
// the in-prologue channel (Bufs::q8 / gen8) serves this counters-only decode: the bit-sliced
// kernel applies, has room for the sampler's tables in its slot region and, with shortened bits
// in the channel, has the shortened-bit marker (a BIG instance)
bool bs_q8_ok(const DevGraph& g, int mode, bool ucn, float clip, int T, bool has_short);
bool bsc_q8_ok(const DevGraph& g, int mode, bool ucn, float clip, int T, bool has_short);
// host-side bounds check of the bsc plan (test infrastructure, ldpc_debug_bs_bounds), and the
// flags of that check (include/ldpc_nms_debug.h): no kernel or launch path reads them
enum { LDPC_BOUNDS_PRE_GUARD = 1, LDPC_BOUNDS_BIG_TABLES = 2, LDPC_BOUNDS_ES = 4, LDPC_BOUNDS_ES_BSC = 8 };
// (es: the graph's early-stop plan instead, LDPC_BOUNDS_ES_BSC)
int bsc_debug_bounds(const DevGraph& g, int mode, float clip, int T, int flags, int& violations,
                     std::string& first, bool es = false);
// early stop (ldpc_decode_es): the bit-sliced kernel's ES instances serve the request,
// or, for a graph that no bsl plan serves, the compressed kernel's early-stop builds (bsc_*_es);
// their decode (counters [0..2], frame flags, n_iter [B], iter_hist [T], each or null; b.q8 / gen8:
// the in-prologue channel, when bs_es_q8_ok) and its kernel name ("bsl[...,es]" / "bsc[...,es]").
// hdw: null, or [packs][n_vars] u32 that takes each codeword's hard decisions at its stop
// iteration (the EW builds)
bool bs_es_supported(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
bool bs_es_q8_ok(const DevGraph& g, int mode, bool ucn, float clip, int T, bool has_short);
const char* bs_es_kernel_name(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
int bs_decode_es(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, int mode, bool ucn,
                 int ntiles_max, int64_t* counters, uint8_t* flags, uint8_t* n_iter, int64_t* iter_hist,
                 uint32_t* hdw, hipStream_t s);
// (fused_decode with it: the bit-sliced kernel or LDPC_ERR_UNSUPPORTED)
bool fused_q8_ok(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w, bool has_short);
// a decode with an in-kernel generator (Bufs::awgn) runs the v5 kernel's prologue channel
bool fused_awgn_v5(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w, bool app);
// compressed bit-sliced kernel (ldpc_bsc.hip): the graphs whose per-edge slots exceed the LDS
bool bsc_supported(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
const char* bsc_kernel_name(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
int bsc_decode(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, int mode,
               bool ucn, int64_t* counters, uint8_t* flags, uint32_t* bad, uint32_t* hdx, bool word,
               hipStream_t s);
// its early-stop builds: the beta = 1 build of the mixed-lane instances (bs_*_es fall through to
// these where bs_decode falls through to bsc_decode); kernel name "bsc[...,es]"
bool bsc_es_supported(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
bool bsc_es_q8_ok(const DevGraph& g, int mode, bool ucn, float clip, int T, bool has_short);
const char* bsc_es_kernel_name(const DevGraph& g, int mode, bool ucn, bool per_edge_w, float clip, int T);
int bsc_decode_es(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, int mode, bool ucn,
                  int64_t* counters, uint8_t* flags, uint32_t* bad, uint8_t* n_iter, int64_t* iter_hist,
                  uint32_t* hdw, hipStream_t s);
// the word mode (ldpc_decode_word): the request is one the bit-sliced kernels decode
// (fused_decode would take bs_decode for its counters); the decode -- the export build storing
// the last iteration's hard decisions alone into ws.hdw, no v5 fixup, then word_out --; and the
// output kernel (ldpc_word.hip): hard_last [B][ceil(n_vars / 32)], word_flags [B] or null (bit 0:
// syndrome nonzero), and, for the packs the decode marked off the grid (bad), zero rows and 0x80
// in word_flags and frame_flags (or null)
constexpr int WORD_MAX_VARS = 4096;      // (the bit-sliced plans' bound: 4 variables on 1024 lanes)
bool fused_word_supported(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w);
int fused_decode_word(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, int mode, bool ucn,
                      int64_t B_max, int64_t* counters, uint8_t* flags, uint32_t* hard_last,
                      uint8_t* word_flags, hipStream_t s);
// the early-stop decode with the decoded word (ldpc_decode_es_word): bs_decode_es with
// ws.hdw (sized as fused_decode_word's) taking each codeword's hard decisions at its stop
// iteration, then word_out: hard_stop [B][ceil(n_vars / 32)], word_flags [B] or null.  Served
// exactly where bs_decode_es is.
int fused_decode_es_word(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, int mode, bool ucn,
                         int64_t B_max, int ntiles_max, int64_t* counters, uint8_t* flags, uint8_t* n_iter,
                         int64_t* iter_hist, uint32_t* hard_stop, uint8_t* word_flags, hipStream_t s);
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
