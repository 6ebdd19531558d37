// ldpc_fused.hip — dispatch of the fused decoder (all T flooding iterations in ONE launch).
//
// Same algorithm as ldpc_flood.hip / oracle/nms_oracle.py (Main_Functions.py:157-385), but a
// workgroup owns CW codewords for the whole decode, so nothing but the input LLRs and the
// final counters touches HBM.  The kernel is v5 (ldpc_fused5_kernel.h, planning and tables in
// ldpc_fused5.hip).  It serves the integer QMS modes (q in {5, -5, 4, 3}) of every graph that
// plan5 can map to a shape; everything else (q = 6, the float modes, graphs no shape fits, a
// clip_LLR off the quantizer grid) is the flood kernel's, which the AUTO selection falls back
// to.  There are no other fused variants: only kernels with parity tests can be selected.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ldpc_fused.h"
#include "ldpc_awgn.h"

namespace ldpc {

namespace {

float mode_step(int mode) {
    switch (mode) {
        case MODE_Q5: return 0.5f;
        case MODE_QM5: case MODE_Q4: return 1.0f;
        case MODE_Q3: return 2.0f;
        default: return 0.f;
    }
}

int mode_qmax(int mode) { return (mode == MODE_Q4) ? 7 : (mode == MODE_Q3) ? 3 : 15; }

// clip_LLR in grid units: the APP clip (Main_Functions.py:322-325) is a clamp in the kernel's
// integer domain only when clip / step is an integer; 0 when it is not representable
int clip_units(int mode, float clip) {
    const float step = mode_step(mode);
    if (!(step > 0.f) || !(clip > 0.f)) return 0;
    const float cu = clip / step;
    if (cu != rintf(cu) || cu > 32000.f) return 0;
    return (int)cu;
}

// ws.bs_bad: one word per pack of this call, and of the context's largest batch (8 packs per
// 256-codeword tile) whatever this call's is.  Both bit-sliced kernels write a pack's off-grid
// mark into it, the v5 fixup reads it as its `only` flags and word_out as the packs to blank, all
// indexed by pack.
int ensure_bs_bad(FusedWorkspace& ws, int64_t npk, int ntiles_max) {
    return dev_grow(ws.bs_bad, ws.bs_bad_n, (size_t)std::max<int64_t>(npk, 8 * (int64_t)ntiles_max));
}

}  // namespace

bool fused_supported(const DevGraph& g, int mode, int T, float clip_llr) {
    if (mode != MODE_Q5 && mode != MODE_QM5 && mode != MODE_Q4 && mode != MODE_Q3) return false;
    if (g.n_vars >= 32768) return false;
    if (clip_units(mode, clip_llr) == 0) return false;
    return fused5_supported(g, T);
}

// counters-only decodes (throughput mode) run the bit-sliced kernel when it applies
static bool use_bs(const DevGraph& g, const BsReq& r) {
    const int cw = fused5_cw(g, r.T);
    return cw > 0 && cw <= 32 && bs_supported(g, r);
}

// the kernel a counters-only decode runs (the throughput / roofline report)
const char* fused_kernel_name(const DevGraph& g, int mode, int T, float clip_llr, bool ucn,
                              bool per_edge_w) {
    const BsReq r{mode, ucn, per_edge_w, clip_llr, T, false};
    if (!fused_supported(g, mode, T, clip_llr)) return "";
    if (use_bs(g, r)) return bs_kernel_name(g, r);
    return fused5_shape_name(g, T);
}

bool fused_q8_ok(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w, bool has_short) {
    const BsReq r{mode, ucn, per_edge_w, clip, T, false};
    return fused_supported(g, mode, T, clip) && use_bs(g, r) && bs_q8_ok(g, r, has_short);
}

bool fused_awgn_v5(const DevGraph& g, int mode, int T, float clip, bool ucn, bool per_edge_w, bool app) {
    // fused_decode with a generator: the v5 prologue, except counters-only decodes the
    // bit-sliced kernels serve (UNSUPPORTED there: ldpc_decode_awgn then generates into HBM)
    return fused_supported(g, mode, T, clip) && (app || !use_bs(g, BsReq{mode, ucn, per_edge_w, clip, T, false}));
}

int64_t fused_bytes_per_cw(const DevGraph& g, int T) {
    (void)T;
    // compulsory: the channel LLRs are read once; outputs are counters only
    return (int64_t)g.n_vars * 4;
}

int fused_decode(const DevGraph& g, Bufs& b, FusedWorkspace& ws, const float* llr, int mode,
                 bool ucn, bool want_bits, int ntiles_max, int T_max, int per_edge_w,
                 int64_t* counters, uint8_t* flags, hipStream_t s) {
    if (!fused_supported(g, mode, b.T, b.clip)) return LDPC_ERR_UNSUPPORTED;
    const BsReq r{mode, ucn, per_edge_w != 0, b.clip, b.T, false};
    // counters-only decodes the bit-sliced kernel serves read their LLRs: with an in-kernel
    // channel requested, the caller (ldpc_decode_awgn) generates them into HBM first — the
    // channel kernel plus the bit-sliced decode beat the v5 kernel's in-prologue channel
    if (b.awgn && !b.app_out && use_bs(g, r)) return LDPC_ERR_UNSUPPORTED;
    const float step = mode_step(mode);
    const int cu = clip_units(mode, b.clip);
    uint64_t* hd_out = nullptr;
    // counters / frame flags / bit exports without APP: the bit-sliced kernel when it applies
    // (its export build stores every iteration's hard decisions, bit-sliced, in ws.hdx)
    const bool bs = !b.app_out && !b.awgn && use_bs(g, r);
    if (b.q8 && !bs) return LDPC_ERR_UNSUPPORTED;          // the in-prologue channel is the bit-sliced kernels'

    ws.bits_packed = false;
    if (want_bits) {
        const int sh = dev_grow(ws.hd, ws.hd_elems, (size_t)(T_max + 1) * ntiles_max * g.n_vars * 4);
        if (sh != LDPC_OK) return sh;
        // the v5 export ORs its bits into a zeroed buffer; a bit-sliced decode reads the tile
        // buffer only for the packs its v5 fixup decodes, and the fixup clears those blocks'
        // bits itself (f5_block), so the (T + 1) x tiles x n_vars x 32 B memset is skipped
        if (!bs &&
            hipMemsetAsync(ws.hd, 0, (size_t)(b.T + 1) * b.ntiles * g.n_vars * 4 * sizeof(uint64_t), s) != hipSuccess)
            return LDPC_ERR_HIP;
        hd_out = ws.hd;
    }
    if (bs) {
        // bit-sliced kernel; packs whose LLRs are off the quantizer grid go to the v5 kernel
        const int64_t npk = (b.B + 31) / 32;
        int st = want_bits ? dev_grow(ws.hdx, ws.hdx_elems, (size_t)b.T * npk * g.n_vars) : LDPC_OK;
        if (st == LDPC_OK) st = ensure_bs_bad(ws, npk, ntiles_max);
        if (st != LDPC_OK) return st;
        BsOut o{};
        o.counters = counters;
        o.flags = flags;
        o.bad = ws.bs_bad;
        o.hdx = want_bits ? ws.hdx : nullptr;
        st = bs_decode(g, b, ws, llr, r, o, s);
        if (st != LDPC_OK) return st;
        ws.last_kernel = bs_kernel_name(g, r);
        ws.bits_packed = want_bits;
        if (b.q8) return LDPC_OK;      // generated channel: every pack is on the grid, nothing to fix up
        // test hook: LDPC_BS_FIXUP=0 skips the v5 fixup, so a test can tell that a batch was
        // decoded by the bit-sliced kernel alone (flagged packs then contribute nothing).  Read
        // per decode (a test sets it after other decodes ran in the same process).
        const char* fx = getenv("LDPC_BS_FIXUP");
        if (fx && atoi(fx) == 0) return LDPC_OK;
        return fused5_decode(g, b, ws, llr, mode_qmax(mode), step, cu, per_edge_w != 0, hd_out,
                             counters, flags, s, ws.bs_bad);
    }
    ws.last_kernel = fused5_shape_name(g, b.T);
    return fused5_decode(g, b, ws, llr, mode_qmax(mode), step, cu, per_edge_w != 0, hd_out,
                         counters, flags, s);
}

bool fused_bs_supported(const DevGraph& g, const BsReq& r) {
    if (r.es) return bs_supported(g, r);
    return fused_supported(g, r.mode, r.T, r.clip) && g.n_vars <= WORD_MAX_VARS && use_bs(g, r);
}

int fused_decode_bs(const DevGraph& g, const Bufs& b, FusedWorkspace& ws, const float* llr, const BsReq& r,
                    int64_t B_max, int ntiles_max, BsOut o, uint32_t* rows, uint8_t* word_flags, hipStream_t s,
                    const EventSink* ev) {
    // (word_out's LDS holds the 4 variables on 1024 lanes that bound every bit-sliced plan)
    const bool planes = rows || ev;
    if (!fused_bs_supported(g, r) || (planes && (g.n_vars > WORD_MAX_VARS || b.B > B_max))) return LDPC_ERR_UNSUPPORTED;
    if (b.q8 && !bs_q8_ok(g, r, reinterpret_cast<const AwgnParams*>(b.gen8)->ss > 0)) return LDPC_ERR_UNSUPPORTED;
    // the word modes' scratch: one word per (pack, variable) of the largest batch, whatever T is
    int st = planes ? dev_grow(ws.hdw, ws.hdw_elems, (size_t)((B_max + 31) / 32) * g.n_vars) : LDPC_OK;
    if (st == LDPC_OK) st = ensure_bs_bad(ws, (b.B + 31) / 32, ntiles_max);
    // (an event's record holds its n_iter: the early-stop decode writes it here when the caller takes none)
    if (st == LDPC_OK && ev && r.es && !o.n_iter) {
        st = dev_grow(ws.ev_niter, ws.ev_niter_n, (size_t)B_max);
        o.n_iter = ws.ev_niter;
    }
    if (st != LDPC_OK) return st;
    // (off-grid packs are marked -- by the kernel, in the rows by word_out --, not decoded: no v5
    // fixup, so none of its tile buffers)
    o.bad = ws.bs_bad;
    if (planes) {
        (r.es ? o.hdw : o.hdx) = ws.hdw;
        o.word = !r.es;
    }
    st = bs_decode(g, b, ws, llr, r, o, s);
    if (st != LDPC_OK || !planes) return st;
    if (ev) return events_out(g, ws.hdw, ws.bs_bad, b.B, r.es ? o.n_iter : nullptr, r.T, *ev, o.flags, s);
    return word_out(g, ws.hdw, ws.bs_bad, b.B, rows, word_flags, o.flags, s);
}

HdView fused_bits_view(const FusedWorkspace& ws) {
    HdView v{};
    v.tile = ws.hd;
    if (ws.bits_packed) {
        v.pack = ws.hdx;
        v.bad = ws.bs_bad;
    }
    return v;
}

void fused_free(FusedWorkspace& ws) {
    if (ws.hd) (void)hipFree(ws.hd);
    ws.hd = nullptr;
    ws.hd_elems = 0;
    if (ws.tables) (void)hipFree(ws.tables);
    ws.tables = nullptr;
    ws.tables_bytes = 0;
    if (ws.bs_graph) (void)hipFree(ws.bs_graph);
    ws.bs_graph = nullptr;
    if (ws.bs_es_graph) (void)hipFree(ws.bs_es_graph);
    ws.bs_es_graph = nullptr;
    if (ws.bs_lut) (void)hipFree(ws.bs_lut);
    ws.bs_lut = nullptr;
    ws.bs_lut_bytes = 0;
    if (ws.bs_bad) (void)hipFree(ws.bs_bad);
    ws.bs_bad = nullptr;
    ws.bs_bad_n = 0;
    if (ws.bs_ticket) (void)hipFree(ws.bs_ticket);
    ws.bs_ticket = nullptr;
    if (ws.hdx) (void)hipFree(ws.hdx);
    ws.hdx = nullptr;
    ws.hdx_elems = 0;
    ws.bits_packed = false;
    if (ws.hdw) (void)hipFree(ws.hdw);
    ws.hdw = nullptr;
    ws.hdw_elems = 0;
    if (ws.ev_niter) (void)hipFree(ws.ev_niter);
    ws.ev_niter = nullptr;
    ws.ev_niter_n = 0;
    ws.key_gad[0] = ws.key_qtab[0] = ws.key_bslut[0] = ~0ull;
}

}  // namespace ldpc
