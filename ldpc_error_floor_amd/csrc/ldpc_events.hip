// ldpc_events.hip — the event collector of the word modes (ldpc_decode_events): from
// the bit-sliced decode's hard decisions, one u32 per (pack, variable) with bit r = codeword
// 32 pack + r (FusedWorkspace::hdw, what word_out transposes), to one record per EVENT -- a frame
// whose word is nonzero anywhere over the n_vars variables -- appended to caller-owned buffers:
// the frame's index, {n_iter, a, a_target, b} (a: ones of the word, a_target: ones among the first
// target_bits, b: unsatisfied checks) and, optionally, the word.  A pack without an event costs one
// read of its plane words and nothing else.
#include <algorithm>

#include "ldpc_fused.h"

namespace ldpc {

namespace {

constexpr int EV_NT = 256;
constexpr int EV_NW = EV_NT / 64;      // waves per workgroup

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) x += __shfl_xor(x, j, 64);
    return x;
}

// One workgroup per pack (grid-stride).  Per pack:
//   nz     = OR of the pack's n_vars plane words & the valid-frame mask of a ragged last pack (the
//            decode kernels do not promise zero bits for the frames past B): wave OR, one LDS word
//            per wave (two sets, alternating by pack, so one barrier per pack suffices), and the
//            workgroup goes to its next pack when nz == 0;
//   else   P[32 nwords] takes the plane words (zero past n_vars) and S[n_checks] the syndrome words
//            as k_word_out forms them -- check (row i, index h) XORs P[j z + (h + shift) mod z] over
//            the row's proto edges --, thread 0 reserves popc(nz) slots with one atomicAdd, and for
//            each set bit r of nz (ascending; slot = base + rank) with slot < cap the workgroup sums
//            bit r over P (a, a_target) and S (b) and writes the record; word w of the row is one
//            ballot of (P[32 w + lane] >> r) & 1 over a 32-lane half wave.
// A pack the decode kernel marked off the grid (bad[pack]) was not decoded and is no event; its
// frame flags take 0x80 as word_out gives them.
__global__ void __launch_bounds__(EV_NT)
k_events(DevGraph g, const uint32_t* __restrict__ planes, const uint32_t* __restrict__ bad, int64_t B,
         int nwords, int target_bits, const uint8_t* __restrict__ n_iter, int T, int64_t frame_base,
         int64_t cap, unsigned long long* __restrict__ ev_count, int64_t* __restrict__ ev_frame,
         int32_t* __restrict__ ev_info, uint32_t* __restrict__ ev_word, uint8_t* __restrict__ frame_flags) {
    extern __shared__ uint32_t esm[];
    __shared__ uint32_t wor[2][EV_NW];
    __shared__ int red[EV_NW][3];
    __shared__ unsigned long long base_s;
    const int nv = g.n_vars, nvp = 32 * nwords, nc = g.n_checks;
    uint32_t* P = esm;
    uint32_t* S = P + nvp;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t npk = (B + 31) >> 5;
    int par2 = 0;
    for (int64_t pk = blockIdx.x; pk < npk; pk += gridDim.x) {
        const int64_t b0 = pk * 32;
        const int nvalid = (int)min<int64_t>(32, B - b0);
        if (bad[pk]) {                               // (workgroup-uniform)
            if (frame_flags && tid < nvalid) frame_flags[b0 + tid] = 0x80;
            continue;
        }
        const uint32_t* src = planes + (size_t)pk * nv;
        uint32_t x = 0u;
        for (int v = tid; v < nv; v += EV_NT) x |= src[v];
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) x |= (uint32_t)__shfl_xor((int)x, j, 64);
        if (lane == 0) wor[par2][wave] = x;
        __syncthreads();
        uint32_t nz = 0u;
#pragma unroll
        for (int w = 0; w < EV_NW; ++w) nz |= wor[par2][w];
        par2 ^= 1;                                   // (toggled per use: a skipped pack has no barrier)
        nz &= nvalid == 32 ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);
        if (nz == 0u) continue;                      // (workgroup-uniform) the common case

        for (int v = tid; v < nvp; v += EV_NT) P[v] = v < nv ? src[v] : 0u;
        if (tid == 0) base_s = atomicAdd(ev_count, (unsigned long long)__popc(nz));
        __syncthreads();
        for (int c = tid; c < nc; c += EV_NT) {
            const int i = c / g.z, h = c - i * g.z;
            uint32_t par = 0u;
            for (int pe = g.row_ptr[i]; pe < g.row_ptr[i + 1]; ++pe) {
                const int s = h + g.pe_shift[pe];
                par ^= P[g.pe_col[pe] * g.z + (s >= g.z ? s - g.z : s)];
            }
            S[c] = par;
        }
        __syncthreads();
        int64_t slot = (int64_t)base_s;
        for (uint32_t m = nz; m != 0u && slot < cap; m &= m - 1u, ++slot) {     // (uniform)
            const int r = __ffs((int)m) - 1;
            int a = 0, at = 0, b = 0;
            for (int v = tid; v < nv; v += EV_NT) {
                const int bit = (int)((P[v] >> r) & 1u);
                a += bit;
                at += v < target_bits ? bit : 0;
            }
            for (int c = tid; c < nc; c += EV_NT) b += (int)((S[c] >> r) & 1u);
            a = wave_sum(a);
            at = wave_sum(at);
            b = wave_sum(b);
            if (lane == 0) {
                red[wave][0] = a;
                red[wave][1] = at;
                red[wave][2] = b;
            }
            __syncthreads();
            if (tid == 0) {
                int sa = 0, sat = 0, sb = 0;
#pragma unroll
                for (int w = 0; w < EV_NW; ++w) {
                    sa += red[w][0];
                    sat += red[w][1];
                    sb += red[w][2];
                }
                ev_frame[slot] = frame_base + b0 + r;
                int32_t* info = ev_info + 4 * slot;
                info[0] = n_iter ? (int32_t)n_iter[b0 + r] : T;
                info[1] = sa;
                info[2] = sat;
                info[3] = sb;
            }
            if (ev_word) {
                uint32_t* row = ev_word + (size_t)slot * nwords;
                for (int w0 = 0; w0 < nwords; w0 += EV_NT / 32) {             // (uniform trip count)
                    const int w = w0 + (tid >> 5);
                    const unsigned long long bal = __ballot(w < nwords && ((P[w < nwords ? 32 * w + (tid & 31) : 0] >> r) & 1u));
                    if ((tid & 31) == 0 && w < nwords) row[w] = (uint32_t)(lane & 32 ? bal >> 32 : bal);
                }
            }
            __syncthreads();                         // red is the next event's
        }
        __syncthreads();                             // P, S and base_s are the next pack's
    }
}

}  // namespace

static size_t events_out_lds(const DevGraph& g) {
    const int nwords = (g.n_vars + 31) / 32;
    return sizeof(uint32_t) * ((size_t)32 * nwords + (size_t)g.n_checks);
}

int events_out(const DevGraph& g, const uint32_t* planes, const uint32_t* bad, int64_t B, const uint8_t* n_iter,
               int T, const EventSink& ev, uint8_t* frame_flags, hipStream_t s) {
    if (g.n_vars > WORD_MAX_VARS || g.n_checks > WORD_MAX_VARS) return LDPC_ERR_UNSUPPORTED;
    const int nwords = (g.n_vars + 31) / 32;
    const int64_t npk = (B + 31) / 32;
    hipLaunchKernelGGL(k_events, dim3((unsigned)std::min<int64_t>(npk, 65535)), dim3(EV_NT), events_out_lds(g), s, g,
                       planes, bad, B, nwords, ev.target_bits, n_iter, T, ev.frame_base, ev.cap,
                       reinterpret_cast<unsigned long long*>(ev.count), ev.frame, ev.info, ev.word, frame_flags);
    return hipGetLastError() == hipSuccess ? LDPC_OK : LDPC_ERR_HIP;
}

}  // namespace ldpc
