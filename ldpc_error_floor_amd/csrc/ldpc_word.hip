// ldpc_word.hip — the word mode's output kernel (ldpc_decode_word): from the
// bit-sliced decode's last-iteration hard decisions, one u32 per (pack, variable) with bit r =
// codeword 32 pack + r, to the decoded words [B][ceil(n_vars / 32)] (bit v % 32 of word v / 32) and
// the per-frame "syndrome nonzero" flag.
#include <algorithm>

#include "ldpc_fused.h"
#include "ldpc_bitplane.h"

namespace ldpc {

namespace {

constexpr int WORD_NT = 256;

// One workgroup per pack (grid-stride).  LDS: P[32 nwords] the pack's plane words (zero past
// n_vars), O[32][nwp] the transposed rows (nwp = nwords | 1: the 32 lanes of a word group write
// one column, stride nwp words, on 32 different banks), U the OR of the syndrome words.
//   syndrome: check (row i, index h) XORs P[j z + (h + shift) mod z] over the row's proto edges --
//             32 codewords per XOR -- and ORs the result into U;
//   transpose: lane r of a 32-lane group takes P[32 w + r] and five tr32_step exchanges leave it
//             with word w of codeword r; the rows then leave LDS in the order they have in memory
//             (a pack's rows are contiguous).
// A pack the decode kernel marked off the grid (bad[pack]) was not decoded: zero rows, 0x80 flags.
__global__ void __launch_bounds__(WORD_NT)
k_word_out(DevGraph g, const uint32_t* __restrict__ planes, const uint32_t* __restrict__ bad, int64_t B,
           int nwords, uint32_t* __restrict__ out, uint8_t* __restrict__ word_flags,
           uint8_t* __restrict__ frame_flags) {
    extern __shared__ uint32_t wsm[];
    const int nv = g.n_vars, nvp = 32 * nwords, nwp = nwords | 1;
    uint32_t* P = wsm;
    uint32_t* O = P + nvp;
    uint32_t* U = O + 32 * nwp;
    const int tid = threadIdx.x, r = tid & 31;
    const int64_t npk = (B + 31) >> 5;
    for (int64_t pk = blockIdx.x; pk < npk; pk += gridDim.x) {
        const int64_t b0 = pk * 32;
        const int nvalid = (int)min<int64_t>(32, B - b0);
        uint32_t* rows = out + (size_t)b0 * nwords;
        if (bad[pk]) {                               // (workgroup-uniform)
            for (int i = tid; i < nvalid * nwords; i += WORD_NT) rows[i] = 0u;
            if (tid < nvalid) {
                if (word_flags) word_flags[b0 + tid] = 0x80;
                if (frame_flags) frame_flags[b0 + tid] = 0x80;
            }
            continue;
        }
        const uint32_t* src = planes + (size_t)pk * nv;
        for (int v = tid; v < nvp; v += WORD_NT) P[v] = v < nv ? src[v] : 0u;
        if (tid == 0) *U = 0u;
        __syncthreads();
        if (word_flags) {
            uint32_t any = 0u;
            for (int c = tid; c < g.n_checks; c += WORD_NT) {
                const int i = c / g.z, h = c - i * g.z;
                uint32_t par = 0u;
                for (int pe = g.row_ptr[i]; pe < g.row_ptr[i + 1]; ++pe) {
                    const int s = h + g.pe_shift[pe];
                    par ^= P[g.pe_col[pe] * g.z + (s >= g.z ? s - g.z : s)];
                }
                any |= par;
            }
            if (any) atomicOr(U, any);
        }
        for (int w0 = 0; w0 < nwords; w0 += WORD_NT / 32) {       // (uniform trip count)
            const int w = w0 + (tid >> 5);
            uint32_t x = w < nwords ? P[32 * w + r] : 0u;
#pragma unroll
            for (int j = 16; j > 0; j >>= 1) x = bs::tr32_step(x, (uint32_t)__shfl_xor((int)x, j, 32), j, (r & j) != 0);
            if (w < nwords) O[r * nwp + w] = x;
        }
        __syncthreads();
        for (int i = tid; i < nvalid * nwords; i += WORD_NT) {
            const int row = i / nwords;
            rows[i] = O[row * nwp + (i - row * nwords)];
        }
        if (word_flags && tid < nvalid) word_flags[b0 + tid] = (uint8_t)((*U >> tid) & 1u);
        __syncthreads();                             // P, O and U are the next pack's
    }
}

}  // namespace

static size_t word_out_lds(int n_vars) {
    const int nwords = (n_vars + 31) / 32;
    return sizeof(uint32_t) * ((size_t)32 * nwords + (size_t)32 * (nwords | 1) + 1);
}

int word_out(const DevGraph& g, const uint32_t* planes, const uint32_t* bad, int64_t B, uint32_t* hard_last,
             uint8_t* word_flags, uint8_t* frame_flags, hipStream_t s) {
    const int nwords = (g.n_vars + 31) / 32;
    const int64_t npk = (B + 31) / 32;
    hipLaunchKernelGGL(k_word_out, dim3((unsigned)std::min<int64_t>(npk, 65535)), dim3(WORD_NT),
                       word_out_lds(g.n_vars), s, g, planes, bad, B, nwords, hard_last, word_flags, frame_flags);
    return hipGetLastError() == hipSuccess ? LDPC_OK : LDPC_ERR_HIP;
}

}  // namespace ldpc
