// ldpc_llr8.hip — int8 quantized LLRs: the QMS channel written as int8 rows and
// the float -> int8 conversion.  The decode of such rows is the bit-sliced kernels' L8 build
// (ldpc_bs_kernel.h, ldpc_bsc.hip); the byte format is include/ldpc_nms.h's.
#include <algorithm>

#include "ldpc_awgn.h"
#include "ldpc_internal.h"

namespace ldpc {

// k_awgn_qf (ldpc_channel.hip) with byte rows: one thread per (global codeword quad, variable),
// the same Philox call and level sampler, the level stored as its grid index level + kmin
// (ldpc_channel_awgn stores val[level] = (level + kmin) step); punctured bits 0, shortened -128
__global__ void __launch_bounds__(256) k_awgn_q8(int8_t* __restrict__ out, int64_t B, int n_vars,
                                                 AwgnParams a) {
    __shared__ uint2 bucket[1 << AWGN_KB];
    __shared__ uint32_t thi[AWGN_NB_MAX], tlo[AWGN_NB_MAX];
    awgn_bucket_fill2(a, bucket, thi, tlo, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint64_t g0 = (uint64_t)a.offset;
    const uint64_t q0 = g0 >> 2;
    const int64_t nq = (int64_t)(((g0 + (uint64_t)B - 1) >> 2) - q0 + 1);
    const int64_t id0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t S = (int64_t)gridDim.x * blockDim.x;
    int64_t m = id0 / n_vars;
    int v = (int)(id0 - m * n_vars);
    const int64_t dm = S / n_vars;
    const int dv = (int)(S - dm * n_vars);
    for (; m < nq; m += dm) {
        const uint64_t gq = q0 + (uint64_t)m;
        const int64_t bq = (int64_t)(gq * 4 - g0);          // batch index of the quad's word 0
        const int fx = awgn_fixed(a, v + 1);
        int l[4];
        if (fx == 0) {
            awgn_levels4b(a, bucket, thi, tlo, (uint32_t)v, gq, l);
#pragma unroll
            for (int j = 0; j < 4; ++j) l[j] += a.kmin;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) l[j] = fx == 1 ? 0 : -128;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (bq + j >= 0 && bq + j < B) out[(bq + j) * n_vars + v] = (int8_t)l[j];
        v += dv;
        if (v >= n_vars) {
            v -= n_vars;
            ++m;
        }
    }
}

// float LLRs -> int8 grid values, one element per thread, grid-strided.  On the grid: x = llr *
// inv equals its rounding and lies within +-qmax (the bit-sliced kernels' test, pack_channel);
// -+clip: the markers; anything else is stored saturated and counted (one atomic per wave)
__global__ void __launch_bounds__(256) k_llr_to_q8(const float* __restrict__ llr, int64_t n, float inv, int qmax,
                                                   float clip, int8_t* __restrict__ out,
                                                   unsigned long long* __restrict__ n_invalid) {
    const float qf = (float)qmax;
    unsigned bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float l = llr[i];
        const float x = l * inv;
        const float q = __builtin_amdgcn_fmed3f(rintf(x), -qf, qf);   // (NaN: -qmax, and counted)
        int8_t b = (int8_t)(int)q;
        if (!(q == x)) {
            if (l == -clip) b = -128;
            else if (l == clip) b = 127;
            else ++bad;
        }
        out[i] = b;
    }
    if (n_invalid) {
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o);
        if ((threadIdx.x & 63) == 0 && bad) atomicAdd(n_invalid, (unsigned long long)bad);
    }
}

}  // namespace ldpc

static bool q8_grid(int32_t q_bit, float* step, int* qmax) {
    switch (q_bit) {
        case 5: *step = 0.5f; *qmax = 15; return true;
        case -5: *step = 1.0f; *qmax = 15; return true;
        case 4: *step = 1.0f; *qmax = 7; return true;
        case 3: *step = 2.0f; *qmax = 3; return true;
        default: return false;
    }
}

extern "C" int ldpc_channel_awgn_q8(int8_t* q8_dev, int64_t B, int32_t n_vars, double sigma, uint64_t seed,
                                    int64_t offset, int32_t q_bit, int32_t punct_start, int32_t punct_end,
                                    int32_t short_start, int32_t short_end, void* stream) {
    if (!q8_dev) return LDPC_ERR_ARG;
    // (the clip value is no part of the bytes: a shortened bit is the marker)
    const int chk = ldpc::host::check_channel(B, n_vars, sigma, offset, LDPC_DEC_QMS, q_bit, punct_start, punct_end,
                                              short_start, short_end, 1.0f);
    if (chk != LDPC_OK) return chk;
    float step;
    int qmax;
    if (!q8_grid(q_bit, &step, &qmax)) return LDPC_ERR_UNSUPPORTED;
    const ldpc::AwgnParams a = ldpc::make_awgn(sigma, seed, offset, LDPC_DEC_QMS, q_bit, punct_start, punct_end,
                                               short_start, short_end, 1.0f);
    const int64_t nq = (int64_t)((((uint64_t)offset + (uint64_t)B - 1) >> 2) - ((uint64_t)offset >> 2) + 1);
    const int64_t total = nq * n_vars;
    const unsigned grid = (unsigned)std::min<int64_t>(8192, (total + 255) / 256);
    hipLaunchKernelGGL(ldpc::k_awgn_q8, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), q8_dev, B,
                       (int)n_vars, a);
    return hipGetLastError() == hipSuccess ? LDPC_OK : LDPC_ERR_HIP;
}

extern "C" int ldpc_llr_to_q8(const float* llr_dev, int64_t n, int32_t q_bit, float clip_llr, int8_t* q8_dev,
                              int64_t* n_invalid_dev, void* stream) {
    if (n < 0 || (n > 0 && (!llr_dev || !q8_dev)) || !(clip_llr > 0.f)) return LDPC_ERR_ARG;
    float step;
    int qmax;
    if (!q8_grid(q_bit, &step, &qmax)) return LDPC_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n_invalid_dev && hipMemsetAsync(n_invalid_dev, 0, sizeof(int64_t), s) != hipSuccess) return LDPC_ERR_HIP;
    if (n == 0) return LDPC_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(8192, (n + 255) / 256);
    hipLaunchKernelGGL(ldpc::k_llr_to_q8, dim3(grid), dim3(256), 0, s, llr_dev, n, 1.0f / step, qmax, clip_llr, q8_dev,
                       reinterpret_cast<unsigned long long*>(n_invalid_dev));
    return hipGetLastError() == hipSuccess ? LDPC_OK : LDPC_ERR_HIP;
}
