// Row LayerNorm over the feature axis of [T][d] (gfx950), forward and backward: a wave per row in general, 16 lanes per
// row for narrow rows (d <= 64, d % 4 == 0, 16-byte aligned operands).  The backward leaves d(gamma), d(beta) partials per
// block; gt_slab_reduce sums them in a fixed order.
#include "gt_common.h"

namespace gt {

// one wave per row, 4 rows per block
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int T, int d,
                                                            float eps, float* __restrict__ y,
                                                            float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    if (row >= T) return;
    const float* xr = x + (int64_t)row * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) s += xr[j];
    const float mu = wave_sum(s) / d;
    float v = 0.f;
    for (int j = lane; j < d; j += 64) { const float c = xr[j] - mu; v += c * c; }
    const float rstd = 1.f / sqrtf(wave_sum(v) / d + eps);
    float* yr = y + (int64_t)row * d;
    for (int j = lane; j < d; j += 64) yr[j] = (xr[j] - mu) * rstd * gamma[j] + beta[j];
    if (lane == 0) { stats[2 * (int64_t)row] = mu; stats[2 * (int64_t)row + 1] = rstd; }
}

// Narrow rows (d <= 64, d % 4 == 0; ex4's d = 48): a row is 16 lanes x one float4 each, four rows per wave -- the generic
// kernels below spend a wave, twelve cross-lane exchanges and (backward) an LDS read-modify-write per element on one 192-byte
// row (layernorm_bwd 50.6 us, layernorm_fwd 19.1 us for [65536, 48]: profiles/r06e_rocprofv3_steady_ex4_ns_after_dkv_fin.txt).
__device__ __forceinline__ float group16_sum(float v) {
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
    return v;
}
__global__ __launch_bounds__(256) void layernorm_fwd16_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int T, int d, float eps,
                                                              float* __restrict__ y, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, q = lane & 15, rg = (threadIdx.x >> 4);      // 16 row slots per block
    const bool on = 4 * q < d;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 g = on ? *reinterpret_cast<const f32x4*>(gamma + 4 * q) : z;
    const f32x4 be = on ? *reinterpret_cast<const f32x4*>(beta + 4 * q) : z;
    const float inv_d = 1.f / (float)d;
    for (int64_t row = (int64_t)blockIdx.x * 16 + rg; row < T; row += (int64_t)gridDim.x * 16) {
        const f32x4 v = on ? *reinterpret_cast<const f32x4*>(x + row * d + 4 * q) : z;
        const float mu = group16_sum((v[0] + v[1]) + (v[2] + v[3])) * inv_d;
        f32x4 c = v - mu;
        if (!on) c = z;
        const float var = group16_sum((c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3])) * inv_d;
        const float rstd = 1.f / sqrtf(var + eps);
        if (on) *reinterpret_cast<f32x4*>(y + row * d + 4 * q) = c * rstd * g + be;
        if (q == 0) { stats[2 * row] = mu; stats[2 * row + 1] = rstd; }
    }
}
__global__ __launch_bounds__(256) void layernorm_bwd16_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ stats, int T, int d, float* __restrict__ dx, float* __restrict__ partial /* [nblk][2][d] */) {
    __shared__ __attribute__((aligned(16))) float red[4][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane & 15, rg = (threadIdx.x >> 4);
    const bool on = 4 * q < d;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 g = on ? *reinterpret_cast<const f32x4*>(gamma + 4 * q) : z;
    const float inv_d = 1.f / (float)d;
    f32x4 mg = z, mb = z;
    for (int64_t row = (int64_t)blockIdx.x * 16 + rg; row < T; row += (int64_t)gridDim.x * 16) {
        const float mu = stats[2 * row], rstd = stats[2 * row + 1];
        const f32x4 xv = on ? *reinterpret_cast<const f32x4*>(x + row * d + 4 * q) : z;
        const f32x4 gr = on ? *reinterpret_cast<const f32x4*>(dy + row * d + 4 * q) : z;
        f32x4 xh = (xv - mu) * rstd;
        if (!on) xh = z;
        const f32x4 gg = gr * g, gx = gg * xh;
        const float a1 = group16_sum((gg[0] + gg[1]) + (gg[2] + gg[3])) * inv_d;
        const float a2 = group16_sum((gx[0] + gx[1]) + (gx[2] + gx[3])) * inv_d;
        mg += gr * xh;
        mb += gr;
        if (on) *reinterpret_cast<f32x4*>(dx + row * d + 4 * q) = (gg - a1 - xh * a2) * rstd;
    }
    // the wave's four row slots (lanes q, q + 16, q + 32, q + 48), then the four waves through LDS: fixed order
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        mg[c] += __shfl_xor(mg[c], 16, 64); mg[c] += __shfl_xor(mg[c], 32, 64);
        mb[c] += __shfl_xor(mb[c], 16, 64); mb[c] += __shfl_xor(mb[c], 32, 64);
    }
    if (lane < 16) {
        *reinterpret_cast<f32x4*>(&red[w][0][4 * q]) = mg;
        *reinterpret_cast<f32x4*>(&red[w][1][4 * q]) = mb;
    }
    __syncthreads();
    float* pg = partial + (int64_t)blockIdx.x * 2 * d;
    for (int jj = threadIdx.x; jj < 2 * d; jj += blockDim.x) {
        const int which = jj / d, col = jj % d;
        pg[jj] = (red[0][which][col] + red[1][which][col]) + (red[2][which][col] + red[3][which][col]);
    }
}
static inline bool ln_narrow(const void* a, const void* b, const void* c, int d) {
    return d <= 64 && d % 4 == 0 && !misaligned16(a, b, c);
}

constexpr int LN_ROWS = 64;   // rows per block in backward (partial dgamma/dbeta per block)
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ stats, int T, int d, float* __restrict__ dx,
    float* __restrict__ partial /* [nblk][2][d] */) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [4][2][d]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* mg = lds + (w * 2) * d;
    float* mb = mg + d;
    for (int j = lane; j < d; j += 64) { mg[j] = 0.f; mb[j] = 0.f; }
    for (int r0 = blockIdx.x * LN_ROWS; r0 < T; r0 += gridDim.x * LN_ROWS) {
    const int r1 = min(T, r0 + LN_ROWS);
    for (int row = r0 + w; row < r1; row += 4) {
        const float mu = stats[2 * (int64_t)row], rstd = stats[2 * (int64_t)row + 1];
        const float* xr = x + (int64_t)row * d;
        const float* gr = dy + (int64_t)row * d;
        float a1 = 0.f, a2 = 0.f;
        for (int j = lane; j < d; j += 64) {
            const float xh = (xr[j] - mu) * rstd, gg = gr[j] * gamma[j];
            a1 += gg;
            a2 += gg * xh;
            mg[j] += gr[j] * xh;
            mb[j] += gr[j];
        }
        a1 = wave_sum(a1) / d;
        a2 = wave_sum(a2) / d;
        float* dr = dx + (int64_t)row * d;
        for (int j = lane; j < d; j += 64) {
            const float xh = (xr[j] - mu) * rstd;
            dr[j] = rstd * (gr[j] * gamma[j] - a1 - xh * a2);
        }
    }
    }   // row groups
    __syncthreads();
    float* pg = partial + (int64_t)blockIdx.x * 2 * d;
    for (int j = threadIdx.x; j < 2 * d; j += blockDim.x)
        pg[j] = lds[j] + lds[2 * d + j] + lds[4 * d + j] + lds[6 * d + j];
}

constexpr int LN_MAXB = 512;
static inline int ln_blocks_bwd(int T) { return std::min(ceil_div(T, LN_ROWS), LN_MAXB); }

}  // namespace gt

using namespace gt;

extern "C" int gt_layernorm_fwd(const float* x, const float* gamma, const float* beta, int32_t T, int32_t d,
                                float eps, float* y, float* stats, void* stream) {
    if (!x || !gamma || !beta || !y || !stats || T <= 0 || d <= 0) return GT_EINVAL;
    if (ln_narrow(x, y, gamma, d) && !misaligned16(beta))
        hipLaunchKernelGGL(layernorm_fwd16_kernel, dim3(std::min(ceil_div(T, 16), 4096)), dim3(256), 0, (hipStream_t)stream, x,
                           gamma, beta, T, d, eps, y, stats);
    else
        hipLaunchKernelGGL(layernorm_fwd_kernel, dim3(ceil_div(T, 4)), dim3(256), 0, (hipStream_t)stream, x,
                           gamma, beta, T, d, eps, y, stats);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_layernorm_bwd_ws_bytes(int32_t T, int32_t d) {
    return (int64_t)ln_blocks_bwd(T) * 2 * d * (int64_t)sizeof(float);
}

extern "C" int gt_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* stats,
                                int32_t T, int32_t d, float* dx, float* dgamma, float* dbeta, void* ws,
                                int64_t ws_bytes, void* stream) {
    if (!dy || !x || !gamma || !stats || !dx || !dgamma || !dbeta || T <= 0 || d <= 0) return GT_EINVAL;
    if (!ws || ws_bytes < gt_layernorm_bwd_ws_bytes(T, d)) return GT_EWS;
    const int nblk = ln_blocks_bwd(T);
    const size_t lds = (size_t)8 * d * sizeof(float);
    if (lds > 64 * 1024) return GT_ENOTSUP;
    float* partial = reinterpret_cast<float*>(ws);
    if (ln_narrow(dy, x, dx, d) && !misaligned16(gamma))
        hipLaunchKernelGGL(layernorm_bwd16_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, stats, T, d,
                           dx, partial);
    else
        hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(nblk), dim3(256), lds, (hipStream_t)stream, dy, x, gamma,
                           stats, T, d, dx, partial);
    GT_LAUNCH_CHECK();
    if (int rc = gt_slab_reduce(partial, 2 * d, nblk, d, 1.f, dgamma, stream)) return rc;
    return gt_slab_reduce(partial + d, 2 * d, nblk, d, 1.f, dbeta, stream);
}
