// 2x2 average pool with the activation behind it, forward and backward (gfx950): nn.AvgPool2d(2) -> activation of the
// reference's Conv2dEncoder (libs/layers.py:329-341), with the channels-first <-> channels-last change of the scaler boundary
// fused in.  The pool floors: an odd trailing row / column of the input is not read and gets a zero gradient.
//   forward : one thread per output value (a float4 of channels when both sides are channels-last, two neighbouring outputs of
//             a row when both are channels-first and W % 4 == 0, one value otherwise), grid-stride over the whole tensor;
//   backward: one thread per 2x2 input CELL of the ceil(H/2) x ceil(W/2) cell grid, which owns the (up to) four dx values of
//             its cell -- every dx value is written exactly once, the cells of a dropped row / column write zeros.  The pooled
//             value is recomputed from x (four loads) instead of being kept by the forward.
// Plain vector loads and stores, no LDS, no atomics; the caller's stream, no allocation.
#include "gt_common.h"

namespace gt {

struct PoolP {
    int B, C, H, W, Ho, Wo;
};

__device__ __forceinline__ float pool_act(int act, float v) {
    return act == GT_ACT_SILU ? silu_f(v) : (act == GT_ACT_RELU ? fmaxf(v, 0.f) : v);
}
__device__ __forceinline__ float pool_dact(int act, float v) {
    return act == GT_ACT_SILU ? dsilu_f(v) : (act == GT_ACT_RELU ? (v > 0.f ? 1.f : 0.f) : 1.f);
}
// the summation order of every variant: (top-left + top-right) + (bottom-left + bottom-right)
__device__ __forceinline__ float pool4(float a, float b, float c, float d) { return 0.25f * ((a + b) + (c + d)); }

template <bool NHWC>
__device__ __forceinline__ int64_t pool_at(int C, int Hh, int Ww, int b, int c, int y, int x) {
    return NHWC ? (((int64_t)b * Hh + y) * Ww + x) * C + c : (((int64_t)b * C + c) * Hh + y) * Ww + x;
}

// ---- any layout pair, one value per thread; the index runs in the order of the OUTPUT layout (forward) / INPUT layout (backward)
template <bool IN_NHWC, bool OUT_NHWC>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, PoolP p, int act) {
    const int64_t total = (int64_t)p.B * p.C * p.Ho * p.Wo, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        int c, ox, oy;
        if (OUT_NHWC) { c = (int)(r % p.C); r /= p.C; ox = (int)(r % p.Wo); r /= p.Wo; oy = (int)(r % p.Ho); r /= p.Ho; }
        else { ox = (int)(r % p.Wo); r /= p.Wo; oy = (int)(r % p.Ho); r /= p.Ho; c = (int)(r % p.C); r /= p.C; }
        const int b = (int)r;
        const int64_t s = pool_at<IN_NHWC>(p.C, p.H, p.W, b, c, 2 * oy, 2 * ox);
        const int64_t dxs = IN_NHWC ? p.C : 1, dys = IN_NHWC ? (int64_t)p.W * p.C : p.W;
        y[i] = pool_act(act, pool4(x[s], x[s + dxs], x[s + dys], x[s + dys + dxs]));
    }
}

template <bool IN_NHWC, bool OUT_NHWC>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ dx, PoolP p, int act) {
    const int Hc = (p.H + 1) >> 1, Wc = (p.W + 1) >> 1;
    const int64_t total = (int64_t)p.B * p.C * Hc * Wc, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        int c, cx, cy;
        if (IN_NHWC) { c = (int)(r % p.C); r /= p.C; cx = (int)(r % Wc); r /= Wc; cy = (int)(r % Hc); r /= Hc; }
        else { cx = (int)(r % Wc); r /= Wc; cy = (int)(r % Hc); r /= Hc; c = (int)(r % p.C); r /= p.C; }
        const int b = (int)r;
        const int64_t s = pool_at<IN_NHWC>(p.C, p.H, p.W, b, c, 2 * cy, 2 * cx);
        const int64_t dxs = IN_NHWC ? p.C : 1, dys = IN_NHWC ? (int64_t)p.W * p.C : p.W;
        const bool right = 2 * cx + 1 < p.W, below = 2 * cy + 1 < p.H;
        float g = 0.f;
        if (cy < p.Ho && cx < p.Wo) {       // a whole cell: all four positions exist
            const float v = pool4(x[s], x[s + dxs], x[s + dys], x[s + dys + dxs]);
            g = 0.25f * pool_dact(act, v) * dy[pool_at<OUT_NHWC>(p.C, p.Ho, p.Wo, b, c, cy, cx)];
        }
        dx[s] = g;
        if (right) dx[s + dxs] = g;
        if (below) dx[s + dys] = g;
        if (right && below) dx[s + dys + dxs] = g;
    }
}

// ---- channels-last on both sides, C % 4 == 0: a float4 of channels per thread
__global__ __launch_bounds__(256) void pool_fwd_nhwc4_kernel(const float* __restrict__ x, float* __restrict__ y, PoolP p, int act) {
    const int C4 = p.C >> 2;
    const int64_t total = (int64_t)p.B * p.Ho * p.Wo * C4, nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t dys = (int64_t)p.W * p.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        const int c = 4 * (int)(r % C4); r /= C4;
        const int ox = (int)(r % p.Wo); r /= p.Wo;
        const int oy = (int)(r % p.Ho); r /= p.Ho;
        const float* s = x + pool_at<true>(p.C, p.H, p.W, (int)r, c, 2 * oy, 2 * ox);
        const f32x4 a = *reinterpret_cast<const f32x4*>(s), bq = *reinterpret_cast<const f32x4*>(s + p.C);
        const f32x4 cq = *reinterpret_cast<const f32x4*>(s + dys), d = *reinterpret_cast<const f32x4*>(s + dys + p.C);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pool_act(act, pool4(a[j], bq[j], cq[j], d[j]));
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
}

__global__ __launch_bounds__(256) void pool_bwd_nhwc4_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ dx, PoolP p, int act) {
    const int C4 = p.C >> 2, Hc = (p.H + 1) >> 1, Wc = (p.W + 1) >> 1;
    const int64_t total = (int64_t)p.B * Hc * Wc * C4, nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t dys = (int64_t)p.W * p.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        const int c = 4 * (int)(r % C4); r /= C4;
        const int cx = (int)(r % Wc); r /= Wc;
        const int cy = (int)(r % Hc); r /= Hc;
        const int b = (int)r;
        const int64_t s = pool_at<true>(p.C, p.H, p.W, b, c, 2 * cy, 2 * cx);
        const bool right = 2 * cx + 1 < p.W, below = 2 * cy + 1 < p.H;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (cy < p.Ho && cx < p.Wo) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(x + s), bq = *reinterpret_cast<const f32x4*>(x + s + p.C);
            const f32x4 cq = *reinterpret_cast<const f32x4*>(x + s + dys), d = *reinterpret_cast<const f32x4*>(x + s + dys + p.C);
            const f32x4 gy = *reinterpret_cast<const f32x4*>(dy + pool_at<true>(p.C, p.Ho, p.Wo, b, c, cy, cx));
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = 0.25f * pool_dact(act, pool4(a[j], bq[j], cq[j], d[j])) * gy[j];
        }
        *reinterpret_cast<f32x4*>(dx + s) = g;
        if (right) *reinterpret_cast<f32x4*>(dx + s + p.C) = g;
        if (below) *reinterpret_cast<f32x4*>(dx + s + dys) = g;
        if (right && below) *reinterpret_cast<f32x4*>(dx + s + dys + p.C) = g;
    }
}

// ---- channels-first on both sides, W % 4 == 0 (so no column is dropped): two neighbouring cells of a row per thread
__global__ __launch_bounds__(256) void pool_fwd_nchw2_kernel(const float* __restrict__ x, float* __restrict__ y, PoolP p, int act) {
    const int W2 = p.Wo >> 1;
    const int64_t total = (int64_t)p.B * p.C * p.Ho * W2, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        const int ox = 2 * (int)(r % W2); r /= W2;
        const int oy = (int)(r % p.Ho); r /= p.Ho;          // r: the (b, c) plane
        const float* s = x + (r * p.H + 2 * oy) * p.W + 2 * ox;
        const f32x4 t = *reinterpret_cast<const f32x4*>(s), u = *reinterpret_cast<const f32x4*>(s + p.W);
        const f32x2 o = {pool_act(act, pool4(t[0], t[1], u[0], u[1])), pool_act(act, pool4(t[2], t[3], u[2], u[3]))};
        *reinterpret_cast<f32x2*>(y + (r * p.Ho + oy) * p.Wo + ox) = o;
    }
}

__global__ __launch_bounds__(256) void pool_bwd_nchw2_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ dx, PoolP p, int act) {
    const int W2 = p.Wo >> 1, Hc = (p.H + 1) >> 1;
    const int64_t total = (int64_t)p.B * p.C * Hc * W2, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        const int cx = 2 * (int)(r % W2); r /= W2;
        const int cy = (int)(r % Hc); r /= Hc;
        const int64_t s = (r * p.H + 2 * cy) * p.W + 2 * cx;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (cy < p.Ho) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(x + s), u = *reinterpret_cast<const f32x4*>(x + s + p.W);
            const f32x2 gy = *reinterpret_cast<const f32x2*>(dy + (r * p.Ho + cy) * p.Wo + cx);
            const float g0 = 0.25f * pool_dact(act, pool4(t[0], t[1], u[0], u[1])) * gy[0];
            const float g1 = 0.25f * pool_dact(act, pool4(t[2], t[3], u[2], u[3])) * gy[1];
            g = f32x4{g0, g0, g1, g1};
            *reinterpret_cast<f32x4*>(dx + s + p.W) = g;
        }
        *reinterpret_cast<f32x4*>(dx + s) = g;        // (cy == Ho: the dropped last row, zeros)
    }
}

static inline int pool_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

static int pool_check(const void* x, const void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t act) {
    if (!x || !y || B <= 0 || C <= 0 || H < 2 || W < 2) return GT_EINVAL;     // (H or W of 1: the pooled map would be empty)
    if (act != GT_ACT_NONE && act != GT_ACT_RELU && act != GT_ACT_SILU) return GT_EINVAL;
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" int gt_avgpool2_act_fwd(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t in_nhwc,
                                   int32_t out_nhwc, int32_t act, void* stream) {
    if (int rc = pool_check(x, y, B, C, H, W, act)) return rc;
    const PoolP p{B, C, H, W, H / 2, W / 2};
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)B * C * p.Ho * p.Wo;
    const bool al = !misaligned16(x, y);
    if (in_nhwc && out_nhwc && al && (C & 3) == 0)
        hipLaunchKernelGGL(pool_fwd_nhwc4_kernel, dim3(pool_grid(n / 4)), dim3(256), 0, st, x, y, p, act);
    else if (!in_nhwc && !out_nhwc && al && (W & 3) == 0)
        hipLaunchKernelGGL(pool_fwd_nchw2_kernel, dim3(pool_grid(n / 2)), dim3(256), 0, st, x, y, p, act);
    else if (in_nhwc && out_nhwc)
        hipLaunchKernelGGL((pool_fwd_kernel<true, true>), dim3(pool_grid(n)), dim3(256), 0, st, x, y, p, act);
    else if (in_nhwc)
        hipLaunchKernelGGL((pool_fwd_kernel<true, false>), dim3(pool_grid(n)), dim3(256), 0, st, x, y, p, act);
    else if (out_nhwc)
        hipLaunchKernelGGL((pool_fwd_kernel<false, true>), dim3(pool_grid(n)), dim3(256), 0, st, x, y, p, act);
    else
        hipLaunchKernelGGL((pool_fwd_kernel<false, false>), dim3(pool_grid(n)), dim3(256), 0, st, x, y, p, act);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_avgpool2_act_bwd(const float* x, const float* dy, float* dx, int32_t B, int32_t C, int32_t H, int32_t W,
                                   int32_t in_nhwc, int32_t out_nhwc, int32_t act, void* stream) {
    if (int rc = pool_check(x, dx, B, C, H, W, act)) return rc;
    if (!dy) return GT_EINVAL;
    const PoolP p{B, C, H, W, H / 2, W / 2};
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)B * C * ((H + 1) / 2) * ((W + 1) / 2);       // cells
    const bool al = !misaligned16(x, dy, dx);
    if (in_nhwc && out_nhwc && al && (C & 3) == 0)
        hipLaunchKernelGGL(pool_bwd_nhwc4_kernel, dim3(pool_grid(n / 4)), dim3(256), 0, st, x, dy, dx, p, act);
    else if (!in_nhwc && !out_nhwc && al && (W & 3) == 0)
        hipLaunchKernelGGL(pool_bwd_nchw2_kernel, dim3(pool_grid(n / 2)), dim3(256), 0, st, x, dy, dx, p, act);
    else if (in_nhwc && out_nhwc)
        hipLaunchKernelGGL((pool_bwd_kernel<true, true>), dim3(pool_grid(n)), dim3(256), 0, st, x, dy, dx, p, act);
    else if (in_nhwc)
        hipLaunchKernelGGL((pool_bwd_kernel<true, false>), dim3(pool_grid(n)), dim3(256), 0, st, x, dy, dx, p, act);
    else if (out_nhwc)
        hipLaunchKernelGGL((pool_bwd_kernel<false, true>), dim3(pool_grid(n)), dim3(256), 0, st, x, dy, dx, p, act);
    else
        hipLaunchKernelGGL((pool_bwd_kernel<false, false>), dim3(pool_grid(n)), dim3(256), 0, st, x, dy, dx, p, act);
    GT_LAUNCH_CHECK();
    return 0;
}
