// The 2-D training objective (reference: libs/ft.py:983-1105, WeightedL2Loss2d): relative L2 error plus the
// gamma h H1-seminorm regulariser on dilated central differences, per sample, forward and backward.  HBM-bound: the forward
// reads P, T, G, K once and writes four floats per block; the backward reads them again and writes dP once.  The stencil's
// neighbours of P (and, in the backward, of K and G) come through the cache.
//   forward : per-block partial sums (A, E, Gs, R) in ws, block order fixed          (h1loss2d_partial_kernel)
//   final   : the partials of a sample summed in block order, in double; the four per-sample scalars (h1loss2d_final_kernel)
//   backward: a gather -- every pixel of dP recomputes the at most four residuals it feeds; no atomics (h1loss2d_bwd_kernel)
// The flat pixel range of a sample is walked in groups of four pixels whose GLOBAL index is a multiple of four, so that a
// group inside the sample is one 16-byte access of T, K, dP (two of G) whatever n is; the at most two groups that straddle a
// sample boundary, and every tensor off a 16-byte boundary, take scalar accesses under a mask.
#include <algorithm>

#include "gt_common.h"

namespace gt {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_ITER = 2;                                // groups of four pixels per thread
constexpr int LOSS_GROUPS = LOSS_THREADS * LOSS_ITER;       // per block

// groups a sample can touch: M / 4 whole ones plus one straddling group at either end
inline int loss_blocks(int64_t M) { return (int)(((M >> 2) + 2 + LOSS_GROUPS - 1) / LOSS_GROUPS); }

struct LossP {
    const float* P; int64_t ldp;        // prediction, pixel pitch in floats
    const float* T; const float* G; const float* K;
    int n, s;                           // grid size, half dilation
    int64_t M;                          // n * n
    int nblk;                           // blocks per sample
    float inv_dh;                       // 1 / (d h)
    bool vec, pvec;                     // T, G, K (and dP) / P may be accessed 16 bytes at a time
};

// one group: the four pixels q0 .. q0 + 3 of sample b (q0 may be -3 .. M - 1); ok[e] marks those inside the sample
struct LossGroup {
    float p[4], t[4], gx[4], gy[4], k[4];
    bool ok[4];
};

template <bool HASG>
__device__ __forceinline__ void loss_load_group(const LossP& a, int64_t base, int64_t q0, LossGroup& v) {
    const bool full = q0 >= 0 && q0 + 4 <= a.M;
#pragma unroll
    for (int e = 0; e < 4; ++e) v.ok[e] = q0 + e >= 0 && q0 + e < a.M;
    const int64_t x = base + q0;
    if (full && a.vec) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(a.T + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) v.t[e] = t[e];
        if (HASG) {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.G + 2 * x), g1 = *reinterpret_cast<const f32x4*>(a.G + 2 * x + 4);
            v.gx[0] = g0[0]; v.gy[0] = g0[1]; v.gx[1] = g0[2]; v.gy[1] = g0[3];
            v.gx[2] = g1[0]; v.gy[2] = g1[1]; v.gx[3] = g1[2]; v.gy[3] = g1[3];
            if (a.K) {
                const f32x4 k = *reinterpret_cast<const f32x4*>(a.K + x);
#pragma unroll
                for (int e = 0; e < 4; ++e) v.k[e] = k[e];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v.t[e] = v.ok[e] ? a.T[x + e] : 0.f;
            if (HASG) {
                v.gx[e] = v.ok[e] ? a.G[2 * (x + e)] : 0.f;
                v.gy[e] = v.ok[e] ? a.G[2 * (x + e) + 1] : 0.f;
                if (a.K) v.k[e] = v.ok[e] ? a.K[x + e] : 0.f;
            }
        }
    }
    if (!HASG || !a.K) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v.k[e] = 1.f;
    }
    if (full && a.pvec) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(a.P + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) v.p[e] = p[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v.p[e] = v.ok[e] ? a.P[(x + e) * a.ldp] : 0.f;
    }
}

__device__ __forceinline__ bool loss_interior(const LossP& a, int i, int j) {
    return i >= a.s && i < a.n - a.s && j >= a.s && j < a.n - a.s;
}
// D_x P and D_y P at the centre (i, j) of an interior stencil; Pb is the sample's first pixel
__device__ __forceinline__ float loss_dx(const LossP& a, const float* __restrict__ Pb, int i, int j) {
    return (Pb[((int64_t)(i + a.s) * a.n + j) * a.ldp] - Pb[((int64_t)(i - a.s) * a.n + j) * a.ldp]) * a.inv_dh;
}
__device__ __forceinline__ float loss_dy(const LossP& a, const float* __restrict__ Pb, int i, int j) {
    return (Pb[((int64_t)i * a.n + j + a.s) * a.ldp] - Pb[((int64_t)i * a.n + j - a.s) * a.ldp]) * a.inv_dh;
}

// MODE 0: no G (A, E only) * 1: G present, norms only (A, E, Gs) * 2: G present and the regulariser (A, E, Gs, R)
// partial[(b * nblk + blk) * 4 + {0, 1, 2, 3}] = this block's share of (A, E, Gs, R); every block writes its four values
template <int MODE>
__global__ __launch_bounds__(LOSS_THREADS) void h1loss2d_partial_kernel(const LossP a, float* __restrict__ partial) {
    __shared__ float red[4][LOSS_THREADS / WAVE];
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x - b * a.nblk;
    const int64_t base = (int64_t)b * a.M;
    const float* Pb = a.P + base * a.ldp;
    float A = 0.f, E = 0.f, Gs = 0.f, R = 0.f;
#pragma unroll
    for (int it = 0; it < LOSS_ITER; ++it) {
        const int64_t g = (base >> 2) + (int64_t)blk * LOSS_GROUPS + it * LOSS_THREADS + threadIdx.x;
        const int64_t q0 = (g << 2) - base;
        if (q0 >= a.M) continue;
        LossGroup v;
        loss_load_group<(MODE > 0)>(a, base, q0, v);
        const int qc = q0 < 0 ? 0 : (int)q0;                                  // M fits 31 bits (loss_params)
        int i = qc / a.n, j = qc - i * a.n + ((int)q0 - qc);                  // j < 0 only where ok[e] is false
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (v.ok[e]) {
                const float d = v.p[e] - v.t[e];
                A = fmaf(v.t[e], v.t[e], A);
                E = fmaf(d, d, E);
                if (MODE > 0) Gs = fmaf(v.k[e], fmaf(v.gx[e], v.gx[e], v.gy[e] * v.gy[e]), Gs);
                if (MODE > 1 && loss_interior(a, i, j)) {
                    const float rx = v.k[e] * (v.gx[e] - loss_dx(a, Pb, i, j)), ry = v.k[e] * (v.gy[e] - loss_dy(a, Pb, i, j));
                    R = fmaf(rx, rx, R);
                    R = fmaf(ry, ry, R);
                }
            }
            if (++j == a.n) { j = 0; ++i; }
        }
    }
    A = wave_sum(A); E = wave_sum(E); Gs = wave_sum(Gs); R = wave_sum(R);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[0][w] = A; red[1][w] = E; red[2][w] = Gs; red[3][w] = R;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const float* r = red[threadIdx.x];
        partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

struct LossFinalP {
    int nblk; double M, m2x2;           // pixels per sample; 2 m^2 elements of the interior differences
    float h, beta, gamma, eps;
    int has_g;
    float* loss; float* reg; float* L2; float* H1;       // reg may be NULL
};

// one wave per sample: lane l sums the partials l, l + 64, ... in that order, lane 0 then sums the 64 lanes in lane order
__global__ __launch_bounds__(WAVE) void h1loss2d_final_kernel(const float* __restrict__ partial, const LossFinalP a) {
    __shared__ double red[4][WAVE];
    const int b = blockIdx.x;
    const float* pb = partial + (int64_t)b * a.nblk * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < a.nblk; i += WAVE) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pb + (int64_t)i * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += (double)v[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int l = 0; l < WAVE; ++l) {
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] += red[c][l];
        }
        const double l2 = t[0] / a.M + (double)a.eps;
        const double h1 = a.has_g ? t[2] / a.M + (double)a.eps : 1.0;
        a.L2[b] = (float)l2;
        a.H1[b] = (float)h1;
        a.loss[b] = (float)((double)a.beta * (t[1] / a.M) / l2);
        if (a.reg) a.reg[b] = (float)((double)a.gamma * (double)a.h * (t[3] / a.m2x2) / h1);
    }
}

struct LossBwdP {
    LossP f;
    const float* L2; const float* H1; const float* gl; const float* gr;      // gl / gr may be NULL (no gradient from there)
    float c1, c2;                       // beta 2 / M  *  gamma h 2 / (2 m^2) / (d h): the parts that need no device value
    float* dP;
};

// r_x / r_y = K^2 (D P - G) at the stencil centre (ci, cj); zero where the stencil leaves the grid
__device__ __forceinline__ float loss_rx(const LossP& a, const float* __restrict__ Pb, int64_t base, int ci, int cj) {
    if (!loss_interior(a, ci, cj)) return 0.f;
    const int64_t x = base + (int64_t)ci * a.n + cj;
    const float k = a.K ? a.K[x] : 1.f;
    return k * k * (loss_dx(a, Pb, ci, cj) - a.G[2 * x]);
}
__device__ __forceinline__ float loss_ry(const LossP& a, const float* __restrict__ Pb, int64_t base, int ci, int cj) {
    if (!loss_interior(a, ci, cj)) return 0.f;
    const int64_t x = base + (int64_t)ci * a.n + cj;
    const float k = a.K ? a.K[x] : 1.f;
    return k * k * (loss_dy(a, Pb, ci, cj) - a.G[2 * x + 1]);
}

__global__ __launch_bounds__(LOSS_THREADS) void h1loss2d_bwd_kernel(const LossBwdP a) {
    const LossP& f = a.f;
    const int b = blockIdx.x / f.nblk, blk = blockIdx.x - b * f.nblk;
    const int64_t base = (int64_t)b * f.M;
    const float* Pb = f.P + base * f.ldp;
    const float c1 = a.gl ? a.gl[b] * a.c1 / a.L2[b] : 0.f;
    const float c2 = (a.gr && f.G) ? a.gr[b] * a.c2 / a.H1[b] : 0.f;
    const bool reg = a.gr && f.G;
#pragma unroll
    for (int it = 0; it < LOSS_ITER; ++it) {
        const int64_t g = (base >> 2) + (int64_t)blk * LOSS_GROUPS + it * LOSS_THREADS + threadIdx.x;
        const int64_t q0 = (g << 2) - base;
        if (q0 >= f.M) continue;
        LossGroup v;
        loss_load_group<false>(f, base, q0, v);
        const int qc = q0 < 0 ? 0 : (int)q0;
        int i = qc / f.n, j = qc - i * f.n + ((int)q0 - qc);
        float out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d = 0.f;
            if (v.ok[e]) {
                d = c1 * (v.p[e] - v.t[e]);
                if (reg) {
                    const float r = (loss_rx(f, Pb, base, i - f.s, j) - loss_rx(f, Pb, base, i + f.s, j)) +
                                    (loss_ry(f, Pb, base, i, j - f.s) - loss_ry(f, Pb, base, i, j + f.s));
                    d = fmaf(c2, r, d);
                }
            }
            out[e] = d;
            if (++j == f.n) { j = 0; ++i; }
        }
        const int64_t x = base + q0;
        if (f.vec && q0 >= 0 && q0 + 4 <= f.M) {
            *reinterpret_cast<f32x4*>(a.dP + x) = f32x4{out[0], out[1], out[2], out[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v.ok[e]) a.dP[x + e] = out[e];
        }
    }
}

// the checks and the derived values the three entry points share; 0 or a GT_E* code
static int loss_params(const float* P, int64_t ldp, const float* T, const float* G, const float* K, int32_t N, int32_t n,
                       int32_t dilation, float h, const float* also, LossP* a) {
    if (!P || !T || N <= 0 || n <= 0 || ldp < 1 || dilation < 2 || (dilation & 1) || n <= dilation || !(h > 0.f))
        return GT_EINVAL;
    if (K && !G) return GT_EINVAL;
    if (misaligned<4>(P, T, G, K, also)) return GT_EALIGN;
    const int64_t M = (int64_t)n * n;
    if (M > 0x7fffffffll || (int64_t)N * loss_blocks(M) > 0x7fffffffll) return GT_ENOTSUP;
    *a = LossP{P, ldp, T, G, K, n, dilation / 2, M, loss_blocks(M), 1.f / ((float)dilation * h),
               !misaligned16(T, G, K, also), ldp == 1 && !misaligned16(P)};
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" int64_t gt_h1loss2d_ws_bytes(int32_t N, int32_t n) {
    if (N <= 0 || n <= 0) return 0;
    return (int64_t)N * loss_blocks((int64_t)n * n) * 4 * (int64_t)sizeof(float);
}

extern "C" int gt_h1loss2d_fwd(const float* P, int64_t ldp, const float* T, const float* G, const float* K, int32_t N,
                               int32_t n, int32_t dilation, float h, int32_t want_reg, void* ws, int64_t ws_bytes,
                               void* stream) {
    LossP a;
    if (const int rc = loss_params(P, ldp, T, G, K, N, n, dilation, h, nullptr, &a)) return rc;
    if (want_reg && !G) return GT_EINVAL;
    if (!ws || ws_bytes < gt_h1loss2d_ws_bytes(N, n)) return GT_EWS;
    if (misaligned16(ws)) return GT_EALIGN;
    float* partial = reinterpret_cast<float*>(ws);
    const dim3 grid((unsigned)(N * a.nblk)), block(LOSS_THREADS);
    if (!G) hipLaunchKernelGGL(h1loss2d_partial_kernel<0>, grid, block, 0, (hipStream_t)stream, a, partial);
    else if (!want_reg) hipLaunchKernelGGL(h1loss2d_partial_kernel<1>, grid, block, 0, (hipStream_t)stream, a, partial);
    else hipLaunchKernelGGL(h1loss2d_partial_kernel<2>, grid, block, 0, (hipStream_t)stream, a, partial);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_h1loss2d_final(int32_t N, int32_t n, int32_t dilation, float h, float beta, float gamma, float eps,
                                 int32_t has_g, float* loss, float* reg, float* L2, float* H1, const void* ws,
                                 int64_t ws_bytes, void* stream) {
    if (!loss || !L2 || !H1 || N <= 0 || n <= 0 || dilation < 2 || (dilation & 1) || n <= dilation) return GT_EINVAL;
    if (reg && !has_g) return GT_EINVAL;
    if (!ws || ws_bytes < gt_h1loss2d_ws_bytes(N, n)) return GT_EWS;
    if (misaligned16(ws) || misaligned<4>(loss, reg, L2, H1)) return GT_EALIGN;
    const int64_t M = (int64_t)n * n, m = n - dilation;
    const LossFinalP a{loss_blocks(M), (double)M, 2.0 * (double)m * (double)m, h, beta, gamma, eps, has_g, loss, reg, L2, H1};
    hipLaunchKernelGGL(h1loss2d_final_kernel, dim3(N), dim3(WAVE), 0, (hipStream_t)stream,
                       reinterpret_cast<const float*>(ws), a);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_h1loss2d_bwd(const float* P, int64_t ldp, const float* T, const float* G, const float* K, const float* L2,
                               const float* H1, const float* gl, const float* gr, int32_t N, int32_t n, int32_t dilation,
                               float h, float beta, float gamma, float* dP, void* stream) {
    LossBwdP a;
    if (!dP || !L2 || !H1) return GT_EINVAL;
    if (const int rc = loss_params(P, ldp, T, G, K, N, n, dilation, h, dP, &a.f)) return rc;
    if (misaligned<4>(L2, H1, gl, gr)) return GT_EALIGN;
    const double M = (double)a.f.M, m = (double)(n - dilation);
    a.L2 = L2; a.H1 = H1; a.gl = gl; a.gr = gr; a.dP = dP;
    a.c1 = (float)((double)beta * 2.0 / M);
    a.c2 = (float)((double)gamma * (double)h * 2.0 / (2.0 * m * m) / ((double)dilation * (double)h));
    hipLaunchKernelGGL(h1loss2d_bwd_kernel, dim3((unsigned)(N * a.f.nblk)), dim3(LOSS_THREADS), 0, (hipStream_t)stream, a);
    GT_LAUNCH_CHECK();
    return 0;
}
