// The training objectives of the examples, per sample, forward and backward: the relative L2 error plus the gamma h
// H1-seminorm regulariser on dilated central differences, in 2-D (reference: libs/ft.py:983-1105, WeightedL2Loss2d) and in
// 1-D (libs/ft.py:898-980, WeightedL2Loss).  HBM-bound in 2-D, launch-bound in 1-D: the forward reads P, T, G (K) once and
// writes four floats per block; the backward reads them again and writes dP once.  The stencil's neighbours of P (and, in
// the backward, of K and G) come through the cache.
//   forward : per-block partial sums (A, E, Gs, R) in ws, block order fixed          (h1loss{2d,1d}_partial_kernel)
//   final   : the partials of a sample summed in block order, in double; the four per-sample scalars (h1loss{2d,1d}_final_kernel)
//   backward: a gather -- every element of dP recomputes the at most four (1-D: two) residuals it feeds; no atomics
//                                                                                     (h1loss{2d,1d}_bwd_kernel)
// The flat element range of a sample is walked in groups of four elements whose GLOBAL index is a multiple of four, so that
// a group inside the sample is one 16-byte access of T, K, dP (two of the 2-D G) whatever the sample's length is; the at most
// two groups that straddle a sample boundary, and every tensor off a 16-byte boundary, take scalar accesses under a mask.
// The walk (loss_q0, loss_mask, loss_load4, loss_write4), the block's reduction (loss_block_store) and the merge of a
// sample's partials (loss_merge) are stated once for both dimensions.
#include <algorithm>

#include "gt_common.h"

namespace gt {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_ITER = 2;                                // groups of four pixels per thread
constexpr int LOSS_GROUPS = LOSS_THREADS * LOSS_ITER;       // per block

// groups a sample can touch: M / 4 whole ones plus one straddling group at either end
inline int loss_blocks(int64_t M) { return (int)(((M >> 2) + 2 + LOSS_GROUPS - 1) / LOSS_GROUPS); }

// first element, relative to the sample's first one at flat index `base`, of the group that thread threadIdx.x of the
// sample's block `blk` walks in its iteration `it`: -3 .. ; the caller drops groups that start past the sample's end
__device__ __forceinline__ int64_t loss_q0(int64_t base, int blk, int it) {
    const int64_t g = (base >> 2) + (int64_t)blk * LOSS_GROUPS + it * LOSS_THREADS + threadIdx.x;
    return (g << 2) - base;
}
// ok[e]: element q0 + e lies inside the sample of M elements; true if all four do
__device__ __forceinline__ bool loss_mask(int64_t q0, int64_t M, bool ok[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) ok[e] = q0 + e >= 0 && q0 + e < M;
    return q0 >= 0 && q0 + 4 <= M;
}
// the four values src[(x + e) * pitch]: one 16-byte access if `vec` (pitch 1, x a multiple of four, src 16-byte aligned and
// all four inside the sample), else scalar accesses under the mask, 0 where it is false
__device__ __forceinline__ void loss_load4(const float* __restrict__ src, int64_t x, int64_t pitch, bool vec,
                                           const bool ok[4], float out[4]) {
    if (vec) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = v[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = ok[e] ? src[(x + e) * pitch] : 0.f;
    }
}
__device__ __forceinline__ void loss_write4(float* __restrict__ dst, int64_t x, bool vec, const bool ok[4],
                                            const float v[4]) {
    if (vec) {
        *reinterpret_cast<f32x4*>(dst + x) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ok[e]) dst[x + e] = v[e];
    }
}
// the block's sums of the four per-thread values, waves added pairwise, into partial[blockIdx.x * 4 + {0, 1, 2, 3}]
__device__ __forceinline__ void loss_block_store(float A, float E, float Gs, float R, float* __restrict__ partial) {
    __shared__ float red[4][LOSS_THREADS / WAVE];
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
// one wave: lane l sums the nblk partials l, l + 64, ... at pb in that order, lane 0 then sums the 64 lanes in lane order
// into t[0 .. 3]; true on lane 0, which alone holds the sums
__device__ __forceinline__ bool loss_merge(const float* __restrict__ pb, int nblk, double t[4]) {
    __shared__ double red[4][WAVE];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += WAVE) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pb + (int64_t)i * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += (double)v[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = 0.0;
#pragma unroll 1
    for (int l = 0; l < WAVE; ++l) {
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] += red[c][l];
    }
    return true;
}

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
    const bool full = loss_mask(q0, a.M, v.ok);
    const int64_t x = base + q0;
    if (full && a.vec) {                                    // one branch for T, G, K: G is two accesses of interleaved pairs
        loss_load4(a.T, x, 1, true, v.ok, v.t);
        if (HASG) {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.G + 2 * x), g1 = *reinterpret_cast<const f32x4*>(a.G + 2 * x + 4);
            v.gx[0] = g0[0]; v.gy[0] = g0[1]; v.gx[1] = g0[2]; v.gy[1] = g0[3];
            v.gx[2] = g1[0]; v.gy[2] = g1[1]; v.gx[3] = g1[2]; v.gy[3] = g1[3];
            if (a.K) loss_load4(a.K, x, 1, true, v.ok, v.k);
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
    loss_load4(a.P, x, a.ldp, full && a.pvec, v.ok, v.p);
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
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x - b * a.nblk;
    const int64_t base = (int64_t)b * a.M;
    const float* Pb = a.P + base * a.ldp;
    float A = 0.f, E = 0.f, Gs = 0.f, R = 0.f;
#pragma unroll
    for (int it = 0; it < LOSS_ITER; ++it) {
        const int64_t q0 = loss_q0(base, blk, it);
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
    loss_block_store(A, E, Gs, R, partial);
}

struct LossFinalP {
    int nblk; double M, m2x2;           // pixels per sample; 2 m^2 elements of the interior differences
    float h, beta, gamma, eps;
    int has_g;
    float* loss; float* reg; float* L2; float* H1;       // reg may be NULL
};

// one wave per sample (loss_merge)
__global__ __launch_bounds__(WAVE) void h1loss2d_final_kernel(const float* __restrict__ partial, const LossFinalP a) {
    const int b = blockIdx.x;
    double t[4];
    if (loss_merge(partial + (int64_t)b * a.nblk * 4, a.nblk, t)) {
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
        const int64_t q0 = loss_q0(base, blk, it);
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
        loss_write4(a.dP, base + q0, f.vec && q0 >= 0 && q0 + 4 <= f.M, v.ok, out);
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

// ------------------------------------------------------------------------------------------------------------- 1-D
// A sample is a row of L elements; the same walk, reduction and merge.  No K, one component of G, no eps in the norms, and
// the sums are scaled by h instead of divided by the element count, as the reference has it.
struct Loss1P {
    const float* P; int64_t ldp;        // prediction, element pitch in floats
    const float* T; const float* G;
    int L, s, nblk;                     // row length, half dilation, blocks per sample
    float inv_dh;                       // 1 / (d h)
    bool vec, pvec;                     // T, G (and dP) / P may be accessed 16 bytes at a time
};

// D P at the centre c of an interior stencil (s <= c < L - s); Pb is the sample's first element
__device__ __forceinline__ float loss1_diff(const Loss1P& a, const float* __restrict__ Pb, int64_t c) {
    return (Pb[(c + a.s) * a.ldp] - Pb[(c - a.s) * a.ldp]) * a.inv_dh;
}

// MODE as in 2-D; partial[(b * nblk + blk) * 4 + {0, 1, 2, 3}] = this block's share of (sum T^2, sum (P - T)^2, sum G^2, R)
template <int MODE>
__global__ __launch_bounds__(LOSS_THREADS) void h1loss1d_partial_kernel(const Loss1P a, float* __restrict__ partial) {
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x - b * a.nblk;
    const int64_t base = (int64_t)b * a.L;
    const float* Pb = a.P + base * a.ldp;
    float A = 0.f, E = 0.f, Gs = 0.f, R = 0.f;
#pragma unroll
    for (int it = 0; it < LOSS_ITER; ++it) {
        const int64_t q0 = loss_q0(base, blk, it);
        if (q0 >= a.L) continue;
        bool ok[4];
        float p[4], t[4], g[4];
        const bool full = loss_mask(q0, a.L, ok);
        loss_load4(a.T, base + q0, 1, full && a.vec, ok, t);
        if (MODE > 0) loss_load4(a.G, base + q0, 1, full && a.vec, ok, g);
        loss_load4(a.P, base + q0, a.ldp, full && a.pvec, ok, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!ok[e]) continue;
            const int64_t c = q0 + e;
            const float d = p[e] - t[e];
            A = fmaf(t[e], t[e], A);
            E = fmaf(d, d, E);
            if (MODE > 0) Gs = fmaf(g[e], g[e], Gs);
            if (MODE > 1 && c >= a.s && c < a.L - a.s) {
                const float r = g[e] - loss1_diff(a, Pb, c);
                R = fmaf(r, r, R);
            }
        }
    }
    loss_block_store(A, E, Gs, R, partial);
}

struct Loss1FinalP {
    int nblk;
    float h, beta, gamma_h;             // gamma_h: the regulariser's weight, already multiplied by h
    int has_g;
    float* loss; float* reg; float* L2; float* H1;       // reg may be NULL
};

// one wave per sample (loss_merge)
__global__ __launch_bounds__(WAVE) void h1loss1d_final_kernel(const float* __restrict__ partial, const Loss1FinalP a) {
    const int b = blockIdx.x;
    double t[4];
    if (loss_merge(partial + (int64_t)b * a.nblk * 4, a.nblk, t)) {
        const double h = (double)a.h;
        const double l2 = h * t[0];
        const double h1 = a.has_g ? h * t[2] : 1.0;
        a.L2[b] = (float)l2;
        a.H1[b] = (float)h1;
        a.loss[b] = (float)((double)a.beta * (h * t[1]) / l2);
        if (a.reg) a.reg[b] = (float)((double)a.gamma_h * (h * t[3]) / h1);
    }
}

struct Loss1BwdP {
    Loss1P f;
    const float* L2; const float* H1; const float* gl; const float* gr;      // gl / gr may be NULL (no gradient from there)
    float c1, c2;                       // beta h 2  *  gamma_h h 2 / (d h): the parts that need no device value
    float* dP;
};

// r = D P - G at the stencil centre c; zero where the stencil leaves the row
__device__ __forceinline__ float loss1_r(const Loss1P& a, const float* __restrict__ Pb, int64_t base, int64_t c) {
    if (c < a.s || c >= a.L - a.s) return 0.f;
    return loss1_diff(a, Pb, c) - a.G[base + c];
}

__global__ __launch_bounds__(LOSS_THREADS) void h1loss1d_bwd_kernel(const Loss1BwdP a) {
    const Loss1P& f = a.f;
    const int b = blockIdx.x / f.nblk, blk = blockIdx.x - b * f.nblk;
    const int64_t base = (int64_t)b * f.L;
    const float* Pb = f.P + base * f.ldp;
    const bool reg = a.gr && f.G;
    const float c1 = a.gl ? a.gl[b] * a.c1 / a.L2[b] : 0.f;
    const float c2 = reg ? a.gr[b] * a.c2 / a.H1[b] : 0.f;
#pragma unroll
    for (int it = 0; it < LOSS_ITER; ++it) {
        const int64_t q0 = loss_q0(base, blk, it);
        if (q0 >= f.L) continue;
        bool ok[4];
        float p[4], t[4], out[4];
        const bool full = loss_mask(q0, f.L, ok);
        loss_load4(f.T, base + q0, 1, full && f.vec, ok, t);
        loss_load4(f.P, base + q0, f.ldp, full && f.pvec, ok, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d = 0.f;
            if (ok[e]) {
                const int64_t i = q0 + e;
                d = c1 * (p[e] - t[e]);
                if (reg) d = fmaf(c2, loss1_r(f, Pb, base, i - f.s) - loss1_r(f, Pb, base, i + f.s), d);
            }
            out[e] = d;
        }
        loss_write4(a.dP, base + q0, full && f.vec, ok, out);
    }
}

static int loss1_params(const float* P, int64_t ldp, const float* T, const float* G, int32_t N, int32_t L, int32_t dilation,
                        float h, const float* also, Loss1P* a) {
    if (!P || !T || N <= 0 || L <= 0 || ldp < 1 || dilation < 2 || (dilation & 1) || L <= dilation || !(h > 0.f))
        return GT_EINVAL;
    if (misaligned<4>(P, T, G, also)) return GT_EALIGN;
    if ((int64_t)N * loss_blocks(L) > 0x7fffffffll) return GT_ENOTSUP;
    *a = Loss1P{P, ldp, T, G, L, dilation / 2, loss_blocks(L), 1.f / ((float)dilation * h), !misaligned16(T, G, also),
                ldp == 1 && !misaligned16(P)};
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

extern "C" int64_t gt_h1loss1d_ws_bytes(int32_t N, int32_t L) {
    if (N <= 0 || L <= 0) return 0;
    return (int64_t)N * loss_blocks(L) * 4 * (int64_t)sizeof(float);
}

extern "C" int gt_h1loss1d_fwd(const float* P, int64_t ldp, const float* T, const float* G, int32_t N, int32_t L,
                               int32_t dilation, float h, int32_t want_reg, void* ws, int64_t ws_bytes, void* stream) {
    Loss1P a;
    if (const int rc = loss1_params(P, ldp, T, G, N, L, dilation, h, nullptr, &a)) return rc;
    if (want_reg && !G) return GT_EINVAL;
    if (!ws || ws_bytes < gt_h1loss1d_ws_bytes(N, L)) return GT_EWS;
    if (misaligned16(ws)) return GT_EALIGN;
    float* partial = reinterpret_cast<float*>(ws);
    const dim3 grid((unsigned)(N * a.nblk)), block(LOSS_THREADS);
    if (!G) hipLaunchKernelGGL(h1loss1d_partial_kernel<0>, grid, block, 0, (hipStream_t)stream, a, partial);
    else if (!want_reg) hipLaunchKernelGGL(h1loss1d_partial_kernel<1>, grid, block, 0, (hipStream_t)stream, a, partial);
    else hipLaunchKernelGGL(h1loss1d_partial_kernel<2>, grid, block, 0, (hipStream_t)stream, a, partial);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_h1loss1d_final(int32_t N, int32_t L, int32_t dilation, float h, float beta, float gamma_h, int32_t has_g,
                                 float* loss, float* reg, float* L2, float* H1, const void* ws, int64_t ws_bytes,
                                 void* stream) {
    if (!loss || !L2 || !H1 || N <= 0 || L <= 0 || dilation < 2 || (dilation & 1) || L <= dilation || !(h > 0.f))
        return GT_EINVAL;
    if (reg && !has_g) return GT_EINVAL;
    if ((int64_t)N * loss_blocks(L) > 0x7fffffffll) return GT_ENOTSUP;
    if (!ws || ws_bytes < gt_h1loss1d_ws_bytes(N, L)) return GT_EWS;
    if (misaligned16(ws) || misaligned<4>(loss, reg, L2, H1)) return GT_EALIGN;
    const Loss1FinalP a{loss_blocks(L), h, beta, gamma_h, has_g, loss, reg, L2, H1};
    hipLaunchKernelGGL(h1loss1d_final_kernel, dim3(N), dim3(WAVE), 0, (hipStream_t)stream,
                       reinterpret_cast<const float*>(ws), a);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_h1loss1d_bwd(const float* P, int64_t ldp, const float* T, const float* G, const float* L2, const float* H1,
                               const float* gl, const float* gr, int32_t N, int32_t L, int32_t dilation, float h, float beta,
                               float gamma_h, float* dP, void* stream) {
    Loss1BwdP a;
    if (!dP || !L2 || !H1) return GT_EINVAL;
    if (const int rc = loss1_params(P, ldp, T, G, N, L, dilation, h, dP, &a.f)) return rc;
    if (misaligned<4>(L2, H1, gl, gr)) return GT_EALIGN;
    a.L2 = L2; a.H1 = H1; a.gl = gl; a.gr = gr; a.dP = dP;
    a.c1 = (float)((double)beta * (double)h * 2.0);
    a.c2 = (float)((double)gamma_h * (double)h * 2.0 / ((double)dilation * (double)h));
    hipLaunchKernelGGL(h1loss1d_bwd_kernel, dim3((unsigned)(N * a.f.nblk)), dim3(LOSS_THREADS), 0, (hipStream_t)stream, a);
    GT_LAUNCH_CHECK();
    return 0;
}
