// Token-axis ("instance") norm of the K / V head tiles: norm_type='instance' of the Galerkin family (reference
// layers.py:842-854, 917-923, 949-951 -- nn.InstanceNorm1d(d_k, affine=True) on the transposed heads).  For every
// (sample b, head i, value channel c) over the n tokens:
//     y[t] = (x[t] - mean_t x) * rstd * gamma[i][c] + beta[i][c],      rstd = 1 / sqrt(biased var_t x + eps)
// on the head-tile layout [B*n][h][DP], DP = round4(dk + p), fp32.  The p coordinate columns pass through unchanged and the
// pad columns dk + p .. DP-1 are written as exact zeros (forward and backward).
//
// One batch item is a dense [n][C4] array of float4 (C4 = h * DP / 4) and the passes are the column-statistics passes of
// gt_colpass.h, which states the block shape, the Welford / pivot / Chan arithmetic and the merge orders: a block owns `chunk`
// consecutive tokens of one sample and CG <= 256 adjacent column groups, its threads form RL = 256 / CG row lanes.
//     forward : partial   per (sample, chunk, column): (mean, M2) relative to the column's first token of the sample
//               finalize  per (sample, column): the chunks merged in chunk order, pivot added back once -> stats
//               apply     y = (x - mean) * (rstd gamma) + beta
//     backward: partial   s1 = sum dY, s2 = sum dY xh per (sample, chunk, column), xh recomputed from x and stats
//               finalize  chunks summed in order per (sample, column)
//               apply     dX = rstd gamma (dY - s1/n - xh s2/n)
//               params    dgamma = sum_b s2, dbeta = sum_b s1, samples in order
// In place is allowed (Y == X, dX == dY): the statistics are complete before the applying launch starts, and there every
// thread reads the elements it owns before it writes them.
#include <math.h>

#include "gt_colpass.h"

namespace gt {
namespace {

struct TnGeom : ColGeom {
    int chunk, nchunks;
};
static inline TnGeom tn_geom(int B, int n, int h, int DP) {
    TnGeom g{col_geom(h * DP / 4), 0, 0};
    g.chunk = col_chunk(n, (int64_t)B * g.ncb);      // small batches: shorter chunks
    g.nchunks = (n + g.chunk - 1) / g.chunk;
    return g;
}

struct TnP {
    const float* X;          // raw tiles
    const float* G;          // bwd: dY
    float* Y;                // fwd: Y ; bwd: dX
    const float* gamma;      // [h][dk]
    const float* beta;       // [h][dk] (fwd)
    float* stats;            // [B][h][dk][2] (mean, rstd): written by the forward's finalize, read by everything after it
    f32x4* part;             // [B][nchunks][2][C4]: fwd (mean, M2), bwd (s1, s2)
    f32x4* sums;             // bwd: [B][2][C4] (s1, s2) over all tokens
    float* dgamma;           // [h][dk] or NULL
    float* dbeta;
    int n, h, dk, pd, DP, C4, CG, RL, chunk, nchunks;
    float eps;
};

// value channel of component j of column group col4 (or -1: coordinate / pad column), and the head
__device__ __forceinline__ void tn_columns(const TnP& p, int col4, int& head, int ch[4], bool coord[4]) {
    const int c = col4 * 4;      // DP % 4 == 0: a float4 never straddles two heads
    head = c / p.DP;
    const int c0 = c - head * p.DP;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = c0 + j - p.pd;
        coord[j] = c0 + j < p.pd;
        ch[j] = (v >= 0 && v < p.dk) ? v : -1;
    }
}

__device__ __forceinline__ void tn_load_stats(const TnP& p, int b, int head, const int ch[4], f32x4& mean, f32x4& rstd) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mean[j] = 0.f;
        rstd[j] = 0.f;
        if (ch[j] >= 0) {
            const f32x2 s = *reinterpret_cast<const f32x2*>(p.stats + (((int64_t)b * p.h + head) * p.dk + ch[j]) * 2);
            mean[j] = s[0];
            rstd[j] = s[1];
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void token_norm_partial_kernel(TnP p) {
    __shared__ f32x4 sa[COL_THREADS], sb[COL_THREADS];
    const ColLane L = col_lane(p.CG, p.RL, p.C4, blockIdx.z);
    const int b = blockIdx.y, chunk = blockIdx.x;
    const ColRows<int> R = col_rows(chunk, p.chunk, p.n);
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};      // fwd: (mean, M2) ; bwd: (s1, s2)
    if (L.active) {
        const int64_t base = (int64_t)b * p.n * p.C4 + L.col4;      // the sample's first token: the pivot row
        const f32x4* X4 = reinterpret_cast<const f32x4*>(p.X) + base;
        if (BWD) {
            int head, ch[4];
            bool coord[4];
            f32x4 mean, rstd;
            tn_columns(p, L.col4, head, ch, coord);
            tn_load_stats(p, b, head, ch, mean, rstd);
            col_gsum_rows(X4, reinterpret_cast<const f32x4*>(p.G) + base, p.C4, R.r0 + L.rl, R.r1, p.RL, mean, rstd, a, m2);
        } else {
            col_welford_rows(X4, p.C4, R.r0 + L.rl, R.r1, p.RL, a, m2);
        }
    }
    col_merge_lanes<BWD>(sa, sb, L, p.CG, p.RL, R.r1 - R.r0, a, m2);
    if (L.active && L.rl == 0) {
        f32x4* o = p.part + ((int64_t)b * p.nchunks + chunk) * 2 * p.C4 + L.col4;
        o[0] = a;
        o[p.C4] = m2;
    }
}

// one thread per (sample, column group): the chunk partials in chunk order
template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void token_norm_finalize_kernel(TnP p, int B) {
    const int64_t idx = (int64_t)blockIdx.x * COL_THREADS + threadIdx.x;
    if (idx >= (int64_t)B * p.C4) return;
    const int b = (int)(idx / p.C4), col4 = (int)(idx - (int64_t)b * p.C4);
    const f32x4* o = p.part + (int64_t)b * p.nchunks * 2 * p.C4 + col4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    col_merge_chunks<BWD>(o, p.C4, 0, p.nchunks, p.chunk, p.n, a, m2);
    if (BWD) {
        p.sums[((int64_t)b * 2 + 0) * p.C4 + col4] = a;
        p.sums[((int64_t)b * 2 + 1) * p.C4 + col4] = m2;
    } else {
        int head, ch[4];
        bool coord[4];
        tn_columns(p, col4, head, ch, coord);
        const f32x4 piv = reinterpret_cast<const f32x4*>(p.X)[(int64_t)b * p.n * p.C4 + col4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ch[j] >= 0) {
                f32x2 s;
                s[0] = piv[j] + a[j];
                s[1] = 1.f / sqrtf(m2[j] / (float)p.n + p.eps);      // biased variance, as nn.InstanceNorm1d
                *reinterpret_cast<f32x2*>(p.stats + (((int64_t)b * p.h + head) * p.dk + ch[j]) * 2) = s;
            }
    }
}

template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void token_norm_apply_kernel(TnP p) {
    const ColLane L = col_lane(p.CG, p.RL, p.C4, blockIdx.z);
    const int b = blockIdx.y, col4 = L.col4;
    if (!L.active) return;
    int head, ch[4];
    bool coord[4];
    f32x4 mean, rstd, sc, sh = {0.f, 0.f, 0.f, 0.f};      // sc = rstd gamma ; sh = beta
    tn_columns(p, col4, head, ch, coord);
    tn_load_stats(p, b, head, ch, mean, rstd);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sc[j] = ch[j] >= 0 ? rstd[j] * p.gamma[head * p.dk + ch[j]] : 0.f;
        if (!BWD && ch[j] >= 0) sh[j] = p.beta[head * p.dk + ch[j]];
    }
    f32x4 m1 = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    if (BWD) {
        const float inv = 1.f / (float)p.n;
        m1 = p.sums[((int64_t)b * 2 + 0) * p.C4 + col4] * inv;
        m2 = p.sums[((int64_t)b * 2 + 1) * p.C4 + col4] * inv;
    }
    const ColRows<int> R = col_rows((int)blockIdx.x, p.chunk, p.n);
    const int64_t base = (int64_t)b * p.n * p.C4 + col4;
    const f32x4* X4 = reinterpret_cast<const f32x4*>(p.X) + base;
    const f32x4* G4 = reinterpret_cast<const f32x4*>(p.G) + base;
    f32x4* Y4 = reinterpret_cast<f32x4*>(p.Y) + base;
#pragma unroll 4
    for (int r = R.r0 + L.rl; r < R.r1; r += p.RL) {
        const f32x4 x = X4[(int64_t)r * p.C4];
        f32x4 y;
        if (BWD) {
            const f32x4 g = G4[(int64_t)r * p.C4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                y[j] = ch[j] >= 0 ? sc[j] * (g[j] - m1[j] - (x[j] - mean[j]) * rstd[j] * m2[j]) : (coord[j] ? g[j] : 0.f);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = ch[j] >= 0 ? (x[j] - mean[j]) * sc[j] + sh[j] : (coord[j] ? x[j] : 0.f);
        }
        Y4[(int64_t)r * p.C4] = y;
    }
}

// dgamma = sum_b s2, dbeta = sum_b s1: one thread per column group, samples in order
__global__ __launch_bounds__(COL_THREADS) void token_norm_params_kernel(TnP p, int B) {
    const int col4 = blockIdx.x * COL_THREADS + threadIdx.x;
    if (col4 >= p.C4) return;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
        s1 += p.sums[((int64_t)b * 2 + 0) * p.C4 + col4];
        s2 += p.sums[((int64_t)b * 2 + 1) * p.C4 + col4];
    }
    int head, ch[4];
    bool coord[4];
    tn_columns(p, col4, head, ch, coord);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (ch[j] >= 0) {
            if (p.dgamma) p.dgamma[head * p.dk + ch[j]] = s2[j];
            if (p.dbeta) p.dbeta[head * p.dk + ch[j]] = s1[j];
        }
}

template <bool BWD>
int token_norm_run(const float* X, const float* G, const float* gamma, const float* beta, float eps, float* Y, float* stats,
                   float* dgamma, float* dbeta, int B, int n, int h, int dk, int pd, void* ws, int64_t ws_bytes,
                   void* stream) {
    if (!X || !Y || !gamma || !stats || (BWD ? !G : !beta) || B <= 0 || n <= 0 || h <= 0) return GT_EINVAL;
    if (!BWD && !(eps >= 0.f)) return GT_EINVAL;
    if (!head_tile_shape_ok(dk, pd) || B > 65535) return GT_ENOTSUP;
    if (misaligned16(X, G, Y, ws) || (reinterpret_cast<uintptr_t>(stats) & 7)) return GT_EALIGN;
    if (!ws || ws_bytes < gt_token_norm_ws_bytes(B, n, h, dk, pd)) return GT_EWS;
    const int DP = round4(dk + pd);
    const TnGeom g = tn_geom(B, n, h, DP);
    if (g.ncb > 65535) return GT_ENOTSUP;
    f32x4* part = reinterpret_cast<f32x4*>(ws);
    TnP p{X, G, Y, gamma, beta, stats, part, part + (int64_t)B * g.nchunks * 2 * g.C4, dgamma, dbeta,
          n, h, dk, pd, DP, g.C4, g.CG, g.RL, g.chunk, g.nchunks, eps};
    const dim3 grid((unsigned)g.nchunks, (unsigned)B, (unsigned)g.ncb);
    const dim3 flat((unsigned)(((int64_t)B * g.C4 + COL_THREADS - 1) / COL_THREADS));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(token_norm_partial_kernel<BWD>, grid, dim3(COL_THREADS), 0, st, p);
    GT_LAUNCH_CHECK();
    hipLaunchKernelGGL(token_norm_finalize_kernel<BWD>, flat, dim3(COL_THREADS), 0, st, p, B);
    GT_LAUNCH_CHECK();
    hipLaunchKernelGGL(token_norm_apply_kernel<BWD>, grid, dim3(COL_THREADS), 0, st, p);
    GT_LAUNCH_CHECK();
    if (BWD && (dgamma || dbeta)) {
        hipLaunchKernelGGL(token_norm_params_kernel, dim3((unsigned)((g.C4 + COL_THREADS - 1) / COL_THREADS)), dim3(COL_THREADS),
                           0, st, p, B);
        GT_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace
}  // namespace gt

using namespace gt;

extern "C" int64_t gt_token_norm_ws_bytes(int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p) {
    if (B <= 0 || n <= 0 || h <= 0 || !head_tile_shape_ok(dk, p)) return 0;
    const TnGeom g = tn_geom(B, n, h, round4(dk + p));
    return ((int64_t)B * g.nchunks + B) * 2 * g.C4 * (int64_t)sizeof(f32x4);
}

extern "C" int gt_token_norm_fwd(const float* X, const float* gamma, const float* beta, float eps, float* Y, float* stats,
                                 int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p, void* ws, int64_t ws_bytes,
                                 void* stream) {
    if (n == 1) return GT_EINVAL;      // one token has no variance (nn.InstanceNorm1d refuses it too)
    return token_norm_run<false>(X, nullptr, gamma, beta, eps, Y, stats, nullptr, nullptr, B, n, h, dk, p, ws, ws_bytes,
                                 stream);
}

extern "C" int gt_token_norm_bwd(const float* X, const float* dY, const float* gamma, const float* stats, float* dX,
                                 float* dgamma, float* dbeta, int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p,
                                 void* ws, int64_t ws_bytes, void* stream) {
    return token_norm_run<true>(X, dY, gamma, nullptr, 0.f, dX, const_cast<float*>(stats), dgamma, dbeta, B, n, h, dk, p, ws,
                                ws_bytes, stream);
}
