// BatchNorm1d of the FeedForward hidden activation: batch_norm=True of FeedForward / SimpleTransformerEncoderLayer (reference
// layers.py:979-987 -- nn.BatchNorm1d(dim_feedforward) on the transposed hidden tensor).  One mean and one biased variance
// per hidden channel over all T = B n token rows, i.e. column statistics of the dense [T][f] matrix, fp32:
//     z[t][c] = (x[t][c] - mean[c]) * rstd[c] * gamma[c] + beta[c],      rstd = 1 / sqrt(biased var + eps)
// training: the batch statistics, and running_mean <- (1 - m) running_mean + m mean,
//                                     running_var  <- (1 - m) running_var  + m var T / (T - 1)
// eval    : mean / var are the running buffers, nothing is updated, and the backward has no mean terms.
//
// The matrix is a dense [T][C4] array of float4 (C4 = f / 4) and the passes are the column-statistics passes of gt_colpass.h,
// which states the block shape, the Welford / pivot / Chan arithmetic and the merge orders: a block owns `chunk` consecutive
// rows and CG <= 256 adjacent column groups; its threads form RL = 256 / CG row lanes.
//     forward : partial   per (chunk, column): (mean, M2) relative to row 0 of the column
//               group     per (group of BN_GROUP chunks, column): the chunks merged in chunk order
//               finalize  per column: the groups merged in group order, pivot added back once -> stats, bvar, running buffers
//               apply     z = (x - mean) * (rstd gamma) + beta
//     eval    : stats     from the running buffers, then the same apply
//     backward: partial   s1 = sum dz, s2 = sum dz xh per (chunk, column), xh recomputed from the raw x and stats
//               group / finalize   summed in the same two levels -> dbeta = s1, dgamma = s2
//               apply     d = rstd gamma (dz - s1/T - xh s2/T)  (eval: rstd gamma dz), times the gate of the activation
//                         and dropout in front of the norm, stored once
// The chunk length follows T: short chunks while the blocks would not cover the device, longer ones so that there are never
// more than BN_MAX_CHUNKS of them, hence at most BN_MAX_CHUNKS / BN_GROUP groups for the last, single-thread merge.
// In place is allowed (Z == X, dX == dZ): the statistics are complete before the applying launch starts, and there every
// thread reads the elements it owns before it writes them.
#include <math.h>

#include "gt_colpass.h"

namespace gt {
namespace {

constexpr int BN_MAX_CHUNKS = 4096;      // longer chunks beyond: the merges stay short whatever T is
constexpr int BN_GROUP = 64;             // chunks per group: the first merge level

struct BnGeom : ColGeom {
    int nchunks, ngroups;
    int64_t chunk;
};
static inline BnGeom bn_geom(int64_t T, int f) {
    BnGeom g{col_geom(f / 4), 0, 0, 0};
    g.chunk = col_chunk(T, g.ncb);
    while ((T + g.chunk - 1) / g.chunk > BN_MAX_CHUNKS) g.chunk <<= 1;
    g.nchunks = (int)((T + g.chunk - 1) / g.chunk);
    g.ngroups = (g.nchunks + BN_GROUP - 1) / BN_GROUP;
    return g;
}

struct BnP {
    const float* X;          // raw hidden activation
    const float* G;          // bwd: dz
    const float* A;          // bwd, GT_AUX_DSILU: the saved pre-activation
    float* Y;                // fwd: z ; bwd: d(hid) behind the gate
    const float* gamma;      // [f]
    const float* beta;       // [f] (fwd)
    float* stats;            // [f][2] (mean, rstd)
    float* bvar;             // [f] biased variance (fwd)
    float* rmean;            // [f] running buffers (fwd) or NULL
    float* rvar;
    f32x4* part;             // [nchunks][2][C4]: fwd (mean, M2), bwd (s1, s2)
    f32x4* gpart;            // [ngroups][2][C4]
    f32x4* sums;             // bwd: [2][C4] (s1, s2) over all rows
    float* dgamma;           // [f] or NULL
    float* dbeta;
    int64_t T, chunk;
    int f, C4, CG, RL, nchunks, ngroups;
    float eps, momentum;
    int training, gate;
    float gate_scale;
    DropDev drop;
};

// (mean, rstd) of the four columns of group col4 from stats [f][2]
__device__ __forceinline__ void bn_load_stats(const BnP& p, int col4, f32x4& mean, f32x4& rstd) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p.stats)[2 * col4], b = reinterpret_cast<const f32x4*>(p.stats)[2 * col4 + 1];
    mean = f32x4{a[0], a[2], b[0], b[2]};
    rstd = f32x4{a[1], a[3], b[1], b[3]};
}
__device__ __forceinline__ void bn_store_stats(const BnP& p, int col4, const f32x4 mean, const f32x4 rstd) {
    reinterpret_cast<f32x4*>(p.stats)[2 * col4] = f32x4{mean[0], rstd[0], mean[1], rstd[1]};
    reinterpret_cast<f32x4*>(p.stats)[2 * col4 + 1] = f32x4{mean[2], rstd[2], mean[3], rstd[3]};
}

template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void batchnorm_partial_kernel(BnP p) {
    __shared__ f32x4 sa[COL_THREADS], sb[COL_THREADS];
    const ColLane L = col_lane(p.CG, p.RL, p.C4, blockIdx.y);
    const int chunk = blockIdx.x;
    const ColRows<int64_t> R = col_rows(chunk, p.chunk, p.T);
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};      // fwd: (mean, M2) ; bwd: (s1, s2)
    if (L.active) {
        const f32x4* X4 = reinterpret_cast<const f32x4*>(p.X) + L.col4;      // row 0: the pivot row
        if (BWD) {
            f32x4 mean, rstd;
            bn_load_stats(p, L.col4, mean, rstd);
            col_gsum_rows(X4, reinterpret_cast<const f32x4*>(p.G) + L.col4, p.C4, R.r0 + L.rl, R.r1, p.RL, mean, rstd, a, m2);
        } else {
            col_welford_rows(X4, p.C4, R.r0 + L.rl, R.r1, p.RL, a, m2);
        }
    }
    col_merge_lanes<BWD>(sa, sb, L, p.CG, p.RL, R.r1 - R.r0, a, m2);
    if (L.active && L.rl == 0) {
        f32x4* o = p.part + (int64_t)chunk * 2 * p.C4 + L.col4;
        o[0] = a;
        o[p.C4] = m2;
    }
}

// first merge level, one thread per (group, column group): the group's chunks in chunk order
template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void batchnorm_group_kernel(BnP p) {
    const int64_t idx = (int64_t)blockIdx.x * COL_THREADS + threadIdx.x;
    if (idx >= (int64_t)p.ngroups * p.C4) return;
    const int grp = (int)(idx / p.C4), col4 = (int)(idx - (int64_t)grp * p.C4);
    const int q0 = grp * BN_GROUP, q1 = min(p.nchunks, q0 + BN_GROUP);
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    col_merge_chunks<BWD>(p.part + col4, p.C4, q0, q1, p.chunk, p.T, a, m2);
    f32x4* o = p.gpart + (int64_t)grp * 2 * p.C4 + col4;
    o[0] = a;
    o[p.C4] = m2;
}

// second merge level, one thread per column group: the groups in group order, then what hangs on the column totals
template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void batchnorm_finalize_kernel(BnP p) {
    const int col4 = blockIdx.x * COL_THREADS + threadIdx.x;
    if (col4 >= p.C4) return;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    col_merge_chunks<BWD>(p.gpart + col4, p.C4, 0, p.ngroups, (int64_t)BN_GROUP * p.chunk, p.T, a, m2);
    const int c = col4 * 4;
    if (BWD) {
        p.sums[col4] = a;
        p.sums[p.C4 + col4] = m2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p.dbeta) p.dbeta[c + j] = a[j];
            if (p.dgamma) p.dgamma[c + j] = m2[j];
        }
    } else {
        const f32x4 mean = reinterpret_cast<const f32x4*>(p.X)[col4] + a;
        const f32x4 var = m2 * (1.f / (float)p.T);      // biased, as nn.BatchNorm1d normalises with
        f32x4 rstd;
#pragma unroll
        for (int j = 0; j < 4; ++j) rstd[j] = 1.f / sqrtf(var[j] + p.eps);
        bn_store_stats(p, col4, mean, rstd);
        const float unb = (float)p.T / (float)(p.T - 1), m = p.momentum;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p.bvar[c + j] = var[j];
            if (p.rmean) p.rmean[c + j] = (1.f - m) * p.rmean[c + j] + m * mean[j];
            if (p.rvar) p.rvar[c + j] = (1.f - m) * p.rvar[c + j] + m * (var[j] * unb);
        }
    }
}

// eval mode: the statistics are the running buffers
__global__ __launch_bounds__(COL_THREADS) void batchnorm_eval_stats_kernel(BnP p) {
    const int col4 = blockIdx.x * COL_THREADS + threadIdx.x;
    if (col4 >= p.C4) return;
    const int c = col4 * 4;
    f32x4 mean, rstd;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = p.rvar[c + j];
        mean[j] = p.rmean[c + j];
        rstd[j] = 1.f / sqrtf(v + p.eps);
        p.bvar[c + j] = v;
    }
    bn_store_stats(p, col4, mean, rstd);
}

template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void batchnorm_apply_kernel(BnP p) {
    const ColLane L = col_lane(p.CG, p.RL, p.C4, blockIdx.y);
    const int col4 = L.col4;
    if (!L.active) return;
    f32x4 mean, rstd, sc, sh = {0.f, 0.f, 0.f, 0.f};      // sc = rstd gamma ; sh = beta
    bn_load_stats(p, col4, mean, rstd);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sc[j] = rstd[j] * p.gamma[col4 * 4 + j];
        if (!BWD) sh[j] = p.beta[col4 * 4 + j];
    }
    f32x4 m1 = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    if (BWD && p.training) {
        const float inv = 1.f / (float)p.T;
        m1 = p.sums[col4] * inv;
        m2 = p.sums[p.C4 + col4] * inv;
    }
    const uint32_t key = BWD ? drop_key_dev(p.drop) : 0u;
    const ColRows<int64_t> R = col_rows((int)blockIdx.x, p.chunk, p.T);
    const f32x4* X4 = reinterpret_cast<const f32x4*>(p.X) + col4;
    const f32x4* G4 = reinterpret_cast<const f32x4*>(p.G) + col4;
    const f32x4* A4 = reinterpret_cast<const f32x4*>(p.A) + col4;
    f32x4* Y4 = reinterpret_cast<f32x4*>(p.Y) + col4;
#pragma unroll 4
    for (int64_t r = R.r0 + L.rl; r < R.r1; r += p.RL) {
        const f32x4 x = X4[r * p.C4];
        f32x4 y;
        if (BWD) {
            const f32x4 g = G4[r * p.C4];
            y = sc * (g - m1 - (x - mean) * rstd * m2);      // eval: m1 = m2 = 0
            if (p.gate == GT_AUX_GT0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = x[j] > 0.f ? y[j] * p.gate_scale : 0.f;
            } else if (p.gate == GT_AUX_DSILU) {
                const f32x4 pre = A4[r * p.C4];
                const uint32_t idx = (uint32_t)((r * p.C4 + col4) * 4);      // the flat element index of gt_dropout_apply
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    y[j] *= dsilu_f(pre[j]) * (p.drop.thresh ? drop_mul(p.drop, key, idx + j) : 1.f);
            }
        } else {
            y = (x - mean) * sc + sh;
        }
        Y4[r * p.C4] = y;
    }
}

template <bool BWD>
int batchnorm_run(BnP p, void* ws, int64_t ws_bytes, void* stream) {
    if (!p.X || !p.Y || !p.gamma || !p.stats || p.T <= 0 || p.f <= 0) return GT_EINVAL;
    if (p.f % 4 != 0) return GT_ENOTSUP;
    const BnGeom g = bn_geom(p.T, p.f);
    if (g.ncb > 65535) return GT_ENOTSUP;
    if (misaligned16(p.X, p.G, p.A, p.Y, p.stats, ws)) return GT_EALIGN;
    if (misaligned<4>(p.gamma, p.beta, p.bvar, p.rmean, p.rvar, p.dgamma, p.dbeta)) return GT_EALIGN;
    if (!ws || ws_bytes < gt_batchnorm_ws_bytes(p.T, p.f)) return GT_EWS;
    p.C4 = g.C4, p.CG = g.CG, p.RL = g.RL, p.chunk = g.chunk, p.nchunks = g.nchunks, p.ngroups = g.ngroups;
    p.part = reinterpret_cast<f32x4*>(ws);
    p.gpart = p.part + (int64_t)g.nchunks * 2 * g.C4;
    p.sums = p.gpart + (int64_t)g.ngroups * 2 * g.C4;
    const dim3 grid((unsigned)g.nchunks, (unsigned)g.ncb), block(COL_THREADS);
    const dim3 cols((unsigned)((g.C4 + COL_THREADS - 1) / COL_THREADS));
    hipStream_t st = (hipStream_t)stream;
    if (BWD || p.training) {
        hipLaunchKernelGGL(batchnorm_partial_kernel<BWD>, grid, block, 0, st, p);
        GT_LAUNCH_CHECK();
        hipLaunchKernelGGL(batchnorm_group_kernel<BWD>,
                           dim3((unsigned)(((int64_t)g.ngroups * g.C4 + COL_THREADS - 1) / COL_THREADS)), block, 0, st, p);
        GT_LAUNCH_CHECK();
        hipLaunchKernelGGL(batchnorm_finalize_kernel<BWD>, cols, block, 0, st, p);
        GT_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(batchnorm_eval_stats_kernel, cols, block, 0, st, p);
        GT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(batchnorm_apply_kernel<BWD>, grid, block, 0, st, p);
    GT_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace gt

using namespace gt;

extern "C" int64_t gt_batchnorm_ws_bytes(int64_t T, int32_t f) {
    if (T <= 0 || f <= 0 || f % 4 != 0) return 0;
    const BnGeom g = bn_geom(T, f);
    if (g.ncb > 65535) return 0;
    return ((int64_t)g.nchunks + g.ngroups + 1) * 2 * g.C4 * (int64_t)sizeof(f32x4);
}

extern "C" int gt_batchnorm_fwd(const float* X, const float* gamma, const float* beta, float eps, float* running_mean,
                                float* running_var, float momentum, int32_t training, float* Z, float* stats, float* bvar,
                                int64_t T, int32_t f, void* ws, int64_t ws_bytes, void* stream) {
    if (!beta || !bvar || !(eps >= 0.f)) return GT_EINVAL;
    if (training ? (T < 2 || !(momentum >= 0.f && momentum <= 1.f)) : (!running_mean || !running_var)) return GT_EINVAL;
    BnP p{};
    p.X = X, p.Y = Z, p.gamma = gamma, p.beta = beta, p.stats = stats, p.bvar = bvar, p.rmean = running_mean, p.rvar = running_var;
    p.T = T, p.f = f, p.eps = eps, p.momentum = momentum, p.training = training != 0;
    return batchnorm_run<false>(p, ws, ws_bytes, stream);
}

extern "C" int gt_batchnorm_bwd(const float* X, const float* dZ, const float* gamma, const float* stats, float* dX,
                                float* dgamma, float* dbeta, int64_t T, int32_t f, int32_t training, int32_t gate_op,
                                const float* gate_aux, float gate_scale, const gt_dropout* gate_drop, void* ws,
                                int64_t ws_bytes, void* stream) {
    if (!dZ || (training && T < 2)) return GT_EINVAL;
    if (gate_op != GT_AUX_NONE && gate_op != GT_AUX_GT0 && gate_op != GT_AUX_DSILU) return GT_ENOTSUP;
    const bool dropped = gate_drop && gate_drop->p > 0.f;
    if (gate_op == GT_AUX_DSILU ? !gate_aux : dropped) return GT_EINVAL;      // the mask replay belongs to the SiLU gate
    if (dropped && !gate_drop->seed) return GT_EINVAL;
    BnP p{};
    p.X = X, p.G = dZ, p.A = gate_op == GT_AUX_DSILU ? gate_aux : nullptr, p.Y = dX, p.gamma = gamma;
    p.stats = const_cast<float*>(stats), p.dgamma = dgamma, p.dbeta = dbeta;
    p.T = T, p.f = f, p.training = training != 0, p.gate = gate_op, p.gate_scale = gate_scale;
    p.drop = make_drop(gate_drop);
    return batchnorm_run<true>(p, ws, ws_bytes, stream);
}
