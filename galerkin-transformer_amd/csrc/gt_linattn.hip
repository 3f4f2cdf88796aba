// The softmax pair of the 'linear' / 'global' attention family (reference layers.py:719-722):
//     Q~ = softmax(Q', dim=-1)   over the Dr = dk + p columns of every (token, head) segment       ("feature softmax")
//     K~ = softmax(K', dim=-2)   over the n tokens of every (batch, head, column < Dr)              ("token softmax")
// forward and backward on the head-tile layout [B*n][h][DP], DP = round4(Dr), fp32.  Pad columns Dr..DP-1 take no part in
// either softmax and are written as exact zeros.  Everything else of the family (K~^T V', the finalize pair, Q~ P, dK / dV)
// is the Galerkin path's kernels on (Q~, K~, V').
//
// Both operators are streaming passes: 16-byte loads and stores, one exponential per element and pass, reductions in a
// fixed order (no atomics): two runs give the same bits.  In-place use (Y == X, dX == dY) is allowed: every block reads
// the elements it owns before it writes them, and no block reads another block's elements of the written tensor.
#include <math.h>

#include <algorithm>

#include "gt_colpass.h"

namespace gt {
namespace {

// ------------------------------------------------------------------------------------------ feature softmax
// A segment is DP floats = L4 = DP / 4 float4 (4, 5, 8, 9, ... 25): no power of two, so lanes are not tied to segments.  A
// block owns S consecutive segments: its 256 threads stream the S * L4 float4 as one flat, fully coalesced array (at most
// FS_ITERS per thread, kept in registers) and park a copy in LDS; thread s < S then reduces segment s from LDS; the third
// phase finishes the elements from the registers.  No lane idles on the HBM phases whatever DP.  The LDS rows have an odd
// pitch of LP = L4 | 1 float4, so the 16 lanes of a ds_read_b128 group hit 16 different 16-byte slots.
constexpr int FS_THREADS = 256;
constexpr int FS_ITERS = 6;
constexpr int FS_F4 = FS_THREADS * FS_ITERS;      // 24 KiB of LDS

#define FS_ADVANCE(seg, c)      \
    do {                        \
        seg += dseg;            \
        c += dc;                \
        if (c >= L4) {          \
            c -= L4;            \
            ++seg;              \
        }                       \
    } while (0)

static inline int fs_segments(int L4) { return std::min(FS_THREADS, FS_F4 / (L4 | 1)); }

__global__ __launch_bounds__(FS_THREADS) void feature_softmax_fwd_kernel(const float* X, float* Y, int64_t rows, int L4,
                                                                         int Dr, int S) {
    __shared__ f32x4 buf[FS_F4];
    __shared__ f32x2 stat[FS_THREADS];
    const int tid = threadIdx.x;
    const int LP = L4 | 1;
    const int64_t seg0 = (int64_t)blockIdx.x * S;
    const int nseg = rows - seg0 < S ? (int)(rows - seg0) : S;
    const int nf4 = nseg * L4;
    const int dseg = FS_THREADS / L4, dc = FS_THREADS - dseg * L4;      // float4 index g -> (segment, column group), stepped
    int seg = tid / L4, c = tid - seg * L4;
    const f32x4* src = reinterpret_cast<const f32x4*>(X) + seg0 * L4;
    f32x4* dst = reinterpret_cast<f32x4*>(Y) + seg0 * L4;
    f32x4 v[FS_ITERS];
#pragma unroll
    for (int i = 0; i < FS_ITERS; ++i) {
        const int g = tid + i * FS_THREADS;
        v[i] = src[g < nf4 ? g : 0];             // unconditional (clamped) load: keeps v[] in plain registers
        if (g < nf4) buf[seg * LP + c] = v[i];
        FS_ADVANCE(seg, c);
    }
    __syncthreads();
    if (tid < nseg) {
        const f32x4* r = buf + tid * LP;
        float m = -INFINITY;
        for (int c = 0; c < L4; ++c) {
            const f32x4 a = r[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c + j < Dr) m = fmaxf(m, a[j]);
        }
        float s = 0.f;
        for (int c = 0; c < L4; ++c) {
            const f32x4 a = r[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c + j < Dr) s += expf(a[j] - m);
        }
        f32x2 st;
        st[0] = m;
        st[1] = 1.f / s;
        stat[tid] = st;
    }
    __syncthreads();
    seg = tid / L4;
    c = tid - seg * L4;
#pragma unroll
    for (int i = 0; i < FS_ITERS; ++i) {
        const int g = tid + i * FS_THREADS;
        if (g < nf4) {
            const f32x2 st = stat[seg];
            f32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = (4 * c + j < Dr) ? expf(v[i][j] - st[0]) * st[1] : 0.f;
            dst[g] = y;
        }
        FS_ADVANCE(seg, c);
    }
}

// dX = Y .* (dY - sum_c Y .* dY): the products go to LDS for the per-segment sum, Y and dY stay in registers.
__global__ __launch_bounds__(FS_THREADS) void feature_softmax_bwd_kernel(const float* Yp, const float* dYp, float* dXp,
                                                                         int64_t rows, int L4, int Dr, int S) {
    __shared__ f32x4 buf[FS_F4];
    __shared__ float dots[FS_THREADS];
    const int tid = threadIdx.x;
    const int LP = L4 | 1;
    const int64_t seg0 = (int64_t)blockIdx.x * S;
    const int nseg = rows - seg0 < S ? (int)(rows - seg0) : S;
    const int nf4 = nseg * L4;
    const int dseg = FS_THREADS / L4, dc = FS_THREADS - dseg * L4;      // float4 index g -> (segment, column group), stepped
    int seg = tid / L4, c = tid - seg * L4;
    const f32x4* ys = reinterpret_cast<const f32x4*>(Yp) + seg0 * L4;
    const f32x4* gs = reinterpret_cast<const f32x4*>(dYp) + seg0 * L4;
    f32x4* dst = reinterpret_cast<f32x4*>(dXp) + seg0 * L4;
    f32x4 y[FS_ITERS], g4[FS_ITERS];
#pragma unroll
    for (int i = 0; i < FS_ITERS; ++i) {
        const int g = tid + i * FS_THREADS;
        y[i] = ys[g < nf4 ? g : 0];              // unconditional (clamped) loads: keep y[], g4[] in plain registers
        g4[i] = gs[g < nf4 ? g : 0];
        if (g < nf4) buf[seg * LP + c] = y[i] * g4[i];
        FS_ADVANCE(seg, c);
    }
    __syncthreads();
    if (tid < nseg) {
        const f32x4* r = buf + tid * LP;
        float s = 0.f;
        for (int c = 0; c < L4; ++c) {
            const f32x4 a = r[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c + j < Dr) s += a[j];
        }
        dots[tid] = s;
    }
    __syncthreads();
    seg = tid / L4;
    c = tid - seg * L4;
#pragma unroll
    for (int i = 0; i < FS_ITERS; ++i) {
        const int g = tid + i * FS_THREADS;
        if (g < nf4) {
            const float dot = dots[seg];
            f32x4 dx;
#pragma unroll
            for (int j = 0; j < 4; ++j) dx[j] = (4 * c + j < Dr) ? y[i][j] * (g4[i][j] - dot) : 0.f;
            dst[g] = dx;
        }
        FS_ADVANCE(seg, c);
    }
}

// ------------------------------------------------------------------------------------------ token softmax
// One batch item is a dense [n][C4] array of float4 (C4 = h * DP / 4 column groups), contiguous along the columns, and the
// softmax runs down the rows: the block shape and the lane-order merge are those of gt_colpass.h.  A block owns TS_CHUNK
// consecutive tokens of one batch item and CG <= 256 adjacent column groups; its threads form RL = 256 / CG row lanes, so a
// wave reads whole contiguous rows.  Pass 1 keeps a running (max, sum) per column and row lane (online rescaling), merges
// the row lanes in LDS in lane order and writes one partial per (batch, chunk, column).  Pass 2 merges the partials of all
// chunks -- chunks q = lane, lane + RL, ... per row lane, then the lanes in order, the same order in every block -- and
// writes exp(x - max) / sum for its own tokens.
// The backward is the same pair of passes with plain sums:  c = sum_t K~ .* dK~,  dK' = K~ .* (dK~ - c).
constexpr int TS_CHUNK = 128;      // constant, whatever the batch: the chunk count fixes pass 2's merge order

struct TsGeom : ColGeom {
    int nchunks;
};
static inline TsGeom ts_geom(int n, int h, int DP) { return {col_geom(h * DP / 4), (n + TS_CHUNK - 1) / TS_CHUNK}; }

// (m, s) <- (m, s) merged with (m2, s2); an empty side has s == 0 (and m == -inf)
__device__ __forceinline__ void ts_merge(f32x4& m, f32x4& s, const f32x4 m2, const f32x4 s2) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s2[j] > 0.f) {
            const float M = fmaxf(m[j], m2[j]);
            s[j] = s[j] * expf(m[j] - M) + s2[j] * expf(m2[j] - M);
            m[j] = M;
        }
}

struct TsP {
    const float* X;      // fwd: K' ; bwd: K~
    const float* G;      // bwd: dK~
    float* Y;            // fwd: K~ ; bwd: dK'
    f32x4* part;         // fwd: [B][nchunks][2][C4] (max, sum) ; bwd: [B][nchunks][C4]
    int n, C4, CG, RL, nchunks, DP, Dr;
};

// lanes 1 .. RL-1 of column cl folded into (m, s) in lane order; the backward has sums only and never reads the max array
template <bool BWD>
__device__ __forceinline__ void ts_fold_lanes(const f32x4* sm, const f32x4* ss, const TsP& p, int cl, f32x4& m, f32x4& s) {
    col_fold_lanes(sm, ss, p.CG, p.RL, cl, [&](const f32x4 m2, const f32x4 s2, int) {
        if (BWD) s += s2;
        else ts_merge(m, s, m2, s2);
    });
}

template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void token_softmax_stats_kernel(TsP p) {
    __shared__ f32x4 sm[COL_THREADS], ss[COL_THREADS];
    const int t = threadIdx.x;
    const ColLane L = col_lane(p.CG, p.RL, p.C4, blockIdx.z);
    const int b = blockIdx.y, chunk = blockIdx.x, col4 = L.col4;
    const ColRows<int> R = col_rows(chunk, TS_CHUNK, p.n);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s = {0.f, 0.f, 0.f, 0.f};      // the empty partial
    if (L.active) {
        const int64_t base = (int64_t)b * p.n * p.C4 + col4;
        const f32x4* X4 = reinterpret_cast<const f32x4*>(p.X) + base;
        const f32x4* G4 = reinterpret_cast<const f32x4*>(p.G) + base;
#pragma unroll 4
        for (int r = R.r0 + L.rl; r < R.r1; r += p.RL) {
            const f32x4 x = X4[(int64_t)r * p.C4];
            if (BWD) {
                s += x * G4[(int64_t)r * p.C4];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float e = expf(-fabsf(x[j] - m[j]));      // m = -inf on the first row: e = 0, s = 0 * 0 + 1
                    if (x[j] > m[j]) {
                        s[j] = s[j] * e + 1.f;
                        m[j] = x[j];
                    } else {
                        s[j] += e;
                    }
                }
            }
        }
    }
    sm[t] = m;
    ss[t] = s;
    __syncthreads();
    if (L.active && L.rl == 0) {
        ts_fold_lanes<BWD>(sm, ss, p, L.cl, m, s);
        if (BWD) {
            p.part[((int64_t)b * p.nchunks + chunk) * p.C4 + col4] = s;
        } else {
            f32x4* o = p.part + ((int64_t)b * p.nchunks + chunk) * 2 * p.C4 + col4;
            o[0] = m;
            o[p.C4] = s;
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(COL_THREADS) void token_softmax_apply_kernel(TsP p) {
    __shared__ f32x4 sm[COL_THREADS], ss[COL_THREADS];
    const int t = threadIdx.x;
    const ColLane L = col_lane(p.CG, p.RL, p.C4, blockIdx.z);
    const int b = blockIdx.y, chunk = blockIdx.x, col4 = L.col4;
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s = {0.f, 0.f, 0.f, 0.f};      // the empty partial
    if (L.active) {
        for (int q = L.rl; q < p.nchunks; q += p.RL) {
            if (BWD) {
                s += p.part[((int64_t)b * p.nchunks + q) * p.C4 + col4];
            } else {
                const f32x4* o = p.part + ((int64_t)b * p.nchunks + q) * 2 * p.C4 + col4;
                const f32x4 m2 = o[0], s2 = o[p.C4];
                ts_merge(m, s, m2, s2);
            }
        }
    }
    sm[t] = m;
    ss[t] = s;
    __syncthreads();
    if (!L.active) return;
    m = sm[L.cl];
    s = ss[L.cl];
    ts_fold_lanes<BWD>(sm, ss, p, L.cl, m, s);
    bool valid[4];
    const int c0 = (col4 * 4) % p.DP;        // DP % 4 == 0: a float4 never straddles two heads
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        valid[j] = c0 + j < p.Dr;
        if (!BWD) s[j] = 1.f / s[j];
    }
    const ColRows<int> R = col_rows(chunk, TS_CHUNK, p.n);
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
            for (int j = 0; j < 4; ++j) y[j] = valid[j] ? x[j] * (g[j] - s[j]) : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = valid[j] ? expf(x[j] - m[j]) * s[j] : 0.f;
        }
        Y4[(int64_t)r * p.C4] = y;
    }
}

template <bool BWD>
int token_softmax_run(const float* X, const float* G, float* Y, int B, int n, int h, int dk, int pd, void* ws,
                      int64_t ws_bytes, void* stream) {
    if (!X || !Y || (BWD && !G) || B <= 0 || n <= 0 || h <= 0) return GT_EINVAL;
    if (!head_tile_shape_ok(dk, pd) || B > 65535) return GT_ENOTSUP;
    if (misaligned16(X, G, Y, ws)) return GT_EALIGN;
    if (!ws || ws_bytes < gt_token_softmax_ws_bytes(B, n, h, dk, pd)) return GT_EWS;
    const int Dr = dk + pd, DP = round4(Dr);
    const TsGeom g = ts_geom(n, h, DP);
    if (g.ncb > 65535) return GT_ENOTSUP;
    TsP p{X, G, Y, reinterpret_cast<f32x4*>(ws), n, g.C4, g.CG, g.RL, g.nchunks, DP, Dr};
    dim3 grid((unsigned)g.nchunks, (unsigned)B, (unsigned)g.ncb);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(token_softmax_stats_kernel<BWD>, grid, dim3(COL_THREADS), 0, st, p);
    GT_LAUNCH_CHECK();
    hipLaunchKernelGGL(token_softmax_apply_kernel<BWD>, grid, dim3(COL_THREADS), 0, st, p);
    GT_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace gt

using namespace gt;

extern "C" int gt_feature_softmax_fwd(const float* X, float* Y, int64_t rows, int32_t dk, int32_t p, void* stream) {
    if (!X || !Y || rows <= 0) return GT_EINVAL;
    if (!head_tile_shape_ok(dk, p)) return GT_ENOTSUP;
    if (misaligned16(X, Y)) return GT_EALIGN;
    const int Dr = dk + p, L4 = round4(Dr) / 4, S = fs_segments(L4);
    const int64_t nblk = (rows + S - 1) / S;
    if (nblk > 0x7fffffff) return GT_ENOTSUP;
    hipLaunchKernelGGL(feature_softmax_fwd_kernel, dim3((unsigned)nblk), dim3(FS_THREADS), 0, (hipStream_t)stream, X, Y, rows,
                       L4, Dr, S);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_feature_softmax_bwd(const float* Y, const float* dY, float* dX, int64_t rows, int32_t dk, int32_t p,
                                      void* stream) {
    if (!Y || !dY || !dX || rows <= 0) return GT_EINVAL;
    if (!head_tile_shape_ok(dk, p)) return GT_ENOTSUP;
    if (misaligned16(Y, dY, dX)) return GT_EALIGN;
    const int Dr = dk + p, L4 = round4(Dr) / 4, S = fs_segments(L4);
    const int64_t nblk = (rows + S - 1) / S;
    if (nblk > 0x7fffffff) return GT_ENOTSUP;
    hipLaunchKernelGGL(feature_softmax_bwd_kernel, dim3((unsigned)nblk), dim3(FS_THREADS), 0, (hipStream_t)stream, Y, dY, dX,
                       rows, L4, Dr, S);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_token_softmax_ws_bytes(int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p) {
    if (B <= 0 || n <= 0 || h <= 0 || !head_tile_shape_ok(dk, p)) return 0;
    const TsGeom g = ts_geom(n, h, round4(dk + p));
    return (int64_t)B * g.nchunks * 2 * g.C4 * (int64_t)sizeof(f32x4);
}

extern "C" int gt_token_softmax_fwd(const float* X, float* Y, int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p,
                                    void* ws, int64_t ws_bytes, void* stream) {
    return token_softmax_run<false>(X, nullptr, Y, B, n, h, dk, p, ws, ws_bytes, stream);
}

extern "C" int gt_token_softmax_bwd(const float* Y, const float* dY, float* dX, int32_t B, int32_t n, int32_t h,
                                    int32_t dk, int32_t p, void* ws, int64_t ws_bytes, void* stream) {
    return token_softmax_run<true>(Y, dY, dX, B, n, h, dk, p, ws, ws_bytes, stream);
}
