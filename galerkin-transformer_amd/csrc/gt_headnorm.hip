// Per-head LayerNorm of the Q / K / V projections with the position concat (gfx950): [T][3 h dk] -> head tiles
// [3][T][h][DP] = [pos(p) | values(dk) | pad], forward and backward.  gt_headtile_* do the same for ONE stream with a row
// count and a leading dimension of its own (cross-attention: Q rows and K, V rows differ), for any dk <= 256 and any
// alignment.  gt_headnorm_* run the bandwidth-shaped v2 kernels, three streams per launch, when dk % 4 == 0, the operands
// are 16-byte aligned and 3 h G <= 1024 (head_geom decides); otherwise the head-tile kernels, once per stream on column
// blocks of the caller's buffers.  The backward leaves d(gamma), d(beta) partials per block; gt_slab_reduce sums them in a
// fixed order.
#include "gt_common.h"

namespace gt {

__device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ f32x4 keep_first(f32x4 v, int nv) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= nv) v[j] = 0.f;
    return v;
}
__device__ __forceinline__ float sum4(f32x4 v) { return v[0] + v[1] + v[2] + v[3]; }

// The per-row LayerNorm of one head segment spread over G lanes (x: this lane's floats, zeros past nv), stated once for the
// kernels below.  Forward: the centred values, with *mu and *rstd.
__device__ __forceinline__ f32x4 seg_center(f32x4 x, int nv, int G, float inv, float eps, float* mu, float* rstd) {
    *mu = group_sum(sum4(x), G) * inv;
    const f32x4 c = keep_first(x - *mu, nv);
    const float var = group_sum(sum4(c * c), G) * inv;
    *rstd = 1.f / sqrtf(var + eps);
    return c;
}
// Backward from the saved (mu, rstd): dx = rstd * (gy g - mean(gy g) - xh mean(gy g xh)); *xh_out for d(gamma).
__device__ __forceinline__ f32x4 seg_norm_bwd(f32x4 x, f32x4 gy, f32x4 gm, int nv, int G, float inv, float mu, float rstd,
                                              f32x4* xh_out) {
    const f32x4 xh = keep_first((x - mu) * rstd, nv);
    const f32x4 gg = gy * gm;
    const float m1 = group_sum(sum4(gg), G) * inv;
    const float m2 = group_sum(sum4(gg * xh), G) * inv;
    *xh_out = xh;
    return rstd * (gg - m1 - xh * m2);
}

// ---- bandwidth-shaped head norm (dk % 4 == 0) ------------------------------------------------------
// Thread layout: PT = 3h*G lanes per token (G = pow2 >= dk/4 lanes per head segment, one float4 each),
// R = blockDim/PT tokens in flight per pass; a lane keeps its (segment, quarter) for the whole kernel, so
// gamma/beta stay in registers and (backward) the affine gradients accumulate in registers.  Segment
// statistics are G-lane shuffle reductions.  qkv / d_qkv move as aligned float4; the head tiles (offset by
// the p coordinate columns) move as float2 when p is even, scalars otherwise.
struct HeadGeom {
    int T, h, dk, p, DP, norm_mask, G, PT, R, tpb;
};

__global__ void headnorm_fwd_v2_kernel(const float* __restrict__ qkv, const float* __restrict__ pos,
                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                       HeadGeom g, float eps, float* __restrict__ out,
                                       float* __restrict__ stats) {
    const int r = threadIdx.x / g.PT, l = threadIdx.x % g.PT;
    if (r >= g.R) return;
    const int seg = l / g.G, q = l % g.G, Q4 = g.dk >> 2;
    const bool active = q < Q4;
    const int stream = seg / g.h, head = seg % g.h;
    const bool normed = (g.norm_mask >> stream) & 1;
    const int ni = __popc(g.norm_mask & ((1 << stream) - 1));
    f32x4 gm = {1.f, 1.f, 1.f, 1.f}, bt = {0.f, 0.f, 0.f, 0.f};
    if (normed && active) {
        gm = *reinterpret_cast<const f32x4*>(gamma + (ni * g.h + head) * g.dk + 4 * q);
        bt = *reinterpret_cast<const f32x4*>(beta + (ni * g.h + head) * g.dk + 4 * q);
    }
    const int d3 = 3 * g.h * g.dk;
    const float inv = 1.f / (float)g.dk;
    const int t_end = min(g.T, (int)(blockIdx.x + 1) * g.tpb);
    // two tokens per trip: both loads are requested before either is consumed
    for (int t = blockIdx.x * g.tpb + r; t < t_end; t += 2 * g.R) {
        const bool two = t + g.R < t_end;
        f32x4 xx[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (active) {
            xx[0] = *reinterpret_cast<const f32x4*>(qkv + (int64_t)t * d3 + seg * g.dk + 4 * q);
            if (two) xx[1] = *reinterpret_cast<const f32x4*>(qkv + (int64_t)(t + g.R) * d3 + seg * g.dk + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !two) break;
            const int tt = t + u * g.R;
            const f32x4 x = xx[u];
            f32x4 y = x;
            if (normed) {
                float mu, rstd;
                y = seg_center(x, active ? 4 : 0, g.G, inv, eps, &mu, &rstd) * rstd * gm + bt;
                if (q == 0)
                    *reinterpret_cast<f32x2*>(stats + (((int64_t)ni * g.T + tt) * g.h + head) * 2) = f32x2{mu, rstd};
            }
            float* row = out + (((int64_t)stream * g.T + tt) * g.h + head) * g.DP;
            if (active) tile_store4(row + g.p + 4 * q, g.p, y);
            if (q == 0)
                for (int j = 0; j < g.p; ++j) row[j] = pos[(int64_t)tt * g.p + j];
            if (q == Q4 - 1)
                for (int j = g.p + g.dk; j < g.DP; ++j) row[j] = 0.f;
        }
    }
}

__global__ void headnorm_bwd_v2_kernel(const float* __restrict__ d_out, const float* __restrict__ qkv,
                                       const float* __restrict__ gamma, const float* __restrict__ stats,
                                       HeadGeom g, float* __restrict__ d_qkv,
                                       float* __restrict__ partial /* [nblk][dg: 2*h*dk | db: 2*h*dk] */) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [R][PT][8]
    const int r = threadIdx.x / g.PT, l = threadIdx.x % g.PT;
    const int hd = g.h * g.dk;
    if (r < g.R) {
        const int seg = l / g.G, q = l % g.G, Q4 = g.dk >> 2;
        const bool active = q < Q4;
        const int stream = seg / g.h, head = seg % g.h;
        const bool normed = (g.norm_mask >> stream) & 1;
        const int ni = __popc(g.norm_mask & ((1 << stream) - 1));
        f32x4 gm = {1.f, 1.f, 1.f, 1.f};
        if (normed && active) gm = *reinterpret_cast<const f32x4*>(gamma + (ni * g.h + head) * g.dk + 4 * q);
        f32x4 dg = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
        const int d3 = 3 * hd;
        const float inv = 1.f / (float)g.dk;
        const int t_end = min(g.T, (int)(blockIdx.x + 1) * g.tpb);
        for (int t = blockIdx.x * g.tpb + r; t < t_end; t += 2 * g.R) {      // two tokens per trip (see forward)
            const bool two = t + g.R < t_end;
            f32x4 gyy[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, xx[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            f32x2 stt[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (u == 1 && !two) break;
                const int tt = t + u * g.R;
                if (active) {
                    gyy[u] = tile_load4(d_out + (((int64_t)stream * g.T + tt) * g.h + head) * g.DP + g.p + 4 * q, g.p);
                    if (normed) xx[u] = *reinterpret_cast<const f32x4*>(qkv + (int64_t)tt * d3 + seg * g.dk + 4 * q);
                }
                if (normed) stt[u] = *reinterpret_cast<const f32x2*>(stats + (((int64_t)ni * g.T + tt) * g.h + head) * 2);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (u == 1 && !two) break;
                const int tt = t + u * g.R;
                const f32x4 gy = gyy[u], x = xx[u];
                f32x4 dx = gy;
                if (normed) {
                    f32x4 xh;
                    dx = seg_norm_bwd(x, gy, gm, active ? 4 : 0, g.G, inv, stt[u][0], stt[u][1], &xh);
                    dg += gy * xh;
                    db += gy;
                }
                if (active) *reinterpret_cast<f32x4*>(d_qkv + (int64_t)tt * d3 + seg * g.dk + 4 * q) = dx;
            }
        }
        float* me = lds + ((size_t)r * g.PT + l) * 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) { me[j] = dg[j]; me[4 + j] = db[j]; }
    }
    __syncthreads();
    // fixed-order combine over the R token rows, one thread per (lane slot, component)
    float* pg = partial + (int64_t)blockIdx.x * 4 * hd;
    const int nn = __popc(g.norm_mask & 7);
    for (int e = threadIdx.x; e < 4 * hd; e += blockDim.x)          // slots of absent norm streams
        if ((e % (2 * hd)) / hd >= nn) pg[e] = 0.f;
    for (int e = threadIdx.x; e < g.PT * 8; e += blockDim.x) {
        const int ll = e >> 3, comp = e & 7;
        const int seg = ll / g.G, q = ll % g.G;
        const int stream = seg / g.h, head = seg % g.h;
        if (q >= (g.dk >> 2) || !((g.norm_mask >> stream) & 1)) continue;
        const int ni = __popc(g.norm_mask & ((1 << stream) - 1));
        float s = 0.f;
        for (int rr = 0; rr < g.R; ++rr) s += lds[((size_t)rr * g.PT + ll) * 8 + comp];
        const int idx = ni * hd + head * g.dk + 4 * q + (comp & 3);
        pg[(comp < 4 ? 0 : 2 * hd) + idx] = s;
    }
}

static bool head_geom(int T, int h, int dk, int p, int norm_mask, int max_blocks, HeadGeom* g, int* threads,
                      int* blocks) {
    if (dk & 3) return false;
    int G = 1;
    while (G < dk / 4) G <<= 1;
    if (G > 64) return false;
    const int PT = 3 * h * G;
    if (PT > 1024) return false;
    // whole waves with no idle lanes when PT and the wave size have a small common multiple (PT = 96 -> 384)
    int lcm = PT;
    while (lcm % 64) lcm += PT;
    int thr = lcm <= 512 ? lcm * std::max(1, 384 / lcm) : std::max(256, ((PT + 63) / 64) * 64);
    const int R = thr / PT;
    int nblk = std::min(max_blocks, ceil_div(T, R * 8));
    nblk = std::max(nblk, 1);
    int tpb = ceil_div(T, nblk);
    tpb = ceil_div(tpb, R) * R;
    nblk = ceil_div(T, tpb);
    *g = HeadGeom{T, h, dk, p, (dk + p + 3) & ~3, norm_mask, G, PT, R, tpb};
    *threads = thr;
    *blocks = nblk;
    return true;
}

// ---- single-stream head tiles (cross-attention; every shape the kernels above do not take) ----------------------------
// One stream of the above on its own row count: X [T][ldx] (a column block of a wider projection buffer) -> out [T][h][DP]
// = [pos | values | zero pad], stats [T][h][2]; gamma == NULL: no norm.  The lane layout of the v2 kernels with PT = h*G
// lanes per token: a lane owns the floats 4q .. 4q+3 of its head segment for the whole kernel.  VEC (dk % 4 == 0, 16-byte
// aligned operands) moves them as float4; otherwise the same kernels move scalars and a segment's last lane holds
// nv < 4 of them, so any dk up to 256 runs.
struct StreamGeom {
    int T, h, dk, p, DP, G, PT, R, tpb;
    int64_t ldx, lddx;
};

template <bool VEC>
__device__ __forceinline__ f32x4 lane_load(const float* __restrict__ src, int nv) {
    if constexpr (VEC) return *reinterpret_cast<const f32x4*>(src);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nv) v[j] = src[j];
    return v;
}
template <bool VEC>
__device__ __forceinline__ void lane_store(float* __restrict__ dst, int nv, f32x4 v) {
    if constexpr (VEC) *reinterpret_cast<f32x4*>(dst) = v;
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) dst[j] = v[j];
    }
}

template <bool VEC>
__global__ void headtile_fwd_kernel(const float* __restrict__ X, const float* __restrict__ pos,
                                    const float* __restrict__ gamma, const float* __restrict__ beta, StreamGeom g,
                                    float eps, float* __restrict__ out, float* __restrict__ stats) {
    const int r = threadIdx.x / g.PT, l = threadIdx.x % g.PT;
    if (r >= g.R) return;
    const int head = l / g.G, q = l % g.G;
    const int nv = max(0, min(4, g.dk - 4 * q));
    const bool normed = gamma != nullptr;
    f32x4 gm = {1.f, 1.f, 1.f, 1.f}, bt = {0.f, 0.f, 0.f, 0.f};
    if (normed && nv > 0) {
        gm = lane_load<VEC>(gamma + head * g.dk + 4 * q, nv);
        bt = lane_load<VEC>(beta + head * g.dk + 4 * q, nv);
    }
    const float inv = 1.f / (float)g.dk;
    const int t_end = min(g.T, (int)(blockIdx.x + 1) * g.tpb);
    for (int t = blockIdx.x * g.tpb + r; t < t_end; t += g.R) {
        f32x4 y = {0.f, 0.f, 0.f, 0.f};
        if (nv > 0) y = lane_load<VEC>(X + (int64_t)t * g.ldx + head * g.dk + 4 * q, nv);
        if (normed) {
            float mu, rstd;
            y = seg_center(y, nv, g.G, inv, eps, &mu, &rstd) * rstd * gm + bt;
            if (q == 0) {
                float* st = stats + ((int64_t)t * g.h + head) * 2;
                st[0] = mu;
                st[1] = rstd;
            }
        }
        float* row = out + ((int64_t)t * g.h + head) * g.DP;
        if (nv > 0) {
            if constexpr (VEC) tile_store4(row + g.p + 4 * q, g.p, y);
            else lane_store<false>(row + g.p + 4 * q, nv, y);
        }
        if (q == 0) {
            for (int j = 0; j < g.p; ++j) row[j] = pos[(int64_t)t * g.p + j];
            for (int j = g.p + g.dk; j < g.DP; ++j) row[j] = 0.f;
        }
    }
}

template <bool VEC>
__global__ void headtile_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ X,
                                    const float* __restrict__ gamma, const float* __restrict__ stats, StreamGeom g,
                                    float* __restrict__ dX, float* __restrict__ partial /* [nblk][dg: h*dk | db: h*dk] */) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [R][PT][8]
    const int r = threadIdx.x / g.PT, l = threadIdx.x % g.PT;
    const int hd = g.h * g.dk;
    const bool normed = gamma != nullptr;
    if (r < g.R) {
        const int head = l / g.G, q = l % g.G;
        const int nv = max(0, min(4, g.dk - 4 * q));
        f32x4 gm = {1.f, 1.f, 1.f, 1.f};
        if (normed && nv > 0) gm = lane_load<VEC>(gamma + head * g.dk + 4 * q, nv);
        f32x4 dg = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
        const float inv = 1.f / (float)g.dk;
        const int t_end = min(g.T, (int)(blockIdx.x + 1) * g.tpb);
        for (int t = blockIdx.x * g.tpb + r; t < t_end; t += g.R) {
            f32x4 gy = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
            if (nv > 0) {
                const float* row = d_out + ((int64_t)t * g.h + head) * g.DP + g.p + 4 * q;
                if constexpr (VEC) gy = tile_load4(row, g.p);
                else gy = lane_load<false>(row, nv);
                if (normed) x = lane_load<VEC>(X + (int64_t)t * g.ldx + head * g.dk + 4 * q, nv);
            }
            f32x4 dx = gy;
            if (normed) {
                const float* st = stats + ((int64_t)t * g.h + head) * 2;
                f32x4 xh;
                dx = seg_norm_bwd(x, gy, gm, nv, g.G, inv, st[0], st[1], &xh);
                dg += gy * xh;
                db += gy;
            }
            if (nv > 0) lane_store<VEC>(dX + (int64_t)t * g.lddx + head * g.dk + 4 * q, nv, dx);
        }
        if (normed) {
            float* me = lds + ((size_t)r * g.PT + l) * 8;
#pragma unroll
            for (int j = 0; j < 4; ++j) { me[j] = dg[j]; me[4 + j] = db[j]; }
        }
    }
    if (!normed) return;
    __syncthreads();
    // fixed-order combine over the R token rows, one thread per (lane slot, component)
    float* pg = partial + (int64_t)blockIdx.x * 2 * hd;
    for (int e = threadIdx.x; e < g.PT * 8; e += blockDim.x) {
        const int ll = e >> 3, comp = e & 7;
        const int head = ll / g.G, c = 4 * (ll % g.G) + (comp & 3);
        if (c >= g.dk) continue;
        float s = 0.f;
        for (int rr = 0; rr < g.R; ++rr) s += lds[((size_t)rr * g.PT + ll) * 8 + comp];
        pg[(comp < 4 ? 0 : hd) + head * g.dk + c] = s;
    }
}

static bool stream_geom(int T, int h, int dk, int p, int64_t ldx, int64_t lddx, int max_blocks, StreamGeom* g, int* threads,
                        int* blocks) {
    int G = 1;
    while (G < (dk + 3) / 4) G <<= 1;
    if (G > 64) return false;
    const int PT = h * G;                  // a multiple of G, G | 64: no segment's lanes straddle a wave
    if (PT > 1024) return false;
    const int thr = std::max(256, ((PT + 63) / 64) * 64);
    const int R = thr / PT;
    int nblk = std::max(1, std::min(max_blocks, ceil_div(T, R * 8)));
    const int tpb = ceil_div(ceil_div(T, nblk), R) * R;
    nblk = ceil_div(T, tpb);
    *g = StreamGeom{T, h, dk, p, (dk + p + 3) & ~3, G, PT, R, tpb, ldx, lddx};
    *threads = thr;
    *blocks = nblk;
    return true;
}

constexpr int HN_MAXB = 1024;      // bound on blocks (= dgamma/dbeta partials) of the backward

}  // namespace gt

using namespace gt;

extern "C" int gt_headnorm_fwd(const float* qkv, const float* pos, const float* gamma, const float* beta,
                               int32_t T, int32_t h, int32_t dk, int32_t p, int32_t norm_mask, float eps,
                               float* out, float* stats, void* stream) {
    if (!qkv || !out || T <= 0 || h <= 0 || dk <= 0 || p < 0) return GT_EINVAL;
    if (p > 0 && !pos) return GT_EINVAL;
    if (norm_mask & ~7) return GT_EINVAL;
    if (norm_mask && (!gamma || !beta || !stats)) return GT_EINVAL;
    HeadGeom g; int thr, nblk;
    if (!misaligned16(qkv, out, gamma, beta, stats) && head_geom(T, h, dk, p, norm_mask, 1 << 20, &g, &thr, &nblk)) {
        hipLaunchKernelGGL(headnorm_fwd_v2_kernel, dim3(nblk), dim3(thr), 0, (hipStream_t)stream, qkv, pos,
                           gamma, beta, g, eps, out, stats);
        GT_LAUNCH_CHECK();
        return 0;
    }
    // stream s: the column block s of qkv into the tile block s of out; ni counts the normalised streams below it
    const int64_t hd = (int64_t)h * dk, tile = (int64_t)T * h * round4(dk + p), st = (int64_t)T * h * 2;
    for (int s = 0, ni = 0; s < 3; ++s) {
        const bool normed = (norm_mask >> s) & 1;
        if (int rc = gt_headtile_fwd(qkv + s * hd, 3 * hd, pos, normed ? gamma + ni * hd : nullptr,
                                     normed ? beta + ni * hd : nullptr, T, h, dk, p, eps, out + s * tile,
                                     normed ? stats + ni * st : nullptr, stream))
            return rc;
        ni += normed;
    }
    return 0;
}

extern "C" int64_t gt_headnorm_bwd_ws_bytes(int32_t T, int32_t h, int32_t dk) {
    (void)T;
    return (int64_t)HN_MAXB * 4 * h * dk * (int64_t)sizeof(float);      // v2's partials; twice one head-tile stream's
}

extern "C" int gt_headnorm_bwd(const float* d_out, const float* qkv, const float* gamma, const float* stats,
                               int32_t T, int32_t h, int32_t dk, int32_t p, int32_t norm_mask, float* d_qkv,
                               float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, void* stream) {
    if (!d_out || !qkv || !d_qkv || T <= 0 || h <= 0 || dk <= 0 || p < 0) return GT_EINVAL;
    if (norm_mask & ~7) return GT_EINVAL;
    if (norm_mask && (!gamma || !stats || !dgamma || !dbeta)) return GT_EINVAL;
    if (!ws || ws_bytes < gt_headnorm_bwd_ws_bytes(T, h, dk)) return GT_EWS;
    const int64_t hd = (int64_t)h * dk;
    HeadGeom g; int thr, nblk;
    if (!misaligned16(qkv, d_qkv, gamma, stats, d_out) && head_geom(T, h, dk, p, norm_mask, HN_MAXB, &g, &thr, &nblk)) {
        float* partial = reinterpret_cast<float*>(ws);      // [nblk][ (dg: 2*hd) | (db: 2*hd) ]
        const size_t lds = (size_t)g.R * g.PT * 8 * sizeof(float);
        hipLaunchKernelGGL(headnorm_bwd_v2_kernel, dim3(nblk), dim3(thr), lds, (hipStream_t)stream, d_out,
                           qkv, gamma, stats, g, d_qkv, partial);
        GT_LAUNCH_CHECK();
        if (!norm_mask) return 0;
        if (int rc = gt_slab_reduce(partial, 4 * hd, nblk, 2 * hd, 1.f, dgamma, stream)) return rc;
        return gt_slab_reduce(partial + 2 * hd, 4 * hd, nblk, 2 * hd, 1.f, dbeta, stream);
    }
    // per stream as in the forward; the streams run in order on `stream`, so each reuses ws for its partials
    const int64_t tile = (int64_t)T * h * round4(dk + p), st = (int64_t)T * h * 2;
    int ni = 0;
    for (int s = 0; s < 3; ++s) {
        const bool normed = (norm_mask >> s) & 1;
        if (int rc = gt_headtile_bwd(d_out + s * tile, qkv + s * hd, 3 * hd, normed ? gamma + ni * hd : nullptr,
                                     normed ? stats + ni * st : nullptr, T, h, dk, p, d_qkv + s * hd, 3 * hd,
                                     normed ? dgamma + ni * hd : nullptr, normed ? dbeta + ni * hd : nullptr, ws,
                                     ws_bytes, stream))
            return rc;
        ni += normed;
    }
    if (ni == 1) {      // the slot with no stream reads zero, as from the kernel above
        hipError_t e = hipMemsetAsync(dgamma + hd, 0, hd * sizeof(float), (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(dbeta + hd, 0, hd * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int gt_headtile_fwd(const float* X, int64_t ldx, const float* pos, const float* gamma, const float* beta,
                               int32_t T, int32_t h, int32_t dk, int32_t p, float eps, float* out, float* stats,
                               void* stream) {
    if (!X || !out || T <= 0 || h <= 0 || dk <= 0 || p < 0 || ldx < (int64_t)h * dk) return GT_EINVAL;
    if (p > 0 && !pos) return GT_EINVAL;
    if (gamma && (!beta || !stats)) return GT_EINVAL;
    StreamGeom g; int thr, nblk;
    if (!stream_geom(T, h, dk, p, ldx, 0, 1 << 20, &g, &thr, &nblk)) return GT_ENOTSUP;
    const bool vec = !(dk & 3) && !(ldx & 3) && !misaligned16(X, out, gamma, beta) && !misaligned<8>(stats);
    hipLaunchKernelGGL(vec ? headtile_fwd_kernel<true> : headtile_fwd_kernel<false>, dim3(nblk), dim3(thr), 0,
                       (hipStream_t)stream, X, pos, gamma, beta, g, eps, out, stats);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_headtile_bwd_ws_bytes(int32_t T, int32_t h, int32_t dk) {
    (void)T;
    return (int64_t)HN_MAXB * 2 * h * dk * (int64_t)sizeof(float);
}

extern "C" int gt_headtile_bwd(const float* d_out, const float* X, int64_t ldx, const float* gamma, const float* stats,
                               int32_t T, int32_t h, int32_t dk, int32_t p, float* dX, int64_t lddx, float* dgamma,
                               float* dbeta, void* ws, int64_t ws_bytes, void* stream) {
    if (!d_out || !dX || T <= 0 || h <= 0 || dk <= 0 || p < 0 || lddx < (int64_t)h * dk) return GT_EINVAL;
    if (gamma && (!X || ldx < (int64_t)h * dk || !stats || !dgamma || !dbeta)) return GT_EINVAL;
    if (gamma && (!ws || ws_bytes < gt_headtile_bwd_ws_bytes(T, h, dk))) return GT_EWS;
    StreamGeom g; int thr, nblk;
    if (!stream_geom(T, h, dk, p, ldx, lddx, HN_MAXB, &g, &thr, &nblk)) return GT_ENOTSUP;
    const bool vec = !(dk & 3) && !(lddx & 3) && !(gamma && (ldx & 3)) && 
                     !misaligned16(d_out, dX, gamma ? X : (const float*)nullptr, gamma);
    const size_t lds = gamma ? (size_t)g.R * g.PT * 8 * sizeof(float) : 0;
    float* partial = reinterpret_cast<float*>(ws);
    hipLaunchKernelGGL(vec ? headtile_bwd_kernel<true> : headtile_bwd_kernel<false>, dim3(nblk), dim3(thr), lds,
                       (hipStream_t)stream, d_out, X, gamma, stats, g, dX, partial);
    GT_LAUNCH_CHECK();
    if (gamma) {
        const int hd = h * dk;
        if (int rc = gt_slab_reduce(partial, 2 * hd, nblk, hd, 1.f, dgamma, stream)) return rc;
        return gt_slab_reduce(partial + hd, 2 * hd, nblk, hd, 1.f, dbeta, stream);
    }
    return 0;
}
