// Causal linear attention (layers.py:736-762, attention_type='causal') in fp32, linear in the token count.
//
// Per (sample, head), on head tiles [T, h, DP] with zero pad columns and an optional keep vector [B, n] (bytes, 0 = dropped):
//
//   k^_j = keep_j k_j / n,  v^_j = keep_j v_j,  S_i = sum_{j<=i} k^_j v^_j^T (DP x DP),  z_i = sum_{j<=i} k^_j
//   den_i = sum_d (z_i[d] + eps) q_i[d],        out_i = S_i^T q_i / den_i
//
// i.e. A = tril(Q K^^T), out = A V^ / (rowsum(A) + eps sum_d q).  Neither the n x n matrix A nor the [n, DP, DP] running state
// reaches HBM: the token axis is cut into chunks of 64 and every direction runs three stages,
//
//   1  causal_chunk_sums   per chunk c:  X_c^T Y_c (DP x DP) and sum_t w_t x_t      forward: X = K^, Y = V^, w = 1
//   2  causal_scan         exclusive prefix over the chunks of a (sample, head), in place, in chunk order
//   3  causal_fwd_kernel   num = Q_c S_prev + tril(Q_c K^_c^T) V^_c,  den likewise from z_prev;  out = num / den
//
// The backward, with g_i = dout_i / den_i, c_i = -(dout_i . out_i) / den_i (causal_rowdot) and W_ij = tril(g_i . v^_j + c_i):
//
//   dq_i  = S_prev g_i + c_i (z_prev + eps) + sum_j W_ij k^_j                        causal_bwd_q_kernel  (owner: queries)
//   dk^_j = R_next v^_j + r_next + sum_i W_ij q_i,   dk_j = keep_j / n dk^_j          causal_bwd_kv_kernel (owner: keys)
//   dv_j  = keep_j (R_next^T k^_j + sum_i A_ij g_i)
//
// R_next = sum of q_i g_i^T, r_next = sum of c_i q_i over the LATER chunks: stage 1 with X = Q, Y = G, w = c and stage 2 run
// in reverse.  S_prev / z_prev are the forward's stage-2 result, kept by the caller for the backward (not recomputed).
//
// Lane layout as in gt_softmax.hip: the score tile is computed transposed (stream rows x owner columns), so that an owner's
// column lives in lane j of the four kq groups and the tile is the B operand of the second product straight from the
// accumulator registers; k-step s of row tile mt contracts stream row 16mt + 4kq + s = accumulator register s.  A wave owns
// 16 tokens of the chunk, a block of four waves the chunk.  Output dimensions are covered by NF = ceil(DP / 16) MFMA tiles
// (LDS tiles are zero-filled up to 16 NF columns); contractions over the head dimension take exactly DP / 4 k-steps.
// No atomics, fixed summation orders: bit-identical from run to run.
#include "gt_common.h"

namespace gt {

constexpr int CA_C = 64;         // tokens per chunk

template <int KS> struct CaShape {
    static constexpr int DP = 4 * KS, NF = (DP + 15) / 16, LD = 16 * NF + 4, SZ = DP * DP + DP;
};

__device__ __forceinline__ f32x4 ca_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Rows [t0, t0 + 64) of one head's tile -> LDS image [64][LD], each row times scale(t); a zero scale, rows at or beyond n and
// the columns DP .. 16 NF - 1 give exact zeros.  `src` points at (sample, token 0, head).
template <int KS, typename F>
__device__ __forceinline__ void ca_load_tile(float* lds, const float* __restrict__ src, int64_t hD, int t0, int n, F scale) {
    constexpr int GR = 4 * CaShape<KS>::NF, LD = CaShape<KS>::LD;
    for (int e = threadIdx.x; e < CA_C * GR; e += 256) {
        const int r = e / GR, g = e % GR, t = t0 + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (g < KS && t < n) {
            const float s = scale(t);
            if (s != 0.f) v = *reinterpret_cast<const f32x4*>(src + (int64_t)t * hD + 4 * g) * s;
        }
        *reinterpret_cast<f32x4*>(lds + r * LD + 4 * g) = v;
    }
}

// c[b, head, t] = -(dout_t . out_t) / den_t: 16 lanes per tile row, four rows per wave
__global__ __launch_bounds__(256) void causal_rowdot(const float* __restrict__ dO, const float* __restrict__ O,
                                                     const float* __restrict__ den, float* __restrict__ c, int64_t rows,
                                                     int n, int h, int KS) {
    const int l16 = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);      // (b n + t) h + head
    const int64_t rc = row < rows ? row : rows - 1;
    float s = 0.f;
    for (int g = l16; g < KS; g += 16) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(dO + rc * (4 * KS) + 4 * g);
        const f32x4 b = *reinterpret_cast<const f32x4*>(O + rc * (4 * KS) + 4 * g);
        s += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l16 == 0 && row < rows) {
        const int head = (int)(row % h);
        const int64_t bt = row / h, b = bt / n, t = bt % n;
        const int64_t i = (b * h + head) * n + t;
        c[i] = -s / den[i];
    }
}

// Stage 1.  Forward: chunks 0 .. nchunk-2 (the last one has no successor), X = K^, Y = V^.  Backward: chunks 1 .. nchunk-1,
// X = Q, Y = G = dout / den, weights c.  Writes [X^T Y | sum_t w_t x_t] of chunk c at states[(bh nchunk + c) SZ].
template <int KS, bool BWD>
__global__ __launch_bounds__(256) void causal_chunk_sums(const float* __restrict__ X, const float* __restrict__ Y,
                                                         const uint8_t* __restrict__ keep, const float* __restrict__ den,
                                                         const float* __restrict__ cvec, float* __restrict__ states, int n,
                                                         int h, int nchunk, float inv_n) {
    using S = CaShape<KS>;
    constexpr int DP = S::DP, NF = S::NF, LD = S::LD;
    __shared__ __attribute__((aligned(16))) float xt[CA_C * LD];
    __shared__ __attribute__((aligned(16))) float yt[CA_C * LD];
    __shared__ float wl[CA_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x + (BWD ? 1 : 0), head = blockIdx.y, b = blockIdx.z;
    const int t0 = chunk * CA_C;
    const int64_t hD = (int64_t)h * DP, base = (int64_t)b * n * hD + (int64_t)head * DP;
    const int64_t bh = (int64_t)b * h + head;
    if (BWD) {
        const float* dn = den + bh * n;
        ca_load_tile<KS>(xt, X + base, hD, t0, n, [](int) { return 1.f; });
        ca_load_tile<KS>(yt, Y + base, hD, t0, n, [dn](int t) { return 1.f / dn[t]; });
        if (tid < CA_C) wl[tid] = t0 + tid < n ? cvec[bh * n + t0 + tid] : 0.f;
    } else {
        const uint8_t* kp = keep ? keep + (int64_t)b * n : nullptr;
        ca_load_tile<KS>(xt, X + base, hD, t0, n, [kp, inv_n](int t) { return (!kp || kp[t]) ? inv_n : 0.f; });
        ca_load_tile<KS>(yt, Y + base, hD, t0, n, [kp](int t) { return (!kp || kp[t]) ? 1.f : 0.f; });
        if (tid < CA_C) wl[tid] = 1.f;
    }
    __syncthreads();
    float* out = states + (bh * nchunk + chunk) * (int64_t)S::SZ;
    for (int tile = wave; tile < NF * NF; tile += 4) {
        const int mt = tile / NF, nt = tile % NF;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CA_C / 4; ++s) {
            const int t = 4 * s + kq;
            acc = ca_mfma(xt[t * LD + 16 * mt + j], yt[t * LD + 16 * nt + j], acc);
        }
        const int e = 16 * nt + j;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * mt + 4 * kq + r;
            if (d < DP && e < DP) out[d * DP + e] = acc[r];
        }
    }
    if (tid < DP) {
        float s = 0.f;
        for (int t = 0; t < CA_C; ++t) s += wl[t] * xt[t * LD + tid];
        out[DP * DP + tid] = s;
    }
}

// Stage 2: exclusive scan over the chunks of each (sample, head), in place, one thread per state element.  Forward order
// reads the sums of chunks 0 .. nchunk-2, reverse order those of chunks nchunk-1 .. 1 (what stage 1 wrote).
template <bool REVERSE>
__global__ __launch_bounds__(256) void causal_scan(float* __restrict__ states, int nchunk, int SZ, int nb) {
    const int64_t bh = blockIdx.x / nb;
    const int e = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (e >= SZ) return;
    float* p = states + bh * nchunk * (int64_t)SZ + e;
    float run = 0.f;
    for (int i = 0; i < nchunk; ++i) {
        const int c = REVERSE ? nchunk - 1 - i : i;
        const float v = i + 1 < nchunk ? p[(int64_t)c * SZ] : 0.f;
        p[(int64_t)c * SZ] = run;
        run += v;
    }
}

// Stage 3, forward.  Stream tiles K^, V^ of the chunk in LDS; owner rows: 16 queries per wave.
template <int KS>
__global__ __launch_bounds__(256) void causal_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                         const float* __restrict__ V, const uint8_t* __restrict__ keep,
                                                         const float* __restrict__ states, float* __restrict__ O,
                                                         float* __restrict__ den, int n, int h, int nchunk, float inv_n,
                                                         float eps) {
    using S = CaShape<KS>;
    constexpr int DP = S::DP, NF = S::NF, LD = S::LD;
    __shared__ __attribute__((aligned(16))) float kt[CA_C * LD];
    __shared__ __attribute__((aligned(16))) float vt[CA_C * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int t0 = chunk * CA_C;
    const int64_t hD = (int64_t)h * DP, base = (int64_t)b * n * hD + (int64_t)head * DP;
    const int64_t bh = (int64_t)b * h + head;
    const uint8_t* kp = keep ? keep + (int64_t)b * n : nullptr;
    ca_load_tile<KS>(kt, K + base, hD, t0, n, [kp, inv_n](int t) { return (!kp || kp[t]) ? inv_n : 0.f; });
    ca_load_tile<KS>(vt, V + base, hD, t0, n, [kp](int t) { return (!kp || kp[t]) ? 1.f : 0.f; });

    const float* sp = states + (bh * nchunk + chunk) * (int64_t)S::SZ;
    const float* zp = sp + DP * DP;
    const int o = t0 + 16 * wave + j, oc = min(o, n - 1);
    const bool live = o < n;
    float fq[KS];
    float dn = 0.f;          // den: the z_prev part, then the chunk's own row sum
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        fq[s] = live ? Q[base + (int64_t)oc * hD + 4 * s + kq] : 0.f;
        dn += fq[s] * (zp[4 * s + kq] + eps);
    }
    __syncthreads();

    // A^T tiles (key 16mt + 4kq + r, query 16 wave + j), keys of tiles mt <= wave only
    f32x4 sa[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        sa[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mt <= wave) {
#pragma unroll
            for (int s = 0; s < KS; ++s) sa[mt] = ca_mfma(kt[(16 * mt + j) * LD + 4 * s + kq], fq[s], sa[mt]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * mt + 4 * kq + r > 16 * wave + j) sa[mt][r] = 0.f;
                dn += sa[mt][r];
            }
        }
    }
    dn += __shfl_xor(dn, 16, 64);
    dn += __shfl_xor(dn, 32, 64);

    // num^T (dims x queries) = S_prev^T Q_c^T + V^_c^T A^T
    f32x4 acc[NF];
#pragma unroll
    for (int dt = 0; dt < NF; ++dt) {
        acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int e = 16 * dt + j;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc[dt] = ca_mfma(e < DP ? sp[(4 * s + kq) * DP + e] : 0.f, fq[s], acc[dt]);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
        if (mt <= wave) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = 16 * mt + 4 * kq + s;
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) acc[dt] = ca_mfma(vt[row * LD + 16 * dt + j], sa[mt][s], acc[dt]);
            }
        }
    if (!live) return;
    const float rinv = 1.f / dn;
#pragma unroll
    for (int dt = 0; dt < NF; ++dt) {
        const int dim = 16 * dt + 4 * kq;
        if (dim < DP) *reinterpret_cast<f32x4*>(O + base + (int64_t)o * hD + dim) = acc[dt] * rinv;
    }
    if (kq == 0) den[bh * n + o] = dn;
}

// Stage 3, backward, d/dQ'.  Stream tiles K^, V^; owner rows: 16 queries per wave with g = dout / den and c.
template <int KS>
__global__ __launch_bounds__(256) void causal_bwd_q_kernel(const float* __restrict__ dO, const float* __restrict__ K,
                                                           const float* __restrict__ V, const uint8_t* __restrict__ keep,
                                                           const float* __restrict__ den, const float* __restrict__ cvec,
                                                           const float* __restrict__ states, float* __restrict__ dQ, int n,
                                                           int h, int nchunk, int Dr, float inv_n, float eps) {
    using S = CaShape<KS>;
    constexpr int DP = S::DP, NF = S::NF, LD = S::LD;
    __shared__ __attribute__((aligned(16))) float kt[CA_C * LD];
    __shared__ __attribute__((aligned(16))) float vt[CA_C * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int t0 = chunk * CA_C;
    const int64_t hD = (int64_t)h * DP, base = (int64_t)b * n * hD + (int64_t)head * DP;
    const int64_t bh = (int64_t)b * h + head;
    const uint8_t* kp = keep ? keep + (int64_t)b * n : nullptr;
    ca_load_tile<KS>(kt, K + base, hD, t0, n, [kp, inv_n](int t) { return (!kp || kp[t]) ? inv_n : 0.f; });
    ca_load_tile<KS>(vt, V + base, hD, t0, n, [kp](int t) { return (!kp || kp[t]) ? 1.f : 0.f; });

    const float* sp = states + (bh * nchunk + chunk) * (int64_t)S::SZ;
    const float* zp = sp + DP * DP;
    const int o = t0 + 16 * wave + j, oc = min(o, n - 1);
    const bool live = o < n;
    const float rden = live ? 1.f / den[bh * n + oc] : 0.f;
    const float cq = live ? cvec[bh * n + oc] : 0.f;
    float fg[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) fg[s] = live ? dO[base + (int64_t)oc * hD + 4 * s + kq] * rden : 0.f;
    __syncthreads();

    // W^T tiles (key 16mt + 4kq + r, query 16 wave + j) = tril(g . v^ + c)
    f32x4 sa[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        sa[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mt <= wave) {
#pragma unroll
            for (int s = 0; s < KS; ++s) sa[mt] = ca_mfma(vt[(16 * mt + j) * LD + 4 * s + kq], fg[s], sa[mt]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sa[mt][r] = (16 * mt + 4 * kq + r > 16 * wave + j) ? 0.f : sa[mt][r] + cq;
        }
    }
    // dQ'^T (dims x queries) = S_prev G_c^T + K^_c^T W^T
    f32x4 acc[NF];
#pragma unroll
    for (int dt = 0; dt < NF; ++dt) {
        acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int d = 16 * dt + j;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc[dt] = ca_mfma(d < DP ? sp[d * DP + 4 * s + kq] : 0.f, fg[s], acc[dt]);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
        if (mt <= wave) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = 16 * mt + 4 * kq + s;
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) acc[dt] = ca_mfma(kt[row * LD + 16 * dt + j], sa[mt][s], acc[dt]);
            }
        }
    if (!live) return;
#pragma unroll
    for (int dt = 0; dt < NF; ++dt) {
        const int dim = 16 * dt + 4 * kq;
        if (dim < DP) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = dim + r < Dr ? acc[dt][r] + cq * (zp[dim + r] + eps) : 0.f;
            *reinterpret_cast<f32x4*>(dQ + base + (int64_t)o * hD + dim) = v;
        }
    }
}

// Stage 3, backward, d/dK' and d/dV'.  Stream tiles Q, G = dout / den (and c) of the chunk; owner rows: 16 keys per wave.
template <int KS>
__global__ __launch_bounds__(256) void causal_bwd_kv_kernel(const float* __restrict__ dO, const float* __restrict__ Q,
                                                            const float* __restrict__ K, const float* __restrict__ V,
                                                            const uint8_t* __restrict__ keep, const float* __restrict__ den,
                                                            const float* __restrict__ cvec, const float* __restrict__ rstates,
                                                            float* __restrict__ dK, float* __restrict__ dV, int n, int h,
                                                            int nchunk, int Dr, float inv_n) {
    using S = CaShape<KS>;
    constexpr int DP = S::DP, NF = S::NF, LD = S::LD;
    __shared__ __attribute__((aligned(16))) float qt[CA_C * LD];
    __shared__ __attribute__((aligned(16))) float gt_[CA_C * LD];
    __shared__ float cl[CA_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int t0 = chunk * CA_C;
    const int64_t hD = (int64_t)h * DP, base = (int64_t)b * n * hD + (int64_t)head * DP;
    const int64_t bh = (int64_t)b * h + head;
    const float* dn = den + bh * n;
    ca_load_tile<KS>(qt, Q + base, hD, t0, n, [](int) { return 1.f; });
    ca_load_tile<KS>(gt_, dO + base, hD, t0, n, [dn](int t) { return 1.f / dn[t]; });
    if (tid < CA_C) cl[tid] = t0 + tid < n ? cvec[bh * n + t0 + tid] : 0.f;

    const float* rp = rstates + (bh * nchunk + chunk) * (int64_t)S::SZ;
    const float* rv = rp + DP * DP;
    const int o = t0 + 16 * wave + j, oc = min(o, n - 1);
    const bool live = o < n && (!keep || keep[(int64_t)b * n + oc]);      // a dropped key: k^ = v^ = 0, zero gradients
    float fk[KS], fv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        fk[s] = live ? K[base + (int64_t)oc * hD + 4 * s + kq] * inv_n : 0.f;
        fv[s] = live ? V[base + (int64_t)oc * hD + 4 * s + kq] : 0.f;
    }
    __syncthreads();

    // W and A tiles (query 16mt + 4kq + r, key 16 wave + j), queries of tiles mt >= wave only
    f32x4 sa[4], sb[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        sa[mt] = sb[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mt >= wave) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                sa[mt] = ca_mfma(gt_[(16 * mt + j) * LD + 4 * s + kq], fv[s], sa[mt]);
                sb[mt] = ca_mfma(qt[(16 * mt + j) * LD + 4 * s + kq], fk[s], sb[mt]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = 16 * mt + 4 * kq + r;
                const bool on = qi >= 16 * wave + j;
                sa[mt][r] = on ? sa[mt][r] + cl[qi] : 0.f;
                sb[mt][r] = on ? sb[mt][r] : 0.f;
            }
        }
    }
    // dK^^T (dims x keys) = R_next V^_c^T + Q_c^T W,   dV^^T = R_next^T K^_c^T + G_c^T A
    f32x4 ack[NF], acv[NF];
#pragma unroll
    for (int dt = 0; dt < NF; ++dt) {
        ack[dt] = acv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int d = 16 * dt + j;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            ack[dt] = ca_mfma(d < DP ? rp[d * DP + 4 * s + kq] : 0.f, fv[s], ack[dt]);
            acv[dt] = ca_mfma(d < DP ? rp[(4 * s + kq) * DP + d] : 0.f, fk[s], acv[dt]);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
        if (mt >= wave) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = 16 * mt + 4 * kq + s;
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) {
                    ack[dt] = ca_mfma(qt[row * LD + 16 * dt + j], sa[mt][s], ack[dt]);
                    acv[dt] = ca_mfma(gt_[row * LD + 16 * dt + j], sb[mt][s], acv[dt]);
                }
            }
        }
    if (o >= n) return;
#pragma unroll
    for (int dt = 0; dt < NF; ++dt) {
        const int dim = 16 * dt + 4 * kq;
        if (dim < DP) {
            f32x4 vk, vv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool on = live && dim + r < Dr;
                vk[r] = on ? (ack[dt][r] + rv[dim + r]) * inv_n : 0.f;
                vv[r] = on ? acv[dt][r] : 0.f;
            }
            *reinterpret_cast<f32x4*>(dK + base + (int64_t)o * hD + dim) = vk;
            *reinterpret_cast<f32x4*>(dV + base + (int64_t)o * hD + dim) = vv;
        }
    }
}

static bool ca_width(int DP) {
    switch (DP) {
        case 16: case 32: case 48: case 64: case 96:
        case 20: case 36: case 52: case 68: case 100: return true;
        default: return false;
    }
}

// one instance per supported width: never the nearest one
#define GT_CA_DISPATCH(DP, CALL)                \
    switch (DP) {                               \
        case 16: { CALL(4); } break;            \
        case 20: { CALL(5); } break;            \
        case 32: { CALL(8); } break;            \
        case 36: { CALL(9); } break;            \
        case 48: { CALL(12); } break;           \
        case 52: { CALL(13); } break;           \
        case 64: { CALL(16); } break;           \
        case 68: { CALL(17); } break;           \
        case 96: { CALL(24); } break;           \
        case 100: { CALL(25); } break;          \
        default: return GT_ENOTSUP;             \
    }

static int ca_check(int32_t B, int32_t n, int32_t h, int32_t DP) {
    if (B <= 0 || n <= 0 || h <= 0 || DP <= 0) return GT_EINVAL;
    if (!ca_width(DP)) return GT_ENOTSUP;
    if (B > 65535 || h > 65535) return GT_EINVAL;
    return 0;
}

static int64_t ca_state_bytes(int32_t B, int32_t n, int32_t h, int32_t DP) {
    return (int64_t)B * h * ceil_div(n, CA_C) * ((int64_t)DP * DP + DP) * 4;
}

}  // namespace gt

using namespace gt;

extern "C" int64_t gt_causal_attn_state_bytes(int32_t B, int32_t n, int32_t h, int32_t DP) {
    return ca_check(B, n, h, DP) ? 0 : ca_state_bytes(B, n, h, DP);
}

extern "C" int64_t gt_causal_attn_bwd_ws_bytes(int32_t B, int32_t n, int32_t h, int32_t DP) {
    return ca_check(B, n, h, DP) ? 0 : ca_state_bytes(B, n, h, DP) + (int64_t)B * h * n * 4;
}

extern "C" int gt_causal_attn_fwd(const float* Q, const float* K, const float* V, const uint8_t* keep, float* O, float* den,
                                  int32_t B, int32_t n, int32_t h, int32_t DP, float eps, float* states,
                                  int64_t states_bytes, void* stream) {
    if (int rc = ca_check(B, n, h, DP)) return rc;
    if (!Q || !K || !V || !O || !den || !states) return GT_EINVAL;
    if (misaligned16(Q, K, V, O)) return GT_EALIGN;
    if (misaligned<4>(den, states)) return GT_EALIGN;
    if (states_bytes < ca_state_bytes(B, n, h, DP)) return GT_EWS;
    const int nchunk = ceil_div(n, CA_C), SZ = DP * DP + DP, nb = ceil_div(SZ, 256);
    if ((int64_t)B * h * nb > 0x7fffffffLL) return GT_EINVAL;
    const float inv_n = (float)(1.0 / (double)n);
    hipStream_t st = (hipStream_t)stream;
    if (nchunk > 1) {
#define GT_CA_SUMS(KS_)                                                                                                   \
    hipLaunchKernelGGL((causal_chunk_sums<KS_, false>), dim3((unsigned)(nchunk - 1), (unsigned)h, (unsigned)B), dim3(256), 0, \
                       st, K, V, keep, (const float*)nullptr, (const float*)nullptr, states, n, h, nchunk, inv_n)
        GT_CA_DISPATCH(DP, GT_CA_SUMS)
#undef GT_CA_SUMS
        GT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((causal_scan<false>), dim3((unsigned)(B * h * nb)), dim3(256), 0, st, states, nchunk, SZ, nb);
    GT_LAUNCH_CHECK();
#define GT_CA_FWD(KS_)                                                                                                      \
    hipLaunchKernelGGL((causal_fwd_kernel<KS_>), dim3((unsigned)nchunk, (unsigned)h, (unsigned)B), dim3(256), 0, st, Q, K, V, \
                       keep, (const float*)states, O, den, n, h, nchunk, inv_n, eps)
    GT_CA_DISPATCH(DP, GT_CA_FWD)
#undef GT_CA_FWD
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_causal_attn_bwd(const float* dO, const float* O, const float* Q, const float* K, const float* V,
                                  const uint8_t* keep, const float* den, const float* states, float* dQ, float* dK,
                                  float* dV, int32_t B, int32_t n, int32_t h, int32_t DP, int32_t D, float eps, void* ws,
                                  int64_t ws_bytes, void* stream) {
    if (int rc = ca_check(B, n, h, DP)) return rc;
    if (!dO || !O || !Q || !K || !V || !den || !states || !dQ || !dK || !dV || !ws) return GT_EINVAL;
    if (D <= 0 || D > DP) return GT_EINVAL;
    if (misaligned16(dO, O, Q, K, V, dQ, dK, dV)) return GT_EALIGN;
    if (misaligned<4>(den, states) || misaligned<4>((const float*)ws)) return GT_EALIGN;
    const int64_t sbytes = ca_state_bytes(B, n, h, DP);
    if (ws_bytes < sbytes + (int64_t)B * h * n * 4) return GT_EWS;
    const int nchunk = ceil_div(n, CA_C), SZ = DP * DP + DP, nb = ceil_div(SZ, 256);
    const int64_t rows = (int64_t)B * n * h;
    if ((int64_t)B * h * nb > 0x7fffffffLL || (rows + 15) / 16 > 0x7fffffffLL) return GT_EINVAL;
    const float inv_n = (float)(1.0 / (double)n);
    float* rstates = (float*)ws;
    float* cvec = rstates + sbytes / 4;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(causal_rowdot, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, dO, O, den, cvec, rows, n, h,
                       DP / 4);
    GT_LAUNCH_CHECK();
    if (nchunk > 1) {
#define GT_CA_SUMS(KS_)                                                                                                  \
    hipLaunchKernelGGL((causal_chunk_sums<KS_, true>), dim3((unsigned)(nchunk - 1), (unsigned)h, (unsigned)B), dim3(256), 0, \
                       st, Q, dO, (const uint8_t*)nullptr, den, (const float*)cvec, rstates, n, h, nchunk, inv_n)
        GT_CA_DISPATCH(DP, GT_CA_SUMS)
#undef GT_CA_SUMS
        GT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((causal_scan<true>), dim3((unsigned)(B * h * nb)), dim3(256), 0, st, rstates, nchunk, SZ, nb);
    GT_LAUNCH_CHECK();
#define GT_CA_BQ(KS_)                                                                                                        \
    hipLaunchKernelGGL((causal_bwd_q_kernel<KS_>), dim3((unsigned)nchunk, (unsigned)h, (unsigned)B), dim3(256), 0, st, dO, K, \
                       V, keep, den, (const float*)cvec, states, dQ, n, h, nchunk, D, inv_n, eps)
    GT_CA_DISPATCH(DP, GT_CA_BQ)
#undef GT_CA_BQ
    GT_LAUNCH_CHECK();
#define GT_CA_BKV(KS_)                                                                                                        \
    hipLaunchKernelGGL((causal_bwd_kv_kernel<KS_>), dim3((unsigned)nchunk, (unsigned)h, (unsigned)B), dim3(256), 0, st, dO, Q, \
                       K, V, keep, den, (const float*)cvec, (const float*)rstates, dK, dV, n, h, nchunk, D, inv_n)
    GT_CA_DISPATCH(DP, GT_CA_BKV)
#undef GT_CA_BKV
    GT_LAUNCH_CHECK();
    return 0;
}
