// Random-feature attention (Performer 'favor' / random Fourier features 'rfa'), one head of width d, m = d features, in fp32:
//
//     u(z) = (s z) Om                 s = d^(-1/4),  Om [d][m/2]
//     rfa  : phi(z) = sqrt(2/m) [cos u, sin u]            favor: phi(z) = [exp(u - c), exp(-u - c)],  c = |s z|^2 / 2 + log(m) / 2
//     KVa  = phi(K)^T [V, 1]          [m][d + 4]: KV, the column sums of phi(K) in column d, three zero columns
//     out  = phi(Q) KVa[:, :d] / den, den = phi(Q) . KVa[:, d] + eps
//
// phi and u live in registers only.  A wave owns 16 tokens.  Both products of a pass run on v_mfma_f32_16x16x4_f32, and the
// result of the first (u, then phi after the VALU feature map) is the B operand of the second from the same lane's
// accumulator registers, the hand-over of gt_softmax.hip: register r of lane (j, kq) of a D tile is element (row 4kq + r,
// column j), which is exactly what k-step r of the next product wants from that lane if the contraction runs over the ROWS.
// So the first product is issued in the orientation the second one contracts over:
//
//     "T" tiles  uT = Om^T z^T   rows = features, column = token j    -> contraction over features:  phi(q) KVa, dQ, dV
//     "N" tiles  u  = z Om       rows = tokens,   column = feature j  -> contraction over tokens:    phi^T [V, 1], phi^T G
//
// from the same operand registers (A and B swapped).  The k index of the first product is free as long as both operands
// agree: lane (j, kq) loads z[token j][16 s + 4 kq .. + 3] as one float4 and pairs element c with Om row 16 s + 4 kq + c.
//
//   pass     streams        resident (LDS)   products
//   kv       K, V           Om               N: u -> phi;  KVa^T += V^T phi           (slab per block, fixed-order merge)
//   q        Q              Om, KVa          T: u -> phi;  out^T = KVa^T phi^T, den
//   bwd_q    Q, dOut, out   Om, KVa          T: phi, dphi = KVa G^T -> du -> dQ^T = Om du^T;   N: phi;  dKVa^T += G^T phi
//   bwd_kv   K, V           Om, dKVa         T: phi, dphi = dKVa [V,1]^T -> du -> dK^T;  dV^T = dKVa^T phi^T
//
// with G = [dOut / den, -(dOut . out) / den].  Rows at or beyond n are loaded from row n - 1 (a valid address), their phi in
// the N tiles is set to zero (exp(-c) and cos 0 of a zero row are not zero), and nothing of theirs is stored.
// No atomics: the four waves of a block are summed through LDS in wave order, the blocks' slabs by gt_slab_reduce.
#include "gt_common.h"
#include <cmath>

namespace gt {

enum { RF_KV = 0, RF_Q = 1, RF_BWDQ = 2, RF_BWDKV = 3 };
constexpr int RF_CHUNK = 256;        // tokens per block: 4 waves x 16 tokens x 4 trips
constexpr int RF_TRIPS = RF_CHUNK / 64;

struct RfP {
    const float* X;          // Q (q, bwd_q) or K (kv, bwd_kv): column block of a [B*n][ld] matrix
    const float* V;          // kv, bwd_kv
    const float* omega;      // [d][d/2]
    const float* M;          // KVa (q, bwd_q) or dKVa (bwd_kv): [B][d][d+4]
    const float* dOut;       // bwd_q: [B*n][d]
    const float* outp;       // bwd_q: the forward's out [B*n][d]
    const float* den;        // bwd_q: [B*n]
    float* O;                // q: out [B*n][d];  bwd_q: dQ, bwd_kv: dK  (column block of [B*n][ldg])
    float* O2;               // q: den [B*n];  bwd_kv: dV
    float* slab;             // kv, bwd_q: [chunks][B][d][d+4]
    int64_t ld, ldg;
    int n, B;
    float eps;
};

__device__ __forceinline__ f32x4 rf_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float rf_sum_kq(float v) {          // sum over the four kq groups of a column j
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// The feature map on one D tile of u: lo = first half of phi (cos / exp(u - c)), hi = second half (sin / exp(-u - c)).
// sincosf / expf are the accurate library routines (range reduction included): |u| reaches tens once the weights have moved.
template <bool FAVOR>
__device__ __forceinline__ f32x2 rf_phi(float u, float c, float amp) {
    if (FAVOR) return f32x2{expf(u - c), expf(-u - c)};
    float sn, cs;
    sincosf(u, &sn, &cs);
    return f32x2{amp * cs, amp * sn};
}

template <int D, int PASS, bool FAVOR>
__global__ __launch_bounds__(256) void rfattn_kernel(const RfP p) {
    constexpr int HF = D / 2, NU = HF / 16, NF = D / 16, KS = D / 16, HP = HF + 4, DP = D + 4;
    constexpr bool ACC = PASS == RF_KV || PASS == RF_BWDQ;         // accumulates a [d][d+4] slab over its tokens
    constexpr bool TT = PASS != RF_KV, NN = ACC;                   // which orientations of u it needs
    constexpr bool BWD = PASS == RF_BWDQ || PASS == RF_BWDKV;
    __shared__ __attribute__((aligned(16))) float om[D * HP];
    __shared__ __attribute__((aligned(16))) float mm[D * DP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const float sc = powf((float)D, -0.25f);
    const float amp = sqrtf(2.f / (float)D), half_log_m = 0.5f * logf((float)D);

    for (int i = tid; i < D * HF; i += 256) om[(i / HF) * HP + i % HF] = p.omega[i];
    for (int i = tid; i < D; i += 256) om[i * HP + HF] = om[i * HP + HF + 1] = om[i * HP + HF + 2] = om[i * HP + HF + 3] = 0.f;
    if constexpr (PASS != RF_KV) {
        const f32x4* src = reinterpret_cast<const f32x4*>(p.M + (int64_t)b * D * DP);
        for (int i = tid; i < D * DP / 4; i += 256) reinterpret_cast<f32x4*>(mm)[i] = src[i];
    }
    __syncthreads();

    f32x4 acc[ACC ? NF : 1][ACC ? NF : 1];       // [dim tile][feature tile]: (feature 16 f + j, dims 16 dt + 4 kq + r)
    float ks[ACC ? NF : 1];                      // column d of the slab: partial over kq
#pragma unroll
    for (int a = 0; a < (ACC ? NF : 1); ++a) {
        ks[a] = 0.f;
#pragma unroll
        for (int f = 0; f < (ACC ? NF : 1); ++f) acc[a][f] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int trip = 0; trip < RF_TRIPS; ++trip) {
        const int tok0 = chunk * RF_CHUNK + trip * 64 + wave * 16;
        if (tok0 >= p.n) break;                              // wave-uniform; no barrier inside the loop
        const int tj = tok0 + j;                             // this lane's token as a column (T tiles, operand loads)
        const int64_t rowj = (int64_t)b * p.n + min(tj, p.n - 1);
        // z = s x, lane (j, kq): elements 16 s + 4 kq + c of token j
        f32x4 xs[KS];
        float cj = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xs[s] = *reinterpret_cast<const f32x4*>(p.X + rowj * p.ld + 16 * s + 4 * kq) * sc;
#pragma unroll
            for (int c = 0; c < 4; ++c) cj += xs[s][c] * xs[s][c];
        }
        cj = 0.5f * rf_sum_kq(cj) + half_log_m;              // favor's offset c of token j
        // second streamed operand by token j: G[:, :d] = dOut / den (bwd_q), V (bwd_kv); and the last column of [.., 1] / G
        f32x4 yr[BWD ? KS : 1];
        float lastj = 1.f, rdenj = 1.f;
        if constexpr (PASS == RF_BWDQ) {
            rdenj = 1.f / p.den[rowj];
            float dot = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                yr[s] = *reinterpret_cast<const f32x4*>(p.dOut + rowj * D + 16 * s + 4 * kq) * rdenj;
                const f32x4 o = *reinterpret_cast<const f32x4*>(p.outp + rowj * D + 16 * s + 4 * kq);
#pragma unroll
                for (int c = 0; c < 4; ++c) dot += yr[s][c] * o[c];
            }
            lastj = -rf_sum_kq(dot);
        } else if constexpr (PASS == RF_BWDKV) {
#pragma unroll
            for (int s = 0; s < KS; ++s) yr[s] = *reinterpret_cast<const f32x4*>(p.V + rowj * p.ld + 16 * s + 4 * kq);
        }

        // ------------------------------------------------------------------ T tiles: phi[token j][feature 16 f + 4 kq + r]
        f32x4 pt[TT ? NF : 1];
        if constexpr (TT) {
#pragma unroll
            for (int ft = 0; ft < NU; ++ft) {
                f32x4 u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int c = 0; c < 4; ++c) u = rf_mfma(om[(16 * s + 4 * kq + c) * HP + 16 * ft + j], xs[s][c], u);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x2 ph = rf_phi<FAVOR>(u[r], cj, amp);
                    pt[ft][r] = ph[0];
                    pt[NU + ft][r] = ph[1];
                }
            }
        }
        // ------------------------------------------------------------------ N tiles: phi[token 4 kq + r][feature 16 f + j]
        if constexpr (NN) {
            f32x4 pn[NF];
            float c4[4], last4[4], rden4[4];
            int64_t row4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                c4[r] = __shfl(cj, 4 * kq + r, 64);
                last4[r] = __shfl(lastj, 4 * kq + r, 64);
                rden4[r] = __shfl(rdenj, 4 * kq + r, 64);
                row4[r] = (int64_t)b * p.n + min(tok0 + 4 * kq + r, p.n - 1);
            }
#pragma unroll
            for (int ft = 0; ft < NU; ++ft) {
                f32x4 u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int c = 0; c < 4; ++c) u = rf_mfma(xs[s][c], om[(16 * s + 4 * kq + c) * HP + 16 * ft + j], u);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x2 ph = rf_phi<FAVOR>(u[r], c4[r], amp);
                    const bool live = tok0 + 4 * kq + r < p.n;                          // rows beyond n contribute nothing
                    pn[ft][r] = live ? ph[0] : 0.f;
                    pn[NU + ft][r] = live ? ph[1] : 0.f;
                }
            }
            // slab^T (dims x features) += Y^T (dims x tokens) phi (tokens x features), Y = V (kv) or dOut / den (bwd_q)
            const float* Y = PASS == RF_KV ? p.V : p.dOut;
            const int64_t ldy = PASS == RF_KV ? p.ld : (int64_t)D;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) {
                    float a = Y[row4[r] * ldy + 16 * dt + j];
                    if (PASS == RF_BWDQ) a *= rden4[r];
#pragma unroll
                    for (int f = 0; f < NF; ++f) acc[dt][f] = rf_mfma(a, pn[f][r], acc[dt][f]);
                }
#pragma unroll
                for (int f = 0; f < NF; ++f) ks[f] += pn[f][r] * last4[r];
            }
        }
        if constexpr (PASS == RF_Q || PASS == RF_BWDKV) {
            // out^T (dims x tokens) = M^T (dims x features) phi^T (features x tokens)
            f32x4 o[NF];
#pragma unroll
            for (int dt = 0; dt < NF; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            float den = 0.f;
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* mrow = &mm[(16 * f + 4 * kq + r) * DP];
#pragma unroll
                    for (int dt = 0; dt < NF; ++dt) o[dt] = rf_mfma(mrow[16 * dt + j], pt[f][r], o[dt]);
                    if (PASS == RF_Q) den += pt[f][r] * mrow[D];
                }
            float rd = 1.f;
            if (PASS == RF_Q) {
                den = rf_sum_kq(den) + p.eps;
                rd = 1.f / den;
            }
            if (tj < p.n) {
                float* dst = PASS == RF_Q ? p.O + rowj * D : p.O2 + rowj * p.ldg;
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) *reinterpret_cast<f32x4*>(dst + 16 * dt + 4 * kq) = o[dt] * rd;
                if (PASS == RF_Q && kq == 0) p.O2[rowj] = den;
            }
        }
        if constexpr (BWD) {
            // dphi^T (features x tokens) = M (features x dims) Y^T (dims x tokens) + M[:, d] last^T
            f32x4 du[NU];
            float e = 0.f;
#pragma unroll
            for (int ft = 0; ft < NU; ++ft) {
                f32x4 dlo = {0.f, 0.f, 0.f, 0.f}, dhi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const f32x4 alo = *reinterpret_cast<const f32x4*>(&mm[(16 * ft + j) * DP + 16 * s + 4 * kq]);
                    const f32x4 ahi = *reinterpret_cast<const f32x4*>(&mm[(16 * (NU + ft) + j) * DP + 16 * s + 4 * kq]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        dlo = rf_mfma(alo[c], yr[s][c], dlo);
                        dhi = rf_mfma(ahi[c], yr[s][c], dhi);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dlo[r] += lastj * mm[(16 * ft + 4 * kq + r) * DP + D];
                    dhi[r] += lastj * mm[(16 * (NU + ft) + 4 * kq + r) * DP + D];
                    const float lo = pt[ft][r], hi = pt[NU + ft][r];
                    if (FAVOR) {
                        du[ft][r] = lo * dlo[r] - hi * dhi[r];      // phi+ dphi+ - phi- dphi-
                        e += lo * dlo[r] + hi * dhi[r];
                    } else {
                        du[ft][r] = lo * dhi[r] - hi * dlo[r];      // phi_c dphi_s - phi_s dphi_c
                    }
                }
            }
            if (FAVOR) e = rf_sum_kq(e);
            // dz^T (dims x tokens) = Om (dims x half-features) du^T;  dx = s dz - (phi . dphi) s z   (favor)
#pragma unroll
            for (int dt = 0; dt < NF; ++dt) {
                f32x4 dz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ft = 0; ft < NU; ++ft)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dz = rf_mfma(om[(16 * dt + j) * HP + 16 * ft + 4 * kq + r], du[ft][r], dz);
                f32x4 dx = dz * sc;
                if (FAVOR) dx -= xs[dt] * (e * sc);
                if (tj < p.n) *reinterpret_cast<f32x4*>(p.O + rowj * p.ldg + 16 * dt + 4 * kq) = dx;
            }
        }
    }

    if constexpr (ACC) {
        // the four waves in wave order through LDS (bwd_q: everybody is done reading KVa first), then one slab per block
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    float* row = &mm[(16 * f + j) * DP];
#pragma unroll
                    for (int dt = 0; dt < NF; ++dt) {
                        f32x4* q = reinterpret_cast<f32x4*>(row + 16 * dt + 4 * kq);
                        *q = w == 0 ? acc[dt][f] : *q + acc[dt][f];
                    }
                    const float col = rf_sum_kq(ks[f]);
                    if (kq == 0) {
                        f32x4* q = reinterpret_cast<f32x4*>(row + D);
                        *q = w == 0 ? f32x4{col, 0.f, 0.f, 0.f} : *q + f32x4{col, 0.f, 0.f, 0.f};
                    }
                }
            }
            __syncthreads();
        }
        f32x4* dst = reinterpret_cast<f32x4*>(p.slab + ((int64_t)chunk * p.B + b) * D * DP);
        for (int i = tid; i < D * DP / 4; i += 256) dst[i] = reinterpret_cast<const f32x4*>(mm)[i];
    }
}

static inline int rf_chunks(int n) { return (n + RF_CHUNK - 1) / RF_CHUNK; }
static inline bool rf_width_ok(int d) { return d == 32 || d == 64 || d == 96; }
static inline int64_t rf_slab_bytes(int B, int n, int d) { return (int64_t)rf_chunks(n) * B * d * (d + 4) * 4; }

template <int D, int PASS>
static void rf_launch_kind(const RfP& p, int kind, dim3 grid, hipStream_t st) {
    if (kind == GT_RFATTN_FAVOR) hipLaunchKernelGGL((rfattn_kernel<D, PASS, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((rfattn_kernel<D, PASS, false>), grid, dim3(256), 0, st, p);
}

// Shared argument checks and the launch; `fin` (kv, bwd_q): where the merged [B][d][d+4] result goes.
template <int PASS>
static int rf_run(RfP p, int32_t d, int32_t kind, float* fin, void* ws, int64_t ws_bytes, void* stream) {
    if (!p.X || !p.omega || p.B <= 0 || p.n <= 0 || d <= 0) return GT_EINVAL;
    if (kind != GT_RFATTN_RFA && kind != GT_RFATTN_FAVOR) return GT_EINVAL;
    if (!rf_width_ok(d) || p.B > 65535) return GT_ENOTSUP;
    if (p.ld < d || (p.ld & 3) || (PASS >= RF_BWDQ && (p.ldg < d || (p.ldg & 3)))) return GT_EALIGN;
    if (misaligned16(p.X, p.V, p.omega, p.M, p.dOut, p.outp, p.O, fin, ws)) return GT_EALIGN;
    if (misaligned<4>(p.den) || (PASS == RF_BWDKV ? misaligned16(p.O2) : misaligned<4>(p.O2))) return GT_EALIGN;
    const int chunks = rf_chunks(p.n);
    constexpr bool ACC = PASS == RF_KV || PASS == RF_BWDQ;
    if (ACC) {
        if (!fin) return GT_EINVAL;
        if (chunks > 1 && (!ws || ws_bytes < rf_slab_bytes(p.B, p.n, d))) return GT_EWS;
        p.slab = chunks > 1 ? static_cast<float*>(ws) : fin;
    }
    dim3 grid((unsigned)chunks, (unsigned)p.B);
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
        case 32: rf_launch_kind<32, PASS>(p, kind, grid, st); break;
        case 64: rf_launch_kind<64, PASS>(p, kind, grid, st); break;
        case 96: rf_launch_kind<96, PASS>(p, kind, grid, st); break;
    }
    GT_LAUNCH_CHECK();
    if (ACC && chunks > 1) {
        const int64_t sz = (int64_t)p.B * d * (d + 4);
        return gt_slab_reduce(p.slab, sz, chunks, sz, 1.f, fin, stream);
    }
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" int32_t gt_rfattn_slabs(int32_t n) { return n > 0 ? rf_chunks(n) : 0; }

extern "C" int64_t gt_rfattn_ws_bytes(int32_t B, int32_t n, int32_t d) {
    if (B <= 0 || n <= 0 || !rf_width_ok(d)) return 0;
    return rf_chunks(n) > 1 ? rf_slab_bytes(B, n, d) : 0;
}

extern "C" int gt_rfattn_kv(const float* K, const float* V, int64_t ld, const float* omega, float* KVa, int32_t B, int32_t n,
                            int32_t d, int32_t kind, void* ws, int64_t ws_bytes, void* stream) {
    if (!V) return GT_EINVAL;
    RfP p{K, V, omega, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ld, 0, n, B, 0.f};
    return rf_run<RF_KV>(p, d, kind, KVa, ws, ws_bytes, stream);
}

extern "C" int gt_rfattn_q(const float* Q, int64_t ld, const float* omega, const float* KVa, float* out, float* den, int32_t B,
                           int32_t n, int32_t d, int32_t kind, float eps, void* stream) {
    if (!KVa || !out || !den) return GT_EINVAL;
    RfP p{Q, nullptr, omega, KVa, nullptr, nullptr, nullptr, out, den, nullptr, ld, 0, n, B, eps};
    return rf_run<RF_Q>(p, d, kind, nullptr, nullptr, 0, stream);
}

extern "C" int gt_rfattn_bwd_q(const float* Q, int64_t ld, const float* omega, const float* KVa, const float* dOut,
                               const float* out, const float* den, float* dQ, int64_t ldg, float* dKVa, int32_t B, int32_t n,
                               int32_t d, int32_t kind, void* ws, int64_t ws_bytes, void* stream) {
    if (!KVa || !dOut || !out || !den || !dQ) return GT_EINVAL;
    RfP p{Q, nullptr, omega, KVa, dOut, out, den, dQ, nullptr, nullptr, ld, ldg, n, B, 0.f};
    return rf_run<RF_BWDQ>(p, d, kind, dKVa, ws, ws_bytes, stream);
}

extern "C" int gt_rfattn_bwd_kv(const float* K, const float* V, int64_t ld, const float* omega, const float* dKVa, float* dK,
                                float* dV, int64_t ldg, int32_t B, int32_t n, int32_t d, int32_t kind, void* stream) {
    if (!V || !dKVa || !dK || !dV) return GT_EINVAL;
    RfP p{K, V, omega, dKVa, nullptr, nullptr, nullptr, dK, dV, nullptr, ld, ldg, n, B, 0.f};
    return rf_run<RF_BWDKV>(p, d, kind, nullptr, nullptr, 0, stream);
}
