// Galerkin small-matrix stage of the attention (gfx950), on the head-tile layout [T][h][DP] = [pos(p) | values(dk) | pad]:
//   forward   K^T V partial slabs per token chunk (two kernels: rows straight into MFMA operands, or staged through LDS),
//             finalize: M = mask .* (sum of slabs) / n, P = M Wfc_h^T
//   backward  finalize backward (dM, dWfc slabs), dK' = V' dM^T and dV' = K' dM, alone or with the per-head LayerNorm
//             backward behind them (gt_slab_reduce sums its d(gamma), d(beta) partials), and the unpadding of dQ'
#include "gt_common.h"

namespace gt {

// ------------------------------------------------------------------------------------------ galerkin K^T V
// M[b,h] = K'^T V' over the tokens of one sample (layers.py:723), K', V' in the head-tile layout
// [T][h][DP] = [pos(p) | values(dk) | pad].  Streaming kernel: every token row is read exactly once,
// straight from HBM into MFMA operand registers (no LDS): lane (i = lane&15, k = lane>>4) of a wave holds
// K'[t0+k][p+16a+i] and V'[t0+k][p+16b+i] for 4 tokens per step, i.e. the A = K^T (16 x 4) and B = V
// (4 x 16) fragments of v_mfma_f32_16x16x4_f32.  The dk x dk core accumulates on the matrix pipe, the p-wide
// coordinate borders (P^T P, P^T V, K^T P) on the VALU beside it.  A block = 4 waves = 4 heads (looped if
// h > 4) of one token chunk of one sample; chunks write partial slabs that gt_galerkin_finalize_fwd sums.
template <int NB>
__global__ __launch_bounds__(256) void galerkin_ktv_kernel(const float* __restrict__ Kp, const float* __restrict__ Vp,
                                                           int n, int h, int DP, int p, int chunk,
                                                           float* __restrict__ slabs, int B,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, ch = blockIdx.x;
    const int t_lo = ch * chunk, t_hi = min(n, t_lo + chunk);
    const int64_t hD = (int64_t)h * DP;
    for (int head = wave; head < h; head += 4) {
        f32x4 acc[NB][NB];
        float kp[NB][2], pv[NB][2], pp[2][2];
#pragma unroll
        for (int a = 0; a < NB; ++a) {
#pragma unroll
            for (int c = 0; c < NB; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            kp[a][0] = kp[a][1] = pv[a][0] = pv[a][1] = 0.f;
        }
        pp[0][0] = pp[0][1] = pp[1][0] = pp[1][1] = 0.f;
        const float* kb = Kp + ((int64_t)b * n) * hD + (int64_t)head * DP;
        const float* vb = Vp + ((int64_t)b * n) * hD + (int64_t)head * DP;
        // "plain" head tiles (gt_hip.h: hn_plain) hold the normalised values without the LayerNorm affine: K' = gamma_K xh +
        // beta_K is formed as the operand is loaded (gamma, beta [2][h][16 NB]: K then V); NULL = tiles hold K', V'
        float gk[NB], bk[NB], gv[NB], bv[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            gk[c] = gv[c] = 1.f;
            bk[c] = bv[c] = 0.f;
            if (gamma) {
                const int o = head * 16 * NB + 16 * c + i, hd = h * 16 * NB;
                gk[c] = gamma[o]; bk[c] = beta[o]; gv[c] = gamma[hd + o]; bv[c] = beta[hd + o];
            }
        }
        for (int tb = t_lo; tb < t_hi; tb += 16) {
          // 4 independent 4-token steps in flight: every load of the 16 tokens is requested before the first is used
          float a[4][NB], v[4][NB], pk[4][2];
          bool okk[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = tb + 4 * u + kq;
            okk[u] = t < t_hi;
            const float* kr = kb + (int64_t)t * hD;
            const float* vr = vb + (int64_t)t * hD;
            pk[u][0] = pk[u][1] = 0.f;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                a[u][c] = okk[u] ? kr[p + 16 * c + i] : 0.f;
                v[u][c] = okk[u] ? vr[p + 16 * c + i] : 0.f;
            }
            if (p > 0) pk[u][0] = okk[u] ? kr[0] : 0.f;
            if (p > 1) pk[u][1] = okk[u] ? kr[1] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (gamma) {                                       // plain tiles: the LayerNorm affine on the way in
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    a[u][c] = okk[u] ? fmaf(a[u][c], gk[c], bk[c]) : 0.f;
                    v[u][c] = okk[u] ? fmaf(v[u][c], gv[c], bv[c]) : 0.f;
                }
            }
#pragma unroll
            for (int c = 0; c < NB; ++c)
#pragma unroll
                for (int e = 0; e < NB; ++e)
                    acc[c][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][c], v[u][e], acc[c][e], 0, 0, 0);
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                kp[c][0] = fmaf(a[u][c], pk[u][0], kp[c][0]); kp[c][1] = fmaf(a[u][c], pk[u][1], kp[c][1]);
                pv[c][0] = fmaf(pk[u][0], v[u][c], pv[c][0]); pv[c][1] = fmaf(pk[u][1], v[u][c], pv[c][1]);
            }
            pp[0][0] = fmaf(pk[u][0], pk[u][0], pp[0][0]); pp[0][1] = fmaf(pk[u][0], pk[u][1], pp[0][1]);
            pp[1][0] = fmaf(pk[u][1], pk[u][0], pp[1][0]); pp[1][1] = fmaf(pk[u][1], pk[u][1], pp[1][1]);
          }
        }
        // borders: combine the 4 token lanes
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                kp[c][e] += __shfl_xor(kp[c][e], 16, 64); kp[c][e] += __shfl_xor(kp[c][e], 32, 64);
                pv[c][e] += __shfl_xor(pv[c][e], 16, 64); pv[c][e] += __shfl_xor(pv[c][e], 32, 64);
            }
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 2; ++e) { pp[c][e] += __shfl_xor(pp[c][e], 16, 64); pp[c][e] += __shfl_xor(pp[c][e], 32, 64); }

        float* M = slabs + ((((int64_t)ch * B + b) * h + head) * DP) * DP;
        const int Dr = p + 16 * NB;
        // core: D layout of the 16x16 tile: row = 4*kq + r, col = i
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int e = 0; e < NB; ++e)
#pragma unroll
                for (int r = 0; r < 4; ++r) M[(int64_t)(p + 16 * c + 4 * kq + r) * DP + p + 16 * e + i] = acc[c][e][r];
        if (kq == 0) {
#pragma unroll
            for (int c = 0; c < NB; ++c)
                for (int e = 0; e < p; ++e) {
                    M[(int64_t)(p + 16 * c + i) * DP + e] = kp[c][e];         // K^T P
                    M[(int64_t)e * DP + p + 16 * c + i] = pv[c][e];           // P^T V
                }
            if (i == 0)
                for (int c = 0; c < p; ++c)
                    for (int e = 0; e < p; ++e) M[(int64_t)c * DP + e] = pp[c][e];
        }
        for (int e = lane; e < DP * DP; e += 64) {               // zero padding rows / columns
            const int rr = e / DP, cc = e % DP;
            if (rr >= Dr || cc >= Dr) M[e] = 0.f;
        }
    }
}

// Same product with the token rows staged through LDS.  The kernel above feeds the MFMA operands with 4-byte loads of 64-byte
// row pieces at an 8-byte offset (the coordinates sit in front of the values): 2.4-2.8 TB/s.  A tile of 16 tokens of all h
// heads is ONE contiguous 16 * h * DP * 4-byte piece of the head-tile array, so the block copies it with 16-byte loads
// (every byte of every line used, one request per 1 KiB) into LDS, register-staged one tile ahead, and the waves (one head
// each) read their operands from there (consecutive lanes on consecutive banks).  h <= 4, 16 * h * DP floats <= 4096.
constexpr int KTV_TT = 16;          // tokens per tile
constexpr int KTV_MAXG = 4;         // 16-byte granules per thread and operand tile (h * DP <= 256)
template <int NB>
__global__ __launch_bounds__(256) void galerkin_ktv_lds_kernel(const float* __restrict__ Kp, const float* __restrict__ Vp,
                                                               int n, int h, int DP, int p, int chunk,
                                                               float* __restrict__ slabs, int B,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta) {
    extern __shared__ __attribute__((aligned(16))) float ktv_lds[];      // [2 buffers][K | V][KTV_TT * hD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int i = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, ch = blockIdx.x;
    const int t_lo = ch * chunk, t_hi = min(n, t_lo + chunk);
    const int hD = h * DP, tile_f = KTV_TT * hD, ng = tile_f >> 2;
    const int head = wave;
    const bool active = head < h;

    f32x4 acc[NB][NB];
    float kp[NB][2], pv[NB][2], pp[2][2];
#pragma unroll
    for (int a = 0; a < NB; ++a) {
#pragma unroll
        for (int c = 0; c < NB; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        kp[a][0] = kp[a][1] = pv[a][0] = pv[a][1] = 0.f;
    }
    pp[0][0] = pp[0][1] = pp[1][0] = pp[1][1] = 0.f;
    float gk[NB], bk[NB], gv[NB], bv[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        gk[c] = gv[c] = 1.f;
        bk[c] = bv[c] = 0.f;
        if (gamma && active) {
            const int o = head * 16 * NB + 16 * c + i, hd = h * 16 * NB;
            gk[c] = gamma[o]; bk[c] = beta[o]; gv[c] = gamma[hd + o]; bv[c] = beta[hd + o];
        }
    }
    const float* kbase = Kp + (int64_t)b * n * hD;
    const float* vbase = Vp + (int64_t)b * n * hD;
    f32x4 rk[KTV_MAXG], rv[KTV_MAXG];
    auto gload = [&](int tb) {                    // tile tb .. tb + 15 -> registers (zeros past the chunk)
        const int valid_f = min(KTV_TT, t_hi - tb) * hD;
#pragma unroll
        for (int q = 0; q < KTV_MAXG; ++q) {
            const int g4 = (tid + 256 * q) * 4;
            const bool ok = g4 < valid_f;         // granules never straddle tokens (hD % 4 == 0)
            rk[q] = ok ? *reinterpret_cast<const f32x4*>(kbase + (int64_t)tb * hD + g4) : f32x4{0.f, 0.f, 0.f, 0.f};
            rv[q] = ok ? *reinterpret_cast<const f32x4*>(vbase + (int64_t)tb * hD + g4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto sstore = [&](int buf) {
        float* ks = ktv_lds + buf * 2 * tile_f;
#pragma unroll
        for (int q = 0; q < KTV_MAXG; ++q) {
            const int g = tid + 256 * q;
            if (g < ng) {
                *reinterpret_cast<f32x4*>(ks + 4 * g) = rk[q];
                *reinterpret_cast<f32x4*>(ks + tile_f + 4 * g) = rv[q];
            }
        }
    };
    int buf = 0;
    if (t_lo < t_hi) gload(t_lo);
    for (int tb = t_lo; tb < t_hi; tb += KTV_TT) {
        sstore(buf);
        __syncthreads();                           // tile tb is in LDS; everybody is done with the other buffer
        if (tb + KTV_TT < t_hi) gload(tb + KTV_TT);
        if (active) {
            const float* ks = ktv_lds + buf * 2 * tile_f + head * DP;
            const float* vs = ks + tile_f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int tt = 4 * u + kq;
                const bool ok = tb + tt < t_hi;
                float a[NB], v[NB], pk[2] = {0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    a[c] = ks[tt * hD + p + 16 * c + i];
                    v[c] = vs[tt * hD + p + 16 * c + i];
                    if (gamma) {                   // plain tiles: the LayerNorm affine on the way in (rows past the chunk stay 0)
                        a[c] = ok ? fmaf(a[c], gk[c], bk[c]) : 0.f;
                        v[c] = ok ? fmaf(v[c], gv[c], bv[c]) : 0.f;
                    }
                }
                if (p > 0) pk[0] = ks[tt * hD];
                if (p > 1) pk[1] = ks[tt * hD + 1];
#pragma unroll
                for (int c = 0; c < NB; ++c)
#pragma unroll
                    for (int e = 0; e < NB; ++e)
                        acc[c][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], v[e], acc[c][e], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    kp[c][0] = fmaf(a[c], pk[0], kp[c][0]); kp[c][1] = fmaf(a[c], pk[1], kp[c][1]);
                    pv[c][0] = fmaf(pk[0], v[c], pv[c][0]); pv[c][1] = fmaf(pk[1], v[c], pv[c][1]);
                }
                pp[0][0] = fmaf(pk[0], pk[0], pp[0][0]); pp[0][1] = fmaf(pk[0], pk[1], pp[0][1]);
                pp[1][0] = fmaf(pk[1], pk[0], pp[1][0]); pp[1][1] = fmaf(pk[1], pk[1], pp[1][1]);
            }
        }
        buf ^= 1;
    }
    if (!active) return;
    // borders: combine the 4 token lanes
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            kp[c][e] += __shfl_xor(kp[c][e], 16, 64); kp[c][e] += __shfl_xor(kp[c][e], 32, 64);
            pv[c][e] += __shfl_xor(pv[c][e], 16, 64); pv[c][e] += __shfl_xor(pv[c][e], 32, 64);
        }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 2; ++e) { pp[c][e] += __shfl_xor(pp[c][e], 16, 64); pp[c][e] += __shfl_xor(pp[c][e], 32, 64); }

    float* M = slabs + ((((int64_t)ch * B + b) * h + head) * DP) * DP;
    const int Dr = p + 16 * NB;
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int e = 0; e < NB; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) M[(int64_t)(p + 16 * c + 4 * kq + r) * DP + p + 16 * e + i] = acc[c][e][r];
    if (kq == 0) {
#pragma unroll
        for (int c = 0; c < NB; ++c)
            for (int e = 0; e < p; ++e) {
                M[(int64_t)(p + 16 * c + i) * DP + e] = kp[c][e];         // K^T P
                M[(int64_t)e * DP + p + 16 * c + i] = pv[c][e];           // P^T V
            }
        if (i == 0)
            for (int c = 0; c < p; ++c)
                for (int e = 0; e < p; ++e) M[(int64_t)c * DP + e] = pp[c][e];
    }
    for (int e = lane; e < DP * DP; e += 64) {               // zero padding rows / columns
        const int rr = e / DP, cc = e % DP;
        if (rr >= Dr || cc >= Dr) M[e] = 0.f;
    }
}

// the instance for dk = 16 NB of either kernel
template <int NB>
static auto ktv_pick(bool staged) { return staged ? galerkin_ktv_lds_kernel<NB> : galerkin_ktv_kernel<NB>; }

// ------------------------------------------------------------------------------------------ galerkin finalize
// One block per (batch, head, group of FIN_RB rows of M): row j of P needs row j of M only.  (Round 5: one block per
// (batch, head) walked the whole 52 x 52 matrix with n_slabs dependent loads per element -- 178 us at ex4's 16 x 64 slabs.)
// Rows per block: a quarter of the matrix (round 6; four until then).  Every block stages all of W_h (d x DP floats: 18 KB at
// d = 128, 40 KB at d = 192) for its rows' products -- with four rows per block that staging was most of the kernel's traffic
// (4 608 blocks x 18 KB at C2, 6 656 x 40 KB at C4).
static inline int fin_rows_per_block(int DP) { return std::max(4, (DP + 3) / 4); }
__global__ __launch_bounds__(256) void galerkin_fin_fwd_kernel(
    const float* __restrict__ slabs, int n_slabs, int64_t slab_stride, int h, int DP, int Dr, int d,
    float inv_n, const float* __restrict__ mask, DropDev drop, const float* __restrict__ Wfc,
    float* __restrict__ Mt, float* __restrict__ P, float* __restrict__ Pv, int pdim, int FIN_RB) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // Both operands of the product loop are read as 16-byte vectors along the contraction (DP % 4 == 0; W_h's rows are padded
    // to DP columns with zeros): a quarter of the LDS instructions of the scalar loop, which was what the kernel waited for.
    float* sM = lds;                    // [FIN_RB][DP]
    float* sW = lds + FIN_RB * DP;      // [d][DP]
    const int bh = blockIdx.x, b = bh / h, hh = bh % h;
    const int j0 = blockIdx.y * FIN_RB, nr = min(FIN_RB, DP - j0);
    const uint32_t key = drop_key_dev(drop);
    const int64_t mo = (int64_t)bh * DP * DP;
    for (int le = threadIdx.x; le < nr * DP; le += blockDim.x) {
        const int e = j0 * DP + le, j = e / DP, c = e % DP;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;           // four independent chains: the loads overlap
        int k = 0;
        for (; k + 4 <= n_slabs; k += 4) {
            s0 += slabs[(k + 0) * slab_stride + mo + e];
            s1 += slabs[(k + 1) * slab_stride + mo + e];
            s2 += slabs[(k + 2) * slab_stride + mo + e];
            s3 += slabs[(k + 3) * slab_stride + mo + e];
        }
        for (; k < n_slabs; ++k) s0 += slabs[k * slab_stride + mo + e];
        const float s = (s0 + s1) + (s2 + s3);
        float mul = inv_n;
        if (mask) mul *= mask[mo + e];
        else if (drop.thresh) mul *= drop_mul(drop, key, (uint32_t)(mo + e));
        const float v = (j < Dr && c < Dr) ? s * mul : 0.f;
        sM[le] = v;
        Mt[mo + e] = v;
    }
    for (int e = threadIdx.x; e < d * DP; e += blockDim.x) {
        const int c = e / DP, ee = e % DP;
        sW[e] = ee < Dr ? Wfc[(int64_t)c * (h * Dr) + hh * Dr + ee] : 0.f;
    }
    __syncthreads();
    float* Pb = P + ((int64_t)b * h * DP + (int64_t)hh * DP) * d;
    for (int le = threadIdx.x; le < nr * d; le += blockDim.x) {
        const int jl = le / d, c = le % d, j = j0 + jl;
        float acc = 0.f;
        if (j < Dr) {
            const f32x4* mr = reinterpret_cast<const f32x4*>(sM + jl * DP);
            const f32x4* wr = reinterpret_cast<const f32x4*>(sW + c * DP);
            for (int q = 0; q < (DP >> 2); ++q) {           // the scalar loop's order (the zero columns behind Dr add nothing)
                const f32x4 m4 = mr[q], w4 = wr[q];
                acc = fmaf(m4[0], w4[0], acc); acc = fmaf(m4[1], w4[1], acc);
                acc = fmaf(m4[2], w4[2], acc); acc = fmaf(m4[3], w4[3], acc);
            }
        }
        Pb[(int64_t)j * d + c] = acc;
        // the value rows of P once more, compact [B][h dk][d]: the B operand of the backward's dQ product (it used to be
        // sliced out of P by an ATen copy in every backward)
        if (Pv && j >= pdim && j < Dr) Pv[((int64_t)b * h * (Dr - pdim) + (int64_t)hh * (Dr - pdim) + (j - pdim)) * d + c] = acc;
    }
}

__global__ __launch_bounds__(256) void galerkin_fin_bwd_kernel(
    const float* __restrict__ dPt, const float* __restrict__ Mt, const float* __restrict__ mask,
    DropDev drop, const float* __restrict__ Wfc, int h, int DP, int Dr, int d, float inv_n,
    float* __restrict__ dM, float* __restrict__ dWfc_slabs) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // gridDim.y blocks share the two output loops of one (batch, head): part q owns ROWS [j0, j1) of dM and feature COLUMNS
    // [c0, c1) of dWfc, and stages only what those need -- the row slice and the column slice of dP_h, all of W_h and M.
    // (Round 6: every part used to stage all of dP_h; at d = 192, DP = 52 that was 89 KB of LDS, one block per CU and
    // 252 us per launch -- now 69 KB at four parts, two blocks per CU.)
    const int part = blockIdx.y, parts = gridDim.y;
    const int jr = (DP + parts - 1) / parts, j0 = part * jr, j1 = min(DP, j0 + jr), nj = max(0, j1 - j0);
    const int cr = (d + parts - 1) / parts, c0 = part * cr, c1 = min(d, c0 + cr), nc = max(0, c1 - c0);
    const int dpitch = d + 1, cpitch = cr + 1;
    // W_h (rows padded to DP columns with zeros) and M first: both are read as 16-byte vectors along ee (four outputs per
    // thread: one broadcast scalar + one vector read per four FMAs, where the scalar loops issued two reads per FMA)
    float* sW = lds;                        // [d][DP]
    float* sM = sW + d * DP;                // [DP][DP]
    float* sdr = sM + DP * DP;              // [jr][d+1]    dP_h[j0 + j][c]        (rows of this part, every feature)
    float* sdc = parts == 1 ? sdr : sdr + jr * dpitch;    // [DP][cr+1]   dP_h[j][c0 + c]   (every row, features of this part;
                                                          //  one part: the same image as sdr)
    const int bh = blockIdx.x, b = bh / h, hh = bh % h;
    const uint32_t key = drop_key_dev(drop);
    const int64_t mo = (int64_t)bh * DP * DP;
    const float* src = dPt + (int64_t)b * d * (h * DP) + hh * DP;
    for (int e = threadIdx.x; e < d * nj; e += blockDim.x) {
        const int c = e / nj, j = e % nj;
        sdr[j * dpitch + c] = src[(int64_t)c * (h * DP) + j0 + j];
    }
    if (parts > 1)
        for (int e = threadIdx.x; e < nc * DP; e += blockDim.x) {
            const int c = e / DP, j = e % DP;
            sdc[j * cpitch + c] = src[(int64_t)(c0 + c) * (h * DP) + j];
        }
    for (int e = threadIdx.x; e < d * DP; e += blockDim.x) {
        const int c = e / DP, ee = e % DP;
        sW[e] = ee < Dr ? Wfc[(int64_t)c * (h * Dr) + hh * Dr + ee] : 0.f;
    }
    for (int e = threadIdx.x; e < DP * DP; e += blockDim.x) sM[e] = Mt[mo + e];
    __syncthreads();
    const int Q4 = DP >> 2;
    for (int e = threadIdx.x; e < nj * Q4; e += blockDim.x) {
        const int jl = e / Q4, q = e - jl * Q4, j = j0 + jl;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (j < Dr) {
            const float* dp = sdr + jl * dpitch;
            for (int c = 0; c < d; ++c) acc += dp[c] * *reinterpret_cast<const f32x4*>(sW + c * DP + 4 * q);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ee = 4 * q + t;
                float mul = inv_n;
                if (mask) mul *= mask[mo + j * DP + ee];
                else if (drop.thresh) mul *= drop_mul(drop, key, (uint32_t)(mo + j * DP + ee));
                acc[t] = ee < Dr ? acc[t] * mul : 0.f;
            }
        }
        *reinterpret_cast<f32x4*>(dM + mo + j * DP + 4 * q) = acc;
    }
    float* dst = dWfc_slabs + (int64_t)b * d * (h * Dr) + hh * Dr;
    for (int e = threadIdx.x; e < nc * Q4; e += blockDim.x) {
        const int cl = e / Q4, q = e - cl * Q4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < Dr; ++j) acc += sdc[j * cpitch + cl] * *reinterpret_cast<const f32x4*>(sM + j * DP + 4 * q);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * q + t < Dr) dst[(int64_t)(c0 + cl) * (h * Dr) + 4 * q + t] = acc[t];
    }
}

// ------------------------------------------------------------------------------------------ galerkin dK', dV'
// dK'[t] = V'[t] dM^T and dV'[t] = K'[t] dM for every token of one (batch, head)  -- the backward of
// M = K'^T V' (layers.py:723) -- as one streaming pass: the two DP x DP operands live in registers as MFMA A
// fragments, token rows go from HBM straight into B fragments.  A row of DP = 16G + 4 floats is G*4 + 1
// float4: lane (row j, kq) loads float4 number kq + 4g (g < G) and the last one; k-step (g, c) contracts
// k = 4(kq + 4g) + c (component c of the lane's g-th float4), the final step k = 16G + kq (component kq of the
// shared last float4) -- every k exactly once, every load a full 64-byte run per row.  Result tiles come out
// transposed (output column x row), i.e. one float4 of the output row per lane.
struct DkvP {
    const float* Kp; const float* Vp; const float* dM; float* dKp; float* dVp;
    int n, h;
};
template <int G>
__global__ __launch_bounds__(256, 2) void galerkin_dkv_kernel(const DkvP p) {
    constexpr int DP = 16 * G + 4, NS = 4 * G + 1, NMT = G + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int head = blockIdx.x % p.h, b = blockIdx.x / p.h;
    const int64_t hD = (int64_t)p.h * DP;
    const int64_t base = ((int64_t)b * p.n) * hD + (int64_t)head * DP;
    const float* dm = p.dM + ((int64_t)b * p.h + head) * DP * DP;
    // A fragments: lane (i = output column 16mt + j, kq); a1 -> dK' (dM[col][k]), a2 -> dV' (dM[k][col])
    float a1[NMT][NS], a2[NMT][NS];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt) {
        const int col = 16 * mt + j, cc = min(col, DP - 1);
        const float live = col < DP ? 1.f : 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = (s < 4 * G) ? 4 * (kq + 4 * (s >> 2)) + (s & 3) : 16 * G + kq;
            a1[mt][s] = live * dm[cc * DP + k];
            a2[mt][s] = live * dm[k * DP + cc];
        }
    }
    // token tiles of this (batch, head) are shared out over gridDim.y blocks (ex4: B h = 16 would leave 240 CUs idle)
    const int ntile = (p.n + 15) >> 4, per = (ntile + gridDim.y - 1) / gridDim.y;
    const int tend = min(ntile, (int)(blockIdx.y + 1) * per);
    for (int tile = blockIdx.y * per + wave; tile < tend; tile += 4) {
        const int t = 16 * tile + j, tc = min(t, p.n - 1);
        const float* kr = p.Kp + base + (int64_t)tc * hD;
        const float* vr = p.Vp + base + (int64_t)tc * hD;
        f32x4 kk[G + 1], vv[G + 1];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            kk[g] = *reinterpret_cast<const f32x4*>(kr + 4 * (kq + 4 * g));
            vv[g] = *reinterpret_cast<const f32x4*>(vr + 4 * (kq + 4 * g));
        }
        kk[G] = *reinterpret_cast<const f32x4*>(kr + 16 * G);
        vv[G] = *reinterpret_cast<const f32x4*>(vr + 16 * G);
        f32x4 acc1[NMT], acc2[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) acc1[mt] = acc2[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float bv, bk;
            if (s < 4 * G) { bv = vv[s >> 2][s & 3]; bk = kk[s >> 2][s & 3]; }
            else {
                bv = kq == 0 ? vv[G][0] : (kq == 1 ? vv[G][1] : (kq == 2 ? vv[G][2] : vv[G][3]));
                bk = kq == 0 ? kk[G][0] : (kq == 1 ? kk[G][1] : (kq == 2 ? kk[G][2] : kk[G][3]));
            }
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                acc1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[mt][s], bv, acc1[mt], 0, 0, 0);
                acc2[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[mt][s], bk, acc2[mt], 0, 0, 0);
            }
        }
        if (t < p.n) {
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                const int col = 16 * mt + 4 * kq;
                if (col < DP) {
                    *reinterpret_cast<f32x4*>(p.dKp + base + (int64_t)t * hD + col) = acc1[mt];
                    *reinterpret_cast<f32x4*>(p.dVp + base + (int64_t)t * hD + col) = acc2[mt];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- galerkin dK', dV' with the LayerNorm backward behind them
// The two products of galerkin_dkv_kernel, and on the same registers the per-head LayerNorm backward of
// headnorm_bwd_v2_kernel for the K and V streams (layers.py:841-874 backwards): the head-tile gradients dK', dV'
// ([T][h][DP], 2 x 136 MB at B = 128) are never written or read back.  A lane holds four consecutive tile columns
// 16 mt + 4 kq .. + 3 of token row j (columns in value order, see the kernel): a row's dk values sit in the four kq
// lanes of its j, so the two row means are a local sum and two cross-lane adds.  d(gamma), d(beta): per-lane running sums
// over the block's tokens, folded over the 16 token lanes, then over the four waves in LDS in a fixed order; block
// (b, head) owns the head's dk-slice of partial[b][dg K | dg V | db K | db V] (the layout gt_headnorm_bwd reduces).
struct DkvLnP {
    const float* Kp; const float* Vp; const float* dM;
    const float* qkv; const float* gamma; const float* stats;
    float* d_qkv; float* partial;
    int n, h, dk, p, T;
    const float* beta;                              // PLAIN only
};
// PLAIN: the head tiles hold the normalised values WITHOUT the LayerNorm affine (gt_hip.h: hn_plain): K' = gamma_K xh + beta_K
// is never formed -- gamma scales the rows of the dM fragments (the contraction index is the tile column), beta dM is a
// per-output-column constant added to the products, and xh for the LayerNorm backward is the tile itself: the raw
// projection is neither stored by the forward nor read here.
// G = 3 (DP = 52: ex3's 48-wide heads): the two sets of dM fragments alone are 104 registers -- at two blocks per CU the
// kernel spilled 220 (PLAIN) / 119 registers to scratch and ran 2.7x slower per token than G = 2 (499 vs 181 us for the same
// bytes, round 6 profile); one block per CU opens the whole 512-entry register file (no scratch).
template <int G, bool PLAIN>
__global__ __launch_bounds__(256, (G >= 3 ? 1 : 2)) void galerkin_dkv_ln_kernel(const DkvLnP p) {
    constexpr int DP = 16 * G + 4, NS = 4 * G + 1, NMT = G + 1;
    __shared__ float red[4][4][NMT][4][4];          // [wave][kq][mt][c][dgK, dbK, dgV, dbV]
    __shared__ __attribute__((aligned(16))) float cst[2][4][NMT][4];    // PLAIN: [dK' | dV'][kq][mt][c] = (beta dM) of the lane's columns
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int head = blockIdx.x % p.h, b = blockIdx.x / p.h;
    const int64_t hD = (int64_t)p.h * DP;
    const int64_t base = ((int64_t)b * p.n) * hD + (int64_t)head * DP;
    const float* dm = p.dM + ((int64_t)b * p.h + head) * DP * DP;
    const int hd = p.h * p.dk, d3 = 3 * hd;
    const float inv = 1.f / (float)p.dk;
    // output columns in VALUE order: column c' < dk is value c' (tile column p + c'), the coordinate columns follow, then
    // the pad -- a permutation of the rows of the dM fragments, so that the lane's four consecutive outputs are an
    // aligned float4 of the raw projection row and of its gradient
    float a1[NMT][NS], a2[NMT][NS];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt) {
        const int cp = 16 * mt + j;
        const int col = cp < p.dk ? cp + p.p : (cp < p.dk + p.p ? cp - p.dk : cp), cc = min(col, DP - 1);
        const float live = cp < DP ? 1.f : 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = (s < 4 * G) ? 4 * (kq + 4 * (s >> 2)) + (s & 3) : 16 * G + kq;
            float sv = 1.f, sk = 1.f;               // PLAIN: the operand rows carry xh; its gamma moves onto dM
            if (PLAIN && k >= p.p && k < p.p + p.dk) {
                sv = p.gamma[hd + (int64_t)head * p.dk + k - p.p];
                sk = p.gamma[(int64_t)head * p.dk + k - p.p];
            }
            a1[mt][s] = live * sv * dm[cc * DP + k];
            a2[mt][s] = live * sk * dm[k * DP + cc];
        }
    }
    if (PLAIN) {                                     // beta dM of every output column, once per block
        for (int e = threadIdx.x; e < 2 * 4 * NMT * 4; e += blockDim.x) {
            const int c = e & 3, mt = (e >> 2) % NMT, kq2 = (e / (4 * NMT)) & 3, which = e / (16 * NMT);
            const int cp = 16 * mt + 4 * kq2 + c;
            const int col = cp < p.dk ? cp + p.p : (cp < p.dk + p.p ? cp - p.dk : cp);
            float acc = 0.f;
            if (cp < DP)
                for (int v = 0; v < p.dk; ++v) {
                    const int k = p.p + v;
                    acc += which == 0 ? p.beta[hd + (int64_t)head * p.dk + v] * dm[col * DP + k]      // dK' = V' dM^T
                                      : p.beta[(int64_t)head * p.dk + v] * dm[k * DP + col];           // dV' = K' dM
                }
            cst[which][kq2][mt][c] = acc;
        }
        __syncthreads();
    }
    bool ok[NMT];                                   // the lane's float4 of group mt holds values (dk % 4 == 0: all or none)
    f32x4 gmK[NMT], gmV[NMT];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt) {
        const int v0 = 16 * mt + 4 * kq;
        ok[mt] = v0 < p.dk;
        gmK[mt] = gmV[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok[mt]) {
            gmK[mt] = *reinterpret_cast<const f32x4*>(p.gamma + (int64_t)head * p.dk + v0);
            gmV[mt] = *reinterpret_cast<const f32x4*>(p.gamma + hd + (int64_t)head * p.dk + v0);
        }
    }
    f32x4 dgK[NMT], dbK[NMT], dgV[NMT], dbV[NMT];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt) dgK[mt] = dbK[mt] = dgV[mt] = dbV[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // a (batch, head)'s token tiles are shared out over gridDim.y blocks (small batches: B h blocks alone leave the chip idle)
    const int ntile = (p.n + 15) >> 4, per = (ntile + gridDim.y - 1) / gridDim.y;
    const int tend = min(ntile, (int)(blockIdx.y + 1) * per);
    for (int tile = blockIdx.y * per + wave; tile < tend; tile += 4) {
        const int t = 16 * tile + j, tc = min(t, p.n - 1);
        const int64_t tok = (int64_t)b * p.n + tc;
        const float* kr = p.Kp + base + (int64_t)tc * hD;
        const float* vr = p.Vp + base + (int64_t)tc * hD;
        f32x4 kk[G + 1], vv[G + 1];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            kk[g] = *reinterpret_cast<const f32x4*>(kr + 4 * (kq + 4 * g));
            vv[g] = *reinterpret_cast<const f32x4*>(vr + 4 * (kq + 4 * g));
        }
        kk[G] = *reinterpret_cast<const f32x4*>(kr + 16 * G);
        vv[G] = *reinterpret_cast<const f32x4*>(vr + 16 * G);
        // raw projection rows (PLAIN: the normalised values themselves, in value order, out of the tile rows just
        // requested -- cache-hot) and statistics of this token: requested before the products, used after them
        const float* xk = PLAIN ? kr + p.p + 4 * kq : p.qkv + tok * d3 + hd + head * p.dk + 4 * kq;       // + 16 mt
        const float* xv = PLAIN ? vr + p.p + 4 * kq : xk + hd;
        f32x4 xK[NMT], xV[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            xK[mt] = xV[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok[mt]) {
                xK[mt] = PLAIN ? tile_load4(xk + 16 * mt, p.p) : *reinterpret_cast<const f32x4*>(xk + 16 * mt);
                xV[mt] = PLAIN ? tile_load4(xv + 16 * mt, p.p) : *reinterpret_cast<const f32x4*>(xv + 16 * mt);
            }
        }
        const f32x2 stK = *reinterpret_cast<const f32x2*>(p.stats + (tok * p.h + head) * 2);
        const f32x2 stV = *reinterpret_cast<const f32x2*>(p.stats + (((int64_t)p.T + tok) * p.h + head) * 2);

        f32x4 acc1[NMT], acc2[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            acc1[mt] = acc2[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (PLAIN) {
                acc1[mt] = *reinterpret_cast<const f32x4*>(&cst[0][kq][mt][0]);
                acc2[mt] = *reinterpret_cast<const f32x4*>(&cst[1][kq][mt][0]);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float bv, bk;
            if (s < 4 * G) { bv = vv[s >> 2][s & 3]; bk = kk[s >> 2][s & 3]; }
            else {
                bv = kq == 0 ? vv[G][0] : (kq == 1 ? vv[G][1] : (kq == 2 ? vv[G][2] : vv[G][3]));
                bk = kq == 0 ? kk[G][0] : (kq == 1 ? kk[G][1] : (kq == 2 ? kk[G][2] : kk[G][3]));
            }
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                acc1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[mt][s], bv, acc1[mt], 0, 0, 0);
                acc2[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[mt][s], bk, acc2[mt], 0, 0, 0);
            }
        }
        const bool live = t < p.n;
        // LayerNorm backward of one stream on the lane's columns: gy = d(normalised head row), x = raw row (PLAIN: xh)
        auto ln_bwd = [&](const f32x4 (&gy)[NMT], const f32x4 (&x)[NMT], const f32x4 (&gm)[NMT], f32x2 st,
                          f32x4 (&dg)[NMT], f32x4 (&db)[NMT], float* __restrict__ dst) {
            const float mu = st[0], rstd = st[1];
            f32x4 xh[NMT], gg[NMT];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    xh[mt][c] = ok[mt] ? (PLAIN ? x[mt][c] : (x[mt][c] - mu) * rstd) : 0.f;
                    gg[mt][c] = ok[mt] ? gy[mt][c] * gm[mt][c] : 0.f;
                    s1 += gg[mt][c];
                    s2 += gg[mt][c] * xh[mt][c];
                }
            s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            const float m1 = s1 * inv, m2 = s2 * inv;
            if (!live) return;
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                if (!ok[mt]) continue;
                f32x4 dx;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    dx[c] = rstd * (gg[mt][c] - m1 - xh[mt][c] * m2);
                    dg[mt][c] += gy[mt][c] * xh[mt][c];
                    db[mt][c] += gy[mt][c];
                }
                *reinterpret_cast<f32x4*>(dst + 16 * mt) = dx;
            }
        };
        float* dk_row = p.d_qkv + tok * d3 + hd + head * p.dk + 4 * kq;
        ln_bwd(acc1, xK, gmK, stK, dgK, dbK, dk_row);
        ln_bwd(acc2, xV, gmV, stV, dgV, dbV, dk_row + hd);
    }
    // fold the 16 token lanes, then the four waves (fixed order)
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v[4] = {dgK[mt][c], dbK[mt][c], dgV[mt][c], dbV[mt][c]};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) v[q] += __shfl_xor(v[q], m, 64);
                if (j == 0) red[wave][kq][mt][c][q] = v[q];
            }
        }
    __syncthreads();
    float* pg = p.partial + ((int64_t)b * gridDim.y + blockIdx.y) * 4 * hd + (int64_t)head * p.dk;
    for (int e = threadIdx.x; e < 4 * NMT * 4 * 4; e += blockDim.x) {
        const int q = e & 3, c = (e >> 2) & 3, mt = (e >> 4) % NMT, kq2 = e / (16 * NMT);
        const int v = 16 * mt + 4 * kq2 + c;
        if (v >= p.dk) continue;
        const float sum = ((red[0][kq2][mt][c][q] + red[1][kq2][mt][c][q]) + red[2][kq2][mt][c][q]) + red[3][kq2][mt][c][q];
        // q: 0 dg K, 1 db K, 2 dg V, 3 db V   ->  partial row [dg K | dg V | db K | db V], each h*dk wide
        pg[((q & 1) * 2 + (q >> 1)) * hd + v] = sum;
    }
}

// Q stream of the galerkin backward (not normalised): drop the coordinate / pad columns of dQ' [T][h][DP] into the Q block
// of d_qkv [T][3 h dk]
__global__ __launch_bounds__(256) void headtile_unpad_kernel(const float* __restrict__ src, float* __restrict__ d_qkv,
                                                             int64_t total4, int h, int dk, int p, int DP) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total4) return;
    const int Q4 = dk >> 2;
    const int q = (int)(e % Q4), head = (int)((e / Q4) % h);
    const int64_t t = e / ((int64_t)Q4 * h);
    const f32x4 v = tile_load4(src + (t * h + head) * DP + p + 4 * q, p);
    *reinterpret_cast<f32x4*>(d_qkv + t * 3 * h * dk + head * dk + 4 * q) = v;
}

static inline int dkv_ln_chunks(int B, int h) { return std::max(1, std::min(16, 512 / std::max(1, B * h))); }
// the instance for DP = 16 G + 4 in {20, 36, 52}
template <bool PLAIN>
static auto dkv_ln_pick(int DP) {
    return DP == 20 ? galerkin_dkv_ln_kernel<1, PLAIN> : DP == 36 ? galerkin_dkv_ln_kernel<2, PLAIN> : galerkin_dkv_ln_kernel<3, PLAIN>;
}

}  // namespace gt

using namespace gt;

extern "C" int32_t gt_galerkin_ktv_slabs(int32_t B, int32_t n) {
    // token chunks per sample: enough blocks to fill the chip (~4 per CU), at least 64 tokens per chunk
    return std::max(1, std::min(ceil_div(1024, std::max(B, 1)), ceil_div(n, 64)));
}

extern "C" int gt_galerkin_ktv(const float* Kp, const float* Vp, int32_t B, int32_t n, int32_t h, int32_t dk,
                               int32_t p, float* slabs, int32_t n_slabs, void* stream) {
    return gt_galerkin_ktv_affine(Kp, Vp, nullptr, nullptr, B, n, h, dk, p, slabs, n_slabs, stream);
}

extern "C" int gt_galerkin_ktv_affine(const float* Kp, const float* Vp, const float* gamma, const float* beta, int32_t B,
                                      int32_t n, int32_t h, int32_t dk, int32_t p, float* slabs, int32_t n_slabs,
                                      void* stream) {
    if (!Kp || !Vp || !slabs || B <= 0 || n <= 0 || h <= 0 || dk <= 0 || p < 0 || n_slabs <= 0) return GT_EINVAL;
    if ((gamma == nullptr) != (beta == nullptr)) return GT_EINVAL;
    if ((dk & 15) || dk > 96 || p > 2) return GT_ENOTSUP;
    if (B > 65535) return GT_EINVAL;
    const int DP = round4(dk + p);
    const int chunk = ((ceil_div(n, n_slabs) + 3) / 4) * 4;
    if ((int64_t)chunk * n_slabs < n) return GT_EINVAL;
    dim3 grid((unsigned)n_slabs, (unsigned)B);
    // LDS-staged rows (16-byte loads of whole contiguous token tiles): one head per wave, 16 * h * DP floats per operand tile
    const bool staged = h <= 4 && h * DP <= 256 && !misaligned16(Kp, Vp);
    const int nb = dk / 16;
    const auto kern = nb == 1 ? ktv_pick<1>(staged) : nb == 2 ? ktv_pick<2>(staged) : nb == 3 ? ktv_pick<3>(staged)
                    : nb == 4 ? ktv_pick<4>(staged) : nb == 6 ? ktv_pick<6>(staged) : nullptr;
    if (!kern) return GT_ENOTSUP;
    const size_t lds = staged ? (size_t)2 * 2 * KTV_TT * h * DP * sizeof(float) : 0;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, Kp, Vp, n, h, DP, p, chunk, slabs, B, gamma, beta);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_galerkin_finalize_fwd(const float* slabs, int32_t n_slabs, int64_t slab_stride, int32_t B,
                                        int32_t h, int32_t DP, int32_t Dr, int32_t d, int32_t n_tokens,
                                        const float* mask, const gt_dropout* drop, const float* Wfc,
                                        float* Mt, float* P, float* Pv, int32_t pos_dim, void* stream) {
    if (!slabs || !Wfc || !Mt || !P || n_slabs <= 0 || B <= 0 || h <= 0 || Dr <= 0 || DP < Dr || d <= 0 ||
        n_tokens <= 0 || pos_dim < 0 || pos_dim >= Dr)
        return GT_EINVAL;
    if (drop && drop->p > 0.f && !drop->seed) return GT_EINVAL;
    if (DP & 3) return GT_EINVAL;
    // (few (batch, head) pairs: four rows per block as before, for the parallelism of the slab sums)
    const int FIN_RB = B * h >= 256 ? fin_rows_per_block(DP) : 4;
    const size_t lds = ((size_t)FIN_RB * DP + (size_t)d * DP) * sizeof(float);
    if (int rc = allow_big_lds<galerkin_fin_fwd_kernel>(lds)) return rc;
    hipLaunchKernelGGL(galerkin_fin_fwd_kernel, dim3(B * h, (DP + FIN_RB - 1) / FIN_RB), dim3(256), lds, (hipStream_t)stream, slabs,
                       n_slabs, slab_stride, h, DP, Dr, d, 1.f / (float)n_tokens, mask,
                       make_drop(mask ? nullptr : drop), Wfc, Mt, P, Pv, pos_dim, FIN_RB);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_galerkin_finalize_bwd(const float* dPt, const float* Mt, const float* mask,
                                        const gt_dropout* drop, const float* Wfc, int32_t B, int32_t h,
                                        int32_t DP, int32_t Dr, int32_t d, int32_t n_tokens, float* dM,
                                        float* dWfc_slabs, void* stream) {
    if (!dPt || !Mt || !Wfc || !dM || !dWfc_slabs || B <= 0 || h <= 0 || Dr <= 0 || DP < Dr || d <= 0 ||
        n_tokens <= 0)
        return GT_EINVAL;
    if (drop && drop->p > 0.f && !drop->seed) return GT_EINVAL;
    // parts: enough blocks to fill the chip (each part stages W_h and M in full, its slices of dP_h); wide models (d >= 160:
    // the full staging would leave one block per CU) always take four
    const int parts = std::max(d >= 160 ? 4 : 1, std::min(4, 1024 / (B * h)));
    const size_t lds = ((size_t)((DP + parts - 1) / parts) * (d + 1) + (parts > 1 ? (size_t)DP * ((d + parts - 1) / parts + 1) : 0) +
                        (size_t)d * DP + (size_t)DP * DP) * sizeof(float);
    if ((DP & 3) || misaligned16(dM)) return GT_EINVAL;
    if (int rc = allow_big_lds<galerkin_fin_bwd_kernel>(lds)) return rc;
    hipLaunchKernelGGL(galerkin_fin_bwd_kernel, dim3(B * h, parts), dim3(256), lds, (hipStream_t)stream, dPt, Mt,
                       mask, make_drop(mask ? nullptr : drop), Wfc, h, DP, Dr, d, 1.f / (float)n_tokens, dM,
                       dWfc_slabs);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_galerkin_dkv(const float* Kp, const float* Vp, const float* dM, float* dKp, float* dVp,
                               int32_t B, int32_t n, int32_t h, int32_t DP, void* stream) {
    if (!Kp || !Vp || !dM || !dKp || !dVp || B <= 0 || n <= 0 || h <= 0) return GT_EINVAL;
    if (DP != 20 && DP != 36 && DP != 52) return GT_ENOTSUP;
    if (misaligned16(Kp, Vp, dKp, dVp)) return GT_EALIGN;
    DkvP p{Kp, Vp, dM, dKp, dVp, n, h};
    const int ntile = (n + 15) / 16;
    const int chunks = std::max(1, std::min({(1024 + B * h - 1) / (B * h), (ntile + 7) / 8, 65535}));
    dim3 grid((unsigned)(B * h), (unsigned)chunks);
    const auto kern = DP == 20 ? galerkin_dkv_kernel<1> : DP == 36 ? galerkin_dkv_kernel<2> : galerkin_dkv_kernel<3>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, p);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_galerkin_dkv_ln_ws_bytes(int32_t B, int32_t h, int32_t dk) {
    return (int64_t)B * dkv_ln_chunks(B, h) * 4 * h * dk * (int64_t)sizeof(float);
}

extern "C" int gt_galerkin_dkv_ln(const float* Kp, const float* Vp, const float* dM, const float* dQp, const float* qkv,
                                  const float* gamma, const float* stats, int32_t B, int32_t n, int32_t h, int32_t dk,
                                  int32_t p, float* d_qkv, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes,
                                  void* stream) {
    if (!qkv) return GT_EINVAL;
    return gt_galerkin_dkv_ln_plain(Kp, Vp, dM, dQp, qkv, gamma, nullptr, stats, B, n, h, dk, p, d_qkv, dgamma, dbeta, ws,
                                    ws_bytes, stream);
}

// beta != NULL: "plain" head tiles (gt_hip.h: hn_plain), qkv unused (may be NULL)
extern "C" int gt_galerkin_dkv_ln_plain(const float* Kp, const float* Vp, const float* dM, const float* dQp,
                                        const float* qkv, const float* gamma, const float* beta, const float* stats,
                                        int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p, float* d_qkv,
                                        float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, void* stream) {
    if (!Kp || !Vp || !dM || (!qkv && !beta) || !gamma || !stats || !d_qkv || !dgamma || !dbeta) return GT_EINVAL;
    if (B <= 0 || n <= 0 || h <= 0 || dk <= 0 || p < 0) return GT_EINVAL;
    const int DP = round4(dk + p);
    if ((DP != 20 && DP != 36 && DP != 52) || (dk & 3)) return GT_ENOTSUP;
    if (misaligned16(Kp, Vp, dQp, qkv, d_qkv, stats, gamma)) return GT_EALIGN;      // dQp may be 0
    if (!ws || ws_bytes < gt_galerkin_dkv_ln_ws_bytes(B, h, dk)) return GT_EWS;
    hipStream_t st = (hipStream_t)stream;
    const int hd = h * dk;
    float* partial = reinterpret_cast<float*>(ws);
    DkvLnP q{Kp, Vp, dM, qkv, gamma, stats, d_qkv, partial, n, h, dk, p, B * n, beta};
    const int chunks = dkv_ln_chunks(B, h);
    dim3 grid((unsigned)(B * h), (unsigned)chunks);
    const auto kern = beta ? dkv_ln_pick<true>(DP) : dkv_ln_pick<false>(DP);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, q);
    GT_LAUNCH_CHECK();
    if (dQp) {                                     // NULL: the caller's dQ product wrote the Q block itself
        const int64_t total4 = (int64_t)B * n * h * (dk >> 2);
        hipLaunchKernelGGL(headtile_unpad_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dQp, d_qkv,
                           total4, h, dk, p, DP);
        GT_LAUNCH_CHECK();
    }
    if (int rc = gt_slab_reduce(partial, 4 * hd, B * chunks, 2 * hd, 1.f, dgamma, stream)) return rc;
    return gt_slab_reduce(partial + 2 * hd, 4 * hd, B * chunks, 2 * hd, 1.f, dbeta, stream);
}
