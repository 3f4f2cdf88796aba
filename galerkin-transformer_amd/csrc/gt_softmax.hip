// Softmax attention  O = (softmax(Q' K'^T * scale) .* m) V'   (layers.py:672-705, attention_type='softmax') in fp32.
//
// Fused route: gt_fourier.hip's flash kernel (owner rows as resident MFMA B fragments, the other token axis streamed through
// double-buffered global->LDS tiles, the score tile consumed by the second product from the same lane's accumulator
// registers) plus what the softmax needs: a running row maximum, a running row sum and a rescale in the forward, and
// P = exp(S - L) recomputed from the saved L = max + log(sum) in the two backward passes.  The n x n matrix never reaches HBM.
//
//   pass      owner    F1            F2    T1   T2    score tiles (stream x owner)          second product(s)
//   forward   queries  Q'            --    K'   V'    S^T = K' Q'^T                         O^T   += V'^T Pm^T
//   d/dQ'     queries  Q'            dO    K'   V'    S^T, dPm^T = V' dO^T                  dQ'^T += K'^T dS^T
//   d/dK',V'  keys     K'            V'    Q'   dO    S = Q' K'^T, dPm = dO V'^T            dV'^T += dO^T Pm,  dK'^T += Q'^T dS
//
// with Pm = P .* m (m: stateless dropout keep/(1-p), an explicit mask, or 1; applied AFTER the softmax, never in the row sum)
// and dS = P .* (m .* dPm - D), D[q] = sum_c dO[q,c] O[q,c].
//
// The three passes must see the SAME scores: a dominant entry has P = exp(0) / sum in the forward, and the backward only gets
// that back if its S is bit-identical and L loses nothing.  So (1) the scale multiplies the finished MFMA sum, never an
// operand (a b = b a and both uses walk k in the same order, so the raw sums agree whichever side owns), and (2) L is kept
// as two floats, L = fl(max + log sum) and its rounding residual Lr = (max - L) + log sum; exp((S - L) - Lr) subtracts two
// nearby large numbers exactly first.  With one float, scores near 1e4 would put 5e-4 of noise on every P of the row.
//
// In the D layout of a 16x16 score tile an owner column lives in lane j of the four kq groups: a reduction over the stream
// rows of a tile is 16 in-lane registers plus xor 16 / xor 32 shuffles, and all accumulators of an owner sit in that owner's
// lanes, so the rescale is one per-lane scalar.
//
// Tail-free instances (gt_softmax_attn_nopos_*): head tiles exactly DP = d_k = 16*NF floats wide, for attention without
// coordinate columns (ops.multihead_attention).  The same kernel with the vector-unit tail (ax1 / ax2) and its store compiled
// out; everything above holds unchanged.
//
// Materialised route (need_weights): gt_row_softmax_fwd / _bwd on a score matrix that gt_gemm wrote.
#include "gt_common.h"
#include <algorithm>
#include <cmath>

namespace gt {

struct SoftmaxP {
    const float* F1; const float* F2; const float* T1; const float* T2;
    float* O1; float* O2;
    const float* Oin;            // d/dQ' only: the forward's output, for D
    float* L;                    // [2][B,h,n]: L and its rounding residual; written by the forward, read by the backward passes
    int64_t lplane;              // B*h*n: offset of the residual plane
    float* D;                    // [B,h,n]: written by d/dQ', read by d/dK',V'
    const float* mask;           // explicit multiplicative mask [B,h,n,n] (query-major) or null
    DropDev drop;
    int n, h;
    float scale;
};

constexpr int SM_TS = 64;        // stream rows per LDS tile
constexpr int SM_OW = 32;        // owner rows per wave
constexpr int SM_WIDE_KS = 17;   // DP >= 68: the wide instances (gt_softmax_attn_wide_*)
constexpr float SM_LOG2E = 1.4426950408889634f;
enum { SM_PLAIN = 0, SM_DROP = 1, SM_MASK = 2 };
enum { SM_FWD = 0, SM_BWDQ = 1, SM_BWDKV = 2 };

__device__ __attribute__((aligned(16))) float sm_zero16[4] = {0.f, 0.f, 0.f, 0.f};
__device__ float sm_inf1 = INFINITY;
typedef __attribute__((address_space(3))) void* sm_lds_ptr_t;
typedef const __attribute__((address_space(1))) void* sm_glb_ptr_t;

__device__ __forceinline__ float sm_exp(float x) { return __builtin_amdgcn_exp2f(x * SM_LOG2E); }

// Blocks per CU of an instance (see the kernel's launch bounds).  A tail-free instance (KS a multiple of 4) takes the bound
// of the tailed instance one granule wider: it holds the same fragment, score and MFMA accumulator sets, and under those
// bounds none of them spills (DESIGN 4.14 has the compiler's figures).
constexpr int sm_blocks(int KS, int PASS) {
    const int k = KS % 4 == 0 ? KS + 1 : KS;
    return k >= SM_WIDE_KS ? 1 : PASS == SM_BWDKV ? (k > 5 ? 1 : 2) : (PASS == SM_BWDQ ? (k > 9 ? 1 : 2) : (k > 5 ? 2 : 3));
}

// Head tiles are DP = 16*NF + 4 floats wide (TAIL), or exactly 16*NF (tail-free: KS a multiple of 4); LDS tile image
// [64][DP], linear in float4 granules (gt_fourier.hip).
template <int KS, int PASS, int MODE>
// Blocks per CU: the widest register budget at which no instance spills (d/dK',V' holds four fragment sets, two score tiles
// and two accumulator sets: from DP = 36 on it takes the whole file, AGPRs included).  The wide instances stage 68 / 100 KiB
// of stream tiles per block: at most two blocks fit a CU at DP = 68, one at DP = 100, so they are bounded at one and the
// allocator is free to use AGPRs in every pass.
__global__ __launch_bounds__(256, sm_blocks(KS, PASS))
void softmax_core_kernel(const SoftmaxP p) {
    constexpr bool TAIL = KS % 4 != 0;             // last 4 columns (coordinates + padding) on the vector unit
    constexpr int DP = 4 * KS, NF = DP / 16, XC = 16 * NF, TILE = SM_TS * DP;
    constexpr bool TWO = PASS != SM_FWD;           // two score tiles (S and dPm)
    constexpr bool DUAL = PASS == SM_BWDKV;        // two second products
    static_assert(DP % 16 == 4 || DP % 16 == 0, "head tile width must be 16*NF + 4 or 16*NF");
    __shared__ __attribute__((aligned(16))) float smem[2][2][TILE];
    __shared__ __attribute__((aligned(16))) float sld[2][3][SM_TS];      // d/dK',V': L, D and Lr of the stream rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int head = blockIdx.y, b = blockIdx.z;
    const int o0 = blockIdx.x * (4 * SM_OW) + wave * SM_OW;
    const int64_t hD = (int64_t)p.h * DP;
    const int64_t base = ((int64_t)b * p.n) * hD + (int64_t)head * DP;
    const uint32_t zn = ((uint32_t)b * (uint32_t)p.h + (uint32_t)head) * (uint32_t)p.n;
    const int64_t zrow = ((int64_t)b * p.h + head) * (int64_t)p.n;        // row of L, D, mask
    const int ntile = (p.n + SM_TS - 1) / SM_TS;

    auto issue = [&](int t, int buf) {
        const int s0 = t * SM_TS;
#pragma unroll
        for (int i = 0; i < (KS + 3) / 4; ++i) {
            const int q = wave + 4 * i;                    // 1-KiB chunk (64 float4 granules) of the tile image
            if (q < KS) {
                const int e = q * 64 + lane, r = e / KS, c = e % KS;
                const bool ok = s0 + r < p.n;
                const int64_t off = base + (int64_t)(s0 + r) * hD + 4 * c;
                const float* s1 = ok ? p.T1 + off : sm_zero16;
                const float* s2 = ok ? p.T2 + off : sm_zero16;
                __builtin_amdgcn_global_load_lds((sm_glb_ptr_t)s1, (sm_lds_ptr_t)(&smem[buf][0][q * 256]), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((sm_glb_ptr_t)s2, (sm_lds_ptr_t)(&smem[buf][1][q * 256]), 16, 0, 0);
            }
        }
        if (DUAL && wave < 3) {
            // L (wave 0), D (wave 1) and Lr (wave 2) of the tile's 64 stream rows, one float per lane.  Rows beyond n:
            // L = +inf, so P = exp(0 - inf) = 0 there, and D = Lr = 0
            const bool ok = s0 + lane < p.n;
            const float* src = !ok ? (wave == 0 ? &sm_inf1 : sm_zero16)
                                   : (wave == 1 ? p.D : p.L + (wave == 2 ? p.lplane : 0)) + zrow + s0 + lane;
            __builtin_amdgcn_global_load_lds((sm_glb_ptr_t)src, (sm_lds_ptr_t)(&sld[buf][wave][0]), 4, 0, 0);
        }
    };
    issue(0, 0);

    // owner fragments: B operand of the first product(s), lane (j, kq) holds F[owner j][4s + kq]
    float f1[2][KS], f2[TWO ? 2 : 1][TWO ? KS : 1];
    float own_l[2] = {0.f, 0.f}, own_r[2] = {0.f, 0.f}, own_d[2] = {0.f, 0.f};      // owner = query: its L, Lr and D
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int o = o0 + 16 * nt + j, oc = min(o, p.n - 1);
        const float live = (o < p.n) ? 1.f : 0.f;
        float dpart = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            f1[nt][s] = live * p.F1[base + (int64_t)oc * hD + 4 * s + kq];
            if (TWO) f2[nt][s] = live * p.F2[base + (int64_t)oc * hD + 4 * s + kq];
            if (PASS == SM_BWDQ) dpart += f2[nt][s] * p.Oin[base + (int64_t)oc * hD + 4 * s + kq];
        }
        if (PASS == SM_BWDQ) {
            dpart += __shfl_xor(dpart, 16, 64);
            dpart += __shfl_xor(dpart, 32, 64);
            own_d[nt] = dpart;
            own_l[nt] = p.L[zrow + oc];
            own_r[nt] = p.L[p.lplane + zrow + oc];
            if (kq == 0 && o < p.n) p.D[zrow + o] = dpart;
        }
    }
    // dropout hash carriers: hw[nt] = idx*G + key of (first stream row of this lane in the tile, owner nt)
    constexpr uint32_t G = 0x9e3779b1u;
    uint32_t hw[2] = {0u, 0u}, hstep = 0u;
    if (MODE == SM_DROP) {
        const uint32_t key = drop_key_dev(p.drop);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const uint32_t ow = (uint32_t)(o0 + 16 * nt + j), st = 4u * (uint32_t)kq;
            const uint32_t idx = DUAL ? (zn + st) * (uint32_t)p.n + ow : (zn + ow) * (uint32_t)p.n + st;
            hw[nt] = idx * G + key;
        }
        hstep = DUAL ? (uint32_t)p.n * G : G;                // idx step per stream row, times G
    }

    f32x4 acc1[NF][2], acc2[DUAL ? NF : 1][2];
    f32x2 ax1[2][2], ax2[2][2];                              // last 4 columns: [nt][column pair], partial over kq
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int dt = 0; dt < NF; ++dt) {
            acc1[dt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (DUAL) acc2[dt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (TAIL) ax1[nt][0] = ax1[nt][1] = ax2[nt][0] = ax2[nt][1] = f32x2{0.f, 0.f};
    }
    float run_m[2] = {-INFINITY, -INFINITY}, run_l[2] = {0.f, 0.f};      // forward: running maximum and sum per owner

    for (int t = 0; t < ntile; ++t) {
        // tile t has landed for this wave (vmcnt) and for everybody (barrier); everybody is also done with
        // tile t-1, whose buffer the next request overwrites
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (t + 1 < ntile) issue(t + 1, (t + 1) & 1);
        const float* t1 = smem[t & 1][0];
        const float* t2 = smem[t & 1][1];
        const int s0 = t * SM_TS;

        // first product(s): sa = S, sb = dPm (stream rows x owner columns), 4 row tiles x 2 column tiles per wave
        f32x4 sa[4][2], sb[TWO ? 4 : 1][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                sa[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (TWO) sb[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float a1 = t1[(16 * mt + j) * DP + 4 * s + kq];
                float a2 = 0.f;
                if (TWO) a2 = t2[(16 * mt + j) * DP + 4 * s + kq];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    sa[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, f1[nt][s], sa[mt][nt], 0, 0, 0);
                    if (TWO) sb[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, f2[nt][s], sb[mt][nt], 0, 0, 0);
                }
            }
        // element (stream row s0 + 16mt + 4kq + r, owner column o0 + 16nt + j).  Stream rows at or beyond n are zero-filled:
        // they score 0, not -inf, and are taken out explicitly
        const bool partial = s0 + SM_TS > p.n;
        {
            // on the finished sum, as a ROUNDED product: were it contracted into an fma with the subtraction behind it, a
            // dominant entry would see its own rounding residual (5e-4 at scores near 1e4) instead of exp(0)
#pragma clang fp contract(off)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) sa[mt][nt] = sa[mt][nt] * p.scale;
        }
        if (PASS == SM_FWD) {
            if (partial) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (s0 + 16 * mt + 4 * kq + r >= p.n) sa[mt][0][r] = sa[mt][1][r] = -INFINITY;
            }
            // online softmax: the tile's column maximum (every tile has a live row, so it is finite), the rescale of what
            // has been accumulated, the exponentials and their sum
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                float mx = -INFINITY;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sa[mt][nt][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mnew = fmaxf(run_m[nt], mx);
                const float alpha = sm_exp(run_m[nt] - mnew);           // first tile: exp(-inf) = 0
                run_m[nt] = mnew;
                float sum = 0.f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = sm_exp(sa[mt][nt][r] - mnew);
                        sa[mt][nt][r] = e;
                        sum += e;
                    }
                sum += __shfl_xor(sum, 16, 64);
                sum += __shfl_xor(sum, 32, 64);
                run_l[nt] = run_l[nt] * alpha + sum;
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) acc1[dt][nt] *= alpha;
                if (TAIL) {
                    ax1[nt][0] *= alpha;
                    ax1[nt][1] *= alpha;
                }
            }
        } else {
            // P = exp(S - L) from the saved row statistic
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * mt + 4 * kq + r;
                    const bool live = !partial || s0 + row < p.n;
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const float l = DUAL ? sld[t & 1][0][row] : own_l[nt];
                        const float lr = DUAL ? sld[t & 1][2][row] : own_r[nt];
                        const float e = sm_exp((sa[mt][nt][r] - l) - lr);
                        sa[mt][nt][r] = live ? e : 0.f;
                    }
                }
        }
        // mask m on P (after the exponential); backward: sa = Pm (d/dK',V' only needs it), sb = dS = P (m dPm - D)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            uint32_t hk = hw[nt];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float m = 1.f;
                    if (MODE == SM_DROP) {
                        m = fmix32(hk) >= p.drop.thresh ? p.drop.scale : 0.f;
                        hk += hstep;
                    } else if (MODE == SM_MASK) {
                        const int st = min(s0 + 16 * mt + 4 * kq + r, p.n - 1), ow = min(o0 + 16 * nt + j, p.n - 1);
                        const int qi = DUAL ? st : ow, ki = DUAL ? ow : st;
                        m = p.mask[(zrow + qi) * (int64_t)p.n + ki];
                    }
                    const float pr = sa[mt][nt][r];
                    if (TWO) {
                        const float dd = DUAL ? sld[t & 1][1][16 * mt + 4 * kq + r] : own_d[nt];
                        sb[mt][nt][r] = pr * (m * sb[mt][nt][r] - dd);
                    }
                    if (MODE != SM_PLAIN) sa[mt][nt][r] = pr * m;
                }
                hk += 12u * hstep;
            }
            hw[nt] = hk;                                      // advanced by 64 stream rows
        }
        // second product(s): O^T (dims x owners) += U^T (dims x stream) * W (stream x owners); k-step s of row tile mt
        // contracts stream row 16mt + 4kq + s = accumulator register s of this lane.
        //   forward: U = V' (T2), W = Pm;  d/dQ': U = K' (T1), W = dS;  d/dK',V': U = dO (T2), W = Pm and U = Q' (T1), W = dS
        const float* u1 = PASS == SM_BWDQ ? t1 : t2;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = 16 * mt + 4 * kq + s;
                const float w1[2] = {PASS == SM_BWDQ ? sb[mt][0][s] : sa[mt][0][s], PASS == SM_BWDQ ? sb[mt][1][s] : sa[mt][1][s]};
#pragma unroll
                for (int dt = 0; dt < NF; ++dt) {
                    const float a1 = u1[row * DP + 16 * dt + j];
                    float a2 = 0.f;
                    if (DUAL) a2 = t1[row * DP + 16 * dt + j];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc1[dt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w1[nt], acc1[dt][nt], 0, 0, 0);
                        if (DUAL)
                            acc2[dt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, sb[mt][nt][s], acc2[dt][nt], 0, 0, 0);
                    }
                }
                if (!TAIL) continue;
                // last 4 columns on the vector unit: this lane's stream row `row`, its owner columns
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(&u1[row * DP + XC]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float sv = w1[nt];
                    ax1[nt][0] += f32x2{sv, sv} * f32x2{x1[0], x1[1]};
                    ax1[nt][1] += f32x2{sv, sv} * f32x2{x1[2], x1[3]};
                }
                if (DUAL) {
                    const f32x4 x2 = *reinterpret_cast<const f32x4*>(&t1[row * DP + XC]);
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const float sv = sb[mt][nt][s];
                        ax2[nt][0] += f32x2{sv, sv} * f32x2{x2[0], x2[1]};
                        ax2[nt][1] += f32x2{sv, sv} * f32x2{x2[2], x2[3]};
                    }
                }
            }
        }
    }
    // O^T tile (dt, nt): rows = dims 16dt + 4kq + r, column = owner o0 + 16nt + j  ->  O[owner][dim..dim+3]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int ow = o0 + 16 * nt + j;
        // forward: 1 / row sum;  d/dQ': the score scale;  d/dK',V': 1 for dV', the score scale for dK'
        const float e1 = PASS == SM_FWD ? 1.f / run_l[nt] : (PASS == SM_BWDQ ? p.scale : 1.f);
#pragma unroll
        for (int dt = 0; dt < NF; ++dt)
            if (ow < p.n) {
                const int dim = 16 * dt + 4 * kq;
                *reinterpret_cast<f32x4*>(p.O1 + base + (int64_t)ow * hD + dim) = acc1[dt][nt] * e1;
                if (DUAL) *reinterpret_cast<f32x4*>(p.O2 + base + (int64_t)ow * hD + dim) = acc2[dt][nt] * p.scale;
            }
        if (!TAIL) {      // no tail store to ride on: lane kq == 0 writes the forward's row statistic
            if (PASS == SM_FWD && kq == 0 && ow < p.n) {
                const float lg = logf(run_l[nt]), lv = run_m[nt] + lg;
                p.L[zrow + ow] = lv;
                p.L[p.lplane + zrow + ow] = (run_m[nt] - lv) + lg;
            }
            continue;
        }
        // last 4 columns: sum the four kq partials (lanes j, j+16, j+32, j+48), lane kq == 0 stores
        f32x4 v1 = {ax1[nt][0][0], ax1[nt][0][1], ax1[nt][1][0], ax1[nt][1][1]};
        f32x4 v2 = {ax2[nt][0][0], ax2[nt][0][1], ax2[nt][1][0], ax2[nt][1][1]};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v1[c] += __shfl_xor(v1[c], 16, 64);
            v1[c] += __shfl_xor(v1[c], 32, 64);
            if (DUAL) {
                v2[c] += __shfl_xor(v2[c], 16, 64);
                v2[c] += __shfl_xor(v2[c], 32, 64);
            }
        }
        if (kq == 0 && ow < p.n) {
            *reinterpret_cast<f32x4*>(p.O1 + base + (int64_t)ow * hD + XC) = v1 * e1;
            if (DUAL) *reinterpret_cast<f32x4*>(p.O2 + base + (int64_t)ow * hD + XC) = v2 * p.scale;
            if (PASS == SM_FWD) {
                const float lg = logf(run_l[nt]), lv = run_m[nt] + lg;
                p.L[zrow + ow] = lv;
                p.L[p.lplane + zrow + ow] = (run_m[nt] - lv) + lg;
            }
        }
    }
}

template <int KS, int PASS>
static void softmax_launch(const SoftmaxP& p, dim3 grid, hipStream_t st) {
    const int mode = p.mask ? SM_MASK : (p.drop.thresh ? SM_DROP : SM_PLAIN);
#define GT_SM(M) hipLaunchKernelGGL((softmax_core_kernel<KS, PASS, M>), grid, dim3(256), 0, st, p)
    if (mode == SM_DROP) GT_SM(SM_DROP);
    else if (mode == SM_MASK) GT_SM(SM_MASK);
    else GT_SM(SM_PLAIN);
#undef GT_SM
}

// SET selects the instance set of the entry point: DP in {20, 36, 52} (gt_softmax_attn_*), {68, 100} (gt_softmax_attn_wide_*)
// or the tail-free {16, 32, 48, 64, 96} (gt_softmax_attn_nopos_*).
enum { SM_NARROW = 0, SM_WIDE = 1, SM_NOPOS = 2 };
template <int PASS, int SET>
static int softmax_attn(SoftmaxP p, int32_t B, int32_t DP, const gt_dropout* drop, void* stream) {
    if (!p.F1 || !p.T1 || !p.T2 || !p.O1 || !p.L || B <= 0 || p.n <= 0 || p.h <= 0 || DP <= 0) return GT_EINVAL;
    if (PASS != SM_FWD && (!p.F2 || !p.D)) return GT_EINVAL;
    if (PASS == SM_BWDQ && !p.Oin) return GT_EINVAL;
    if (PASS == SM_BWDKV && !p.O2) return GT_EINVAL;
    if (drop && drop->p > 0.f && !drop->seed) return GT_EINVAL;
    if (B > 65535 || p.h > 65535) return GT_EINVAL;
    if (misaligned16(p.T1, p.T2, p.O1, p.O2)) return GT_EALIGN;
    if (misaligned<4>(p.L, p.D)) return GT_EALIGN;
    p.drop = make_drop(p.mask ? nullptr : drop);
    p.lplane = (int64_t)B * p.h * p.n;
    dim3 grid((unsigned)ceil_div(p.n, 4 * SM_OW), (unsigned)p.h, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (SET == SM_NOPOS) {
        switch (DP) {
            case 16: softmax_launch<4, PASS>(p, grid, st); break;
            case 32: softmax_launch<8, PASS>(p, grid, st); break;
            case 48: softmax_launch<12, PASS>(p, grid, st); break;
            case 64: softmax_launch<16, PASS>(p, grid, st); break;
            case 96: softmax_launch<24, PASS>(p, grid, st); break;
            default: return GT_ENOTSUP;
        }
    } else if (SET == SM_WIDE) {
        switch (DP) {
            case 68: softmax_launch<17, PASS>(p, grid, st); break;
            case 100: softmax_launch<25, PASS>(p, grid, st); break;
            default: return GT_ENOTSUP;
        }
    } else {
        switch (DP) {
            case 20: softmax_launch<5, PASS>(p, grid, st); break;
            case 36: softmax_launch<9, PASS>(p, grid, st); break;
            case 52: softmax_launch<13, PASS>(p, grid, st); break;
            default: return GT_ENOTSUP;
        }
    }
    GT_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ materialised route
// One wave per row of the [rows][n] score matrix, four rows per block.  Mask index of element (row, k): (row0 + row)*n + k,
// i.e. ((b*h+head)*n + query)*n + key for the dense [B,h,n,n] tensor with row0 = 0 -- the index of the fused route.
template <bool BWD>
__global__ __launch_bounds__(256) void row_softmax_kernel(const float* X, const float* G_,
                                                          float* Y, float* Ym, int64_t rows, int n,
                                                          int64_t row0, const float* mask, const DropDev drop) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t off = row * n;
    const uint32_t key = drop_key_dev(drop);
    const uint32_t i0 = (uint32_t)(row0 + row) * (uint32_t)n;
    auto mval = [&](int k) -> float {
        if (mask) return mask[off + k];
        if (drop.thresh) return drop_mul(drop, key, i0 + (uint32_t)k);
        return 1.f;
    };
    if (!BWD) {
        // X = S: stable maximum-subtracted softmax; Y = P, Ym = P .* m
        float mx = -INFINITY;
        for (int k = lane; k < n; k += 64) mx = fmaxf(mx, X[off + k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.f;
        for (int k = lane; k < n; k += 64) sum += sm_exp(X[off + k] - mx);
        sum = wave_sum(sum);
        const float inv = 1.f / sum;
        for (int k = lane; k < n; k += 64) {
            const float pr = sm_exp(X[off + k] - mx) * inv;
            const float pm = pr * mval(k);
            Y[off + k] = pr;
            if (Ym != Y) Ym[off + k] = pm;
        }
    } else {
        // X = P, G_ = dPm: Y = dS = P .* (m .* dPm - sum_k P m dPm)
        float dot = 0.f;
        for (int k = lane; k < n; k += 64) dot += X[off + k] * (mval(k) * G_[off + k]);
        dot = wave_sum(dot);
        for (int k = lane; k < n; k += 64) Y[off + k] = X[off + k] * (mval(k) * G_[off + k] - dot);
    }
}

}  // namespace gt

using namespace gt;

extern "C" int gt_softmax_attn_fwd(const float* Q, const float* K, const float* V, float* O, float* L, int32_t B, int32_t n,
                                   int32_t h, int32_t DP, float scale, const float* mask, const gt_dropout* drop,
                                   void* stream) {
    SoftmaxP p{Q, nullptr, K, V, O, nullptr, nullptr, L, 0, nullptr, mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_FWD, SM_NARROW>(p, B, DP, drop, stream);
}

extern "C" int gt_softmax_attn_bwd_q(const float* dO, const float* O, const float* Q, const float* K, const float* V,
                                     const float* L, float* D, float* dQ, int32_t B, int32_t n, int32_t h, int32_t DP,
                                     float scale, const float* mask, const gt_dropout* drop, void* stream) {
    SoftmaxP p{Q, dO, K, V, dQ, nullptr, O, const_cast<float*>(L), 0, D, mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_BWDQ, SM_NARROW>(p, B, DP, drop, stream);
}

extern "C" int gt_softmax_attn_bwd_kv(const float* K, const float* V, const float* Q, const float* dO, const float* L,
                                      const float* D, float* dK, float* dV, int32_t B, int32_t n, int32_t h, int32_t DP,
                                      float scale, const float* mask, const gt_dropout* drop, void* stream) {
    SoftmaxP p{K, V, Q, dO, dV, dK, nullptr, const_cast<float*>(L), 0, const_cast<float*>(D), mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_BWDKV, SM_NARROW>(p, B, DP, drop, stream);
}

// The same three passes at DP = 68 / 100: entry points of their own, so that the narrow ones keep answering GT_ENOTSUP there.
extern "C" int gt_softmax_attn_wide_fwd(const float* Q, const float* K, const float* V, float* O, float* L, int32_t B, int32_t n,
                                        int32_t h, int32_t DP, float scale, const float* mask, const gt_dropout* drop,
                                        void* stream) {
    SoftmaxP p{Q, nullptr, K, V, O, nullptr, nullptr, L, 0, nullptr, mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_FWD, SM_WIDE>(p, B, DP, drop, stream);
}

extern "C" int gt_softmax_attn_wide_bwd_q(const float* dO, const float* O, const float* Q, const float* K, const float* V,
                                          const float* L, float* D, float* dQ, int32_t B, int32_t n, int32_t h, int32_t DP,
                                          float scale, const float* mask, const gt_dropout* drop, void* stream) {
    SoftmaxP p{Q, dO, K, V, dQ, nullptr, O, const_cast<float*>(L), 0, D, mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_BWDQ, SM_WIDE>(p, B, DP, drop, stream);
}

extern "C" int gt_softmax_attn_wide_bwd_kv(const float* K, const float* V, const float* Q, const float* dO, const float* L,
                                           const float* D, float* dK, float* dV, int32_t B, int32_t n, int32_t h, int32_t DP,
                                           float scale, const float* mask, const gt_dropout* drop, void* stream) {
    SoftmaxP p{K, V, Q, dO, dV, dK, nullptr, const_cast<float*>(L), 0, const_cast<float*>(D), mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_BWDKV, SM_WIDE>(p, B, DP, drop, stream);
}

// The same three passes on tail-free head tiles, DP = d_k in {16, 32, 48, 64, 96}: no coordinate and no pad columns.
extern "C" int gt_softmax_attn_nopos_fwd(const float* Q, const float* K, const float* V, float* O, float* L, int32_t B, int32_t n,
                                         int32_t h, int32_t DP, float scale, const float* mask, const gt_dropout* drop,
                                         void* stream) {
    SoftmaxP p{Q, nullptr, K, V, O, nullptr, nullptr, L, 0, nullptr, mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_FWD, SM_NOPOS>(p, B, DP, drop, stream);
}

extern "C" int gt_softmax_attn_nopos_bwd_q(const float* dO, const float* O, const float* Q, const float* K, const float* V,
                                           const float* L, float* D, float* dQ, int32_t B, int32_t n, int32_t h, int32_t DP,
                                           float scale, const float* mask, const gt_dropout* drop, void* stream) {
    SoftmaxP p{Q, dO, K, V, dQ, nullptr, O, const_cast<float*>(L), 0, D, mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_BWDQ, SM_NOPOS>(p, B, DP, drop, stream);
}

extern "C" int gt_softmax_attn_nopos_bwd_kv(const float* K, const float* V, const float* Q, const float* dO, const float* L,
                                            const float* D, float* dK, float* dV, int32_t B, int32_t n, int32_t h, int32_t DP,
                                            float scale, const float* mask, const gt_dropout* drop, void* stream) {
    SoftmaxP p{K, V, Q, dO, dV, dK, nullptr, const_cast<float*>(L), 0, const_cast<float*>(D), mask, DropDev{}, n, h, scale};
    return softmax_attn<SM_BWDKV, SM_NOPOS>(p, B, DP, drop, stream);
}

static int row_softmax_check(const void* a, const void* b, int64_t rows, int32_t n, const gt_dropout* drop) {
    if (!a || !b || rows <= 0 || n <= 0 || (rows + 3) / 4 > 0x7fffffffLL) return GT_EINVAL;
    if (drop && drop->p > 0.f && !drop->seed) return GT_EINVAL;
    return 0;
}

extern "C" int gt_row_softmax_fwd(const float* S, float* P, float* Pm, int64_t rows, int32_t n, int64_t row0,
                                  const float* mask, const gt_dropout* drop, void* stream) {
    if (int rc = row_softmax_check(S, P, rows, n, drop)) return rc;
    if (!Pm) return GT_EINVAL;
    hipLaunchKernelGGL((row_softmax_kernel<false>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, S,
                       (const float*)nullptr, P, Pm, rows, n, row0, mask, make_drop(mask ? nullptr : drop));
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_row_softmax_bwd(const float* P, const float* dPm, float* dS, int64_t rows, int32_t n, int64_t row0,
                                  const float* mask, const gt_dropout* drop, void* stream) {
    if (int rc = row_softmax_check(P, dPm, rows, n, drop)) return rc;
    if (!dS) return GT_EINVAL;
    hipLaunchKernelGGL((row_softmax_kernel<true>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P, dPm,
                       dS, (float*)nullptr, rows, n, row0, mask, make_drop(mask ? nullptr : drop));
    GT_LAUNCH_CHECK();
    return 0;
}
