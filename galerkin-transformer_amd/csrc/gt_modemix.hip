// Spectral complex mode mixing (gfx950), forward and backward: Y[b][q][o] = sum_i X[b][q][i] W[i][o][q] over the retained
// modes q.  Two kernel families, picked per direction by modemix_plan (the launchers and the workspace query all ask it):
//   resident  one block per mode and batch slice, the whole [Cin][Cout] weight slice of the mode in LDS; the backward keeps
//             its weight-gradient pairs in registers (Cin * Cout <= 6144).  The narrow layers of the shipped models.
//   tiled     any width: a block owns four adjacent modes and one tile of output channels, the contraction axis goes
//             through LDS in chunks; LDS and registers are set by the tile constants alone.
// The weight gradient is accumulated per batch slice; gt_slab_reduce sums the slices in a fixed order.
#include "gt_common.h"

namespace gt {

// One block per retained mode q.  X: [B][2][Qx][Cin], Y: [B][2][Qy][Cout] (re plane, im plane),
// W: [Cin][Cout][Q][2].  Complex product, no conjugate (layers.py:1143-1151).
constexpr int MM_BCH = 8;   // batch entries staged per pass
__global__ __launch_bounds__(256) void modemix_fwd_kernel(const float* __restrict__ X,
                                                          const float* __restrict__ W, int B, int Q,
                                                          int Cin, int Cout, int64_t xbs, int64_t ybs,
                                                          int Qx, int Qy, int qoff,
                                                          float* __restrict__ Y) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sWr = lds;                       // [Cin][Cout]
    float* sWi = sWr + Cin * Cout;          // [Cin][Cout]
    float* sX = sWi + Cin * Cout;           // [MM_BCH][2][Cin]
    const int q = blockIdx.x;
    for (int e = threadIdx.x; e < Cin * Cout; e += blockDim.x) {
        const float2 w = *reinterpret_cast<const float2*>(W + ((int64_t)e * Q + q) * 2);
        sWr[e] = w.x;
        sWi[e] = w.y;
    }
    // the batch is cut into gridDim.y slices: Q = m*m blocks alone (144 for the Darcy decoder) leave the chip half empty
    const int bchunk = (B + gridDim.y - 1) / gridDim.y;
    const int bend = min(B, (int)(blockIdx.y + 1) * bchunk);
    for (int bb = blockIdx.y * bchunk; bb < bend; bb += MM_BCH) {
        const int nb = min(MM_BCH, bend - bb);
        __syncthreads();
        for (int e = threadIdx.x; e < nb * 2 * Cin; e += blockDim.x) {
            const int b = e / (2 * Cin), ri = (e / Cin) & 1, i = e % Cin;
            sX[e] = X[(int64_t)(bb + b) * xbs + ((int64_t)ri * Qx + qoff + q) * Cin + i];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nb * Cout; e += blockDim.x) {
            const int b = e / Cout, o = e % Cout;
            const float* xr = sX + b * 2 * Cin;
            const float* xi = xr + Cin;
            float yr = 0.f, yi = 0.f;
            for (int i = 0; i < Cin; ++i) {
                const float wr = sWr[i * Cout + o], wi = sWi[i * Cout + o];
                yr = fmaf(xr[i], wr, yr); yr = fmaf(-xi[i], wi, yr);
                yi = fmaf(xi[i], wr, yi); yi = fmaf(xr[i], wi, yi);
            }
            float* yp = Y + (int64_t)(bb + b) * ybs + ((int64_t)qoff + q) * Cout + o;
            yp[0] = yr;
            yp[(int64_t)Qy * Cout] = yi;
        }
    }
}

template <int MAXP>      // (i, o) weight-gradient pairs per thread: Cin * Cout <= 256 * MAXP
__global__ __launch_bounds__(256) void modemix_bwd_kernel(
    const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ dY, int B, int Q,
    int Cin, int Cout, int64_t xbs, int64_t ybs, int Qx, int Qy, int qoff, float* __restrict__ dX,
    float* __restrict__ dW) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // weight rows padded by one float: the dX loop below reads W[i][o] with the lanes running over i -- at a row pitch of
    // Cout = 32 floats every lane of a wave hit the same LDS bank (a 32-way conflict on both reads of each of the Cout steps)
    const int CW = Cout + 1;
    float* sWr = lds;                       // [Cin][Cout + 1]
    float* sWi = sWr + Cin * CW;
    float* sX = sWi + Cin * CW;             // [MM_BCH][2][Cin]
    float* sG = sX + MM_BCH * 2 * Cin;      // [MM_BCH][2][Cout]
    const int q = blockIdx.x;
    for (int e = threadIdx.x; e < Cin * Cout; e += blockDim.x) {
        const float2 w = *reinterpret_cast<const float2*>(W + ((int64_t)e * Q + q) * 2);
        const int i = e / Cout, o = e - i * Cout;
        sWr[i * CW + o] = w.x;
        sWi[i * CW + o] = w.y;
    }
    // each thread owns up to MAXP (i,o) pairs of dW, accumulated over the whole batch in registers
    float gr[MAXP], gi[MAXP];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) gr[k] = gi[k] = 0.f;
    const int bchunk = (B + gridDim.y - 1) / gridDim.y;      // batch slice of this block (dW: one partial per slice)
    const int bend = min(B, (int)(blockIdx.y + 1) * bchunk);
    for (int bb = blockIdx.y * bchunk; bb < bend; bb += MM_BCH) {
        const int nb = min(MM_BCH, bend - bb);
        __syncthreads();
        for (int e = threadIdx.x; e < nb * 2 * Cin; e += blockDim.x) {
            const int b = e / (2 * Cin), ri = (e / Cin) & 1, i = e % Cin;
            sX[e] = X[(int64_t)(bb + b) * xbs + ((int64_t)ri * Qx + qoff + q) * Cin + i];
        }
        for (int e = threadIdx.x; e < nb * 2 * Cout; e += blockDim.x) {
            const int b = e / (2 * Cout), ri = (e / Cout) & 1, o = e % Cout;
            sG[e] = dY[(int64_t)(bb + b) * ybs + ((int64_t)ri * Qy + qoff + q) * Cout + o];
        }
        __syncthreads();
        // dX[b][.][q][i] = sum_o dY (x) conj(W)
        for (int e = threadIdx.x; e < nb * Cin; e += blockDim.x) {
            const int b = e / Cin, i = e % Cin;
            const float* g_r = sG + b * 2 * Cout;
            const float* g_i = g_r + Cout;
            float xr = 0.f, xi = 0.f;
            for (int o = 0; o < Cout; ++o) {
                const float wr = sWr[i * CW + o], wi = sWi[i * CW + o];
                xr = fmaf(g_r[o], wr, xr); xr = fmaf(g_i[o], wi, xr);
                xi = fmaf(g_i[o], wr, xi); xi = fmaf(-g_r[o], wi, xi);
            }
            float* xp = dX + (int64_t)(bb + b) * xbs + ((int64_t)qoff + q) * Cin + i;
            xp[0] = xr;
            xp[(int64_t)Qx * Cin] = xi;
        }
        // dW[i][o] += sum_b conj(X) (x) dY
#pragma unroll
        for (int k = 0; k < MAXP; ++k) {
            const int e = threadIdx.x + k * 256;
            if (e < Cin * Cout) {
                const int i = e / Cout, o = e % Cout;
                for (int b = 0; b < nb; ++b) {
                    const float xr = sX[b * 2 * Cin + i], xi = sX[b * 2 * Cin + Cin + i];
                    const float g_r = sG[b * 2 * Cout + o], g_i = sG[b * 2 * Cout + Cout + o];
                    gr[k] = fmaf(xr, g_r, gr[k]); gr[k] = fmaf(xi, g_i, gr[k]);
                    gi[k] = fmaf(xr, g_i, gi[k]); gi[k] = fmaf(-xi, g_r, gi[k]);
                }
            }
        }
    }
    float* dWs = dW + (int64_t)blockIdx.y * Cin * Cout * Q * 2;       // slab of this batch slice (gridDim.y == 1: dW itself)
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
        const int e = threadIdx.x + k * 256;
        if (e < Cin * Cout)
            *reinterpret_cast<float2*>(dWs + ((int64_t)e * Q + q) * 2) = make_float2(gr[k], gi[k]);
    }
}

// ------------------------------------------------------------------------------------------
// Tiled family.  LDS and registers depend on the constants below only, never on Cin / Cout.
// ------------------------------------------------------------------------------------------
constexpr int MT_QT = 4;    // adjacent modes of a block: one (i, o) weight element of them is 32 contiguous bytes of W
constexpr int MT_BT = 8;    // batch entries of a block (apply) / staged per pass (weight gradient)
constexpr int MT_TT = 32;   // apply: output channels of a block
constexpr int MT_SC = 16;   // apply: contraction channels per LDS chunk
constexpr int MT_IT = 32;   // weight gradient: Cin tile
constexpr int MT_OT = 32;   // weight gradient: Cout tile

// Out[b][q][t] = sum_s In[b][q][s] (x) Wc(s, t, q) for the block's 8 samples x 4 modes x 32 output channels.
//   CONJ = false (forward):        In = X,  s = i, t = o, Wc = W[s][t][q]
//   CONJ = true  (data gradient):  In = dY, s = o, t = i, Wc = conj(W[t][s][q])
// grid.x = (mode group, t tile), grid.y = batch tile.  Each weight element of the block's tile is read once; the next
// chunk's global loads are issued ahead of the current chunk's products.  A thread owns (t, q) and 4 samples.
template <bool CONJ>
__global__ __launch_bounds__(256) void modemix_tiled_apply_kernel(
    const float* __restrict__ In, const float* __restrict__ W, int B, int Q, int S, int T, int Cout, int64_t ibs,
    int64_t obs, int Qi, int Qo, int qoff, int ntile, float* __restrict__ Out) {
    // weight chunk: element (q, s, t) at q * PL + s * SS + t * ST (float2).  The lanes read along t and store along
    // (q, t) [forward] or (q, s) [CONJ: s is the contiguous axis of W there]; ST = 34 and PL = 16 mod 64 keep both free of
    // bank conflicts.
    constexpr int SS = CONJ ? 2 : MT_TT * 2;
    constexpr int ST = CONJ ? MT_SC * 2 + 2 : 2;
    constexpr int PL = (CONJ ? MT_TT * ST : MT_SC * SS) + 16;
    constexpr int NW = MT_QT * MT_SC * MT_TT / 256;          // float2 weight loads of a thread per chunk (8)
    constexpr int NX = MT_BT * 2 * MT_QT * MT_SC / 256;      // input loads of a thread per chunk (4)
    __shared__ __attribute__((aligned(16))) float sW[MT_QT * PL];
    __shared__ __attribute__((aligned(16))) float sIn[MT_QT * MT_SC * MT_BT * 2];      // [q][s][b][re, im]
    const int tid = threadIdx.x;
    const int q0 = (int)(blockIdx.x / ntile) * MT_QT, t0 = (int)(blockIdx.x % ntile) * MT_TT, b0 = blockIdx.y * MT_BT;

    float2 wreg[NW];
    float xreg[NX];
    auto fetch = [&](int s0) {
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int e = tid + k * 256;
            const int q = e % MT_QT;
            const int s = CONJ ? (e / MT_QT) % MT_SC : e / (MT_QT * MT_TT);
            const int t = CONJ ? e / (MT_QT * MT_SC) : (e / MT_QT) % MT_TT;
            wreg[k] = make_float2(0.f, 0.f);
            if (q0 + q < Q && s0 + s < S && t0 + t < T) {
                const int64_t io = CONJ ? (int64_t)(t0 + t) * Cout + (s0 + s) : (int64_t)(s0 + s) * Cout + (t0 + t);
                wreg[k] = *reinterpret_cast<const float2*>(W + (io * Q + q0 + q) * 2);
            }
        }
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const int e = tid + k * 256;
            const int s = e % MT_SC, q = (e / MT_SC) % MT_QT, ri = (e / (MT_SC * MT_QT)) & 1, b = e / (MT_SC * MT_QT * 2);
            xreg[k] = 0.f;
            if (b0 + b < B && q0 + q < Q && s0 + s < S)
                xreg[k] = In[(int64_t)(b0 + b) * ibs + ((int64_t)ri * Qi + qoff + q0 + q) * S + s0 + s];
        }
    };

    const int t = tid % MT_TT, q = (tid / MT_TT) % MT_QT, bh = tid / (MT_TT * MT_QT);      // samples bh * 4 .. bh * 4 + 3
    float yr[4] = {0.f, 0.f, 0.f, 0.f}, yi[4] = {0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int s0 = 0; s0 < S; s0 += MT_SC) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int e = tid + k * 256;
            const int wq = e % MT_QT;
            const int ws = CONJ ? (e / MT_QT) % MT_SC : e / (MT_QT * MT_TT);
            const int wt = CONJ ? e / (MT_QT * MT_SC) : (e / MT_QT) % MT_TT;
            *reinterpret_cast<float2*>(sW + wq * PL + ws * SS + wt * ST) = wreg[k];
        }
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const int e = tid + k * 256;
            const int xs = e % MT_SC, xq = (e / MT_SC) % MT_QT, ri = (e / (MT_SC * MT_QT)) & 1, b = e / (MT_SC * MT_QT * 2);
            sIn[((xq * MT_SC + xs) * MT_BT + b) * 2 + ri] = xreg[k];
        }
        __syncthreads();
        if (s0 + MT_SC < S) fetch(s0 + MT_SC);
#pragma unroll
        for (int s = 0; s < MT_SC; ++s) {
            const float2 w = *reinterpret_cast<const float2*>(sW + q * PL + s * SS + t * ST);
            const float wr = w.x, wi = CONJ ? -w.y : w.y;
            const f32x4* xp = reinterpret_cast<const f32x4*>(sIn + ((q * MT_SC + s) * MT_BT + bh * 4) * 2);
            const f32x4 xa = xp[0], xb = xp[1];
            const float xr[4] = {xa[0], xa[2], xb[0], xb[2]}, xi[4] = {xa[1], xa[3], xb[1], xb[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                yr[j] = fmaf(xr[j], wr, yr[j]); yr[j] = fmaf(-xi[j], wi, yr[j]);
                yi[j] = fmaf(xi[j], wr, yi[j]); yi[j] = fmaf(xr[j], wi, yi[j]);
            }
        }
    }
    if (q0 + q < Q && t0 + t < T) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = b0 + bh * 4 + j;
            if (b < B) {
                float* op = Out + (int64_t)b * obs + ((int64_t)qoff + q0 + q) * T + t0 + t;
                op[0] = yr[j];
                op[(int64_t)Qo * T] = yi[j];
            }
        }
    }
}

// dW[i][o][q] = sum_b conj(X[b][q][i]) (x) dY[b][q][o] for the block's 4 modes x (32 x 32) channel tile, summed over the batch
// slice blockIdx.y (one dW slab per slice, gridDim.y == 1: dW itself).  grid.x = (mode group, Cin tile, Cout tile).
// A thread owns (q, o) and 16 consecutive i: 16 complex sums.  The lanes run over (q, o), so a wave's stores are runs of 32
// contiguous bytes, as its W reads are in the apply kernel.
__global__ __launch_bounds__(256) void modemix_tiled_wgrad_kernel(
    const float* __restrict__ X, const float* __restrict__ dY, int B, int Q, int Cin, int Cout, int64_t xbs, int64_t ybs,
    int Qx, int Qy, int qoff, int nit, int notile, float* __restrict__ dW) {
    constexpr int XS = 2 * MT_IT + 4;      // sX row of one (b, q): [re | im][32 i] + 4: the wave's 4 modes read 4 different banks
    constexpr int GS = MT_OT + 16;         // sG row of one (b, re/im, q): 48, the wave's (4 q) x (16 o) lanes hit 64 banks
    __shared__ __attribute__((aligned(16))) float sX[MT_BT * MT_QT * XS];
    __shared__ __attribute__((aligned(16))) float sG[MT_BT * 2 * MT_QT * GS];
    const int tid = threadIdx.x;
    const int ot = blockIdx.x % notile, it = (blockIdx.x / notile) % nit, qg = blockIdx.x / notile / nit;
    const int q0 = qg * MT_QT, i0 = it * MT_IT, o0 = ot * MT_OT;
    const int q = tid % MT_QT, o = (tid / MT_QT) % MT_OT, ih = tid / (MT_QT * MT_OT);       // i = i0 + ih * 16 + k
    float gr[16], gi[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) gr[k] = gi[k] = 0.f;
    const int bchunk = (B + gridDim.y - 1) / gridDim.y;
    const int bend = min(B, (int)(blockIdx.y + 1) * bchunk);
    for (int bb = blockIdx.y * bchunk; bb < bend; bb += MT_BT) {
        const int nb = min(MT_BT, bend - bb);
        __syncthreads();
        {   // stage X and dY of nb samples: thread -> (channel c, mode lq, re/im), one sample per step
            const int c = tid % 32, lq = (tid / 32) % MT_QT, ri = tid / (32 * MT_QT);
            const bool qok = q0 + lq < Q;
            for (int b = 0; b < nb; ++b) {
                float xv = 0.f, gv = 0.f;
                if (qok && i0 + c < Cin)
                    xv = X[(int64_t)(bb + b) * xbs + ((int64_t)ri * Qx + qoff + q0 + lq) * Cin + i0 + c];
                if (qok && o0 + c < Cout)
                    gv = dY[(int64_t)(bb + b) * ybs + ((int64_t)ri * Qy + qoff + q0 + lq) * Cout + o0 + c];
                sX[(b * MT_QT + lq) * XS + ri * MT_IT + c] = xv;
                sG[((b * 2 + ri) * MT_QT + lq) * GS + c] = gv;
            }
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const float g_r = sG[((b * 2 + 0) * MT_QT + q) * GS + o], g_i = sG[((b * 2 + 1) * MT_QT + q) * GS + o];
            const float* xrow = sX + (b * MT_QT + q) * XS + ih * 16;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const f32x4 xr = *reinterpret_cast<const f32x4*>(xrow + k4 * 4);
                const f32x4 xi = *reinterpret_cast<const f32x4*>(xrow + MT_IT + k4 * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = k4 * 4 + j;
                    gr[k] = fmaf(xr[j], g_r, gr[k]); gr[k] = fmaf(xi[j], g_i, gr[k]);
                    gi[k] = fmaf(xr[j], g_i, gi[k]); gi[k] = fmaf(-xi[j], g_r, gi[k]);
                }
            }
        }
    }
    float* dWs = dW + (int64_t)blockIdx.y * Cin * Cout * Q * 2;
    if (q0 + q < Q && o0 + o < Cout) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = i0 + ih * 16 + k;
            if (i < Cin)
                *reinterpret_cast<float2*>(dWs + (((int64_t)i * Cout + o0 + o) * Q + q0 + q) * 2) = make_float2(gr[k], gi[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Route pick (host only, no device call): the launchers and the workspace query all go through it.
// ------------------------------------------------------------------------------------------
static inline size_t modemix_fwd_lds(int Cin, int Cout) {
    return ((size_t)2 * Cin * Cout + (size_t)MM_BCH * 2 * Cin) * sizeof(float);
}
static inline size_t modemix_bwd_lds(int Cin, int Cout) {
    return ((size_t)2 * Cin * (Cout + 1) + (size_t)MM_BCH * 2 * Cin + (size_t)MM_BCH * 2 * Cout) * sizeof(float);
}
constexpr size_t MM_LDS_MAX = 160 * 1024;      // what allow_big_lds grants
constexpr int64_t MM_MAX_PAIRS = 24 * 256;     // resident backward: 24 (i, o) pairs per thread; 96 x 48 (ex1 as shipped) = 18

// resident route: batch slices per mode block, enough blocks for ~3 per CU, at least 8 samples per slice
static inline int modemix_slices(int B, int Q) { return std::max(1, std::min(ceil_div(768, Q), ceil_div(B, 8))); }

static inline int64_t tiled_wgrad_blocks(int Q, int Cin, int Cout) {
    return (int64_t)ceil_div(Q, MT_QT) * ceil_div(Cin, MT_IT) * ceil_div(Cout, MT_OT);
}
// tiled route: the weight gradient has one block per (mode group, channel tile) already -- the batch stays whole once
// those fill the chip (256 CUs); below that, slices of at least 8 samples up to ~2 blocks per CU
static inline int modemix_tiled_slices(int B, int Q, int Cin, int Cout) {
    const int64_t blocks = tiled_wgrad_blocks(Q, Cin, Cout);
    if (blocks >= 256) return 1;
    return std::max(1, std::min(ceil_div(512, blocks), ceil_div(B, 8)));
}

struct ModemixPlan { int fwd, bwd, slices; };
static ModemixPlan modemix_plan(int B, int Q, int Cin, int Cout) {
    ModemixPlan p;
    p.fwd = modemix_fwd_lds(Cin, Cout) <= MM_LDS_MAX ? GT_MODEMIX_RESIDENT : GT_MODEMIX_TILED;
    p.bwd = (int64_t)Cin * Cout <= MM_MAX_PAIRS && modemix_bwd_lds(Cin, Cout) <= MM_LDS_MAX ? GT_MODEMIX_RESIDENT
                                                                                            : GT_MODEMIX_TILED;
    p.slices = p.bwd == GT_MODEMIX_RESIDENT ? modemix_slices(B, Q) : modemix_tiled_slices(B, Q, Cin, Cout);
    return p;
}

template <bool CONJ>
static int tiled_apply(const float* In, const float* W, int B, int Q, int S, int T, int Cout, int64_t ibs, int64_t obs,
                       int Qi, int Qo, int qoff, float* Out, hipStream_t stream) {
    const int ntile = ceil_div(T, MT_TT);
    const int64_t gx = (int64_t)ceil_div(Q, MT_QT) * ntile;
    const int gy = ceil_div(B, MT_BT);
    if (gx > 0x7fffffff || gy > 65535) return GT_ENOTSUP;
    hipLaunchKernelGGL(modemix_tiled_apply_kernel<CONJ>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, stream, In, W, B,
                       Q, S, T, Cout, ibs, obs, Qi, Qo, qoff, ntile, Out);
    GT_LAUNCH_CHECK();
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" int gt_modemix_plan(int32_t B, int32_t Q, int32_t Cin, int32_t Cout, int32_t* fwd_route, int32_t* bwd_route,
                               int32_t* bwd_slices) {
    if (B <= 0 || Q <= 0 || Cin <= 0 || Cout <= 0) return GT_EINVAL;
    const ModemixPlan p = modemix_plan(B, Q, Cin, Cout);
    if (fwd_route) *fwd_route = p.fwd;
    if (bwd_route) *bwd_route = p.bwd;
    if (bwd_slices) *bwd_slices = p.slices;
    return 0;
}

extern "C" int gt_modemix_fwd(const float* X, const float* W, int32_t B, int32_t Q, int32_t Cin, int32_t Cout,
                              int64_t x_bstride, int64_t y_bstride, int32_t q_total_x, int32_t q_total_y,
                              int32_t q_off, float* Y, void* stream) {
    if (!X || !W || !Y || B <= 0 || Q <= 0 || Cin <= 0 || Cout <= 0 || q_off < 0 ||
        q_off + Q > q_total_x || q_off + Q > q_total_y)
        return GT_EINVAL;
    if (misaligned<8>(W)) return GT_EALIGN;
    if (modemix_plan(B, Q, Cin, Cout).fwd == GT_MODEMIX_TILED)
        return tiled_apply<false>(X, W, B, Q, Cin, Cout, Cout, x_bstride, y_bstride, q_total_x, q_total_y, q_off, Y,
                                  (hipStream_t)stream);
    const size_t lds = modemix_fwd_lds(Cin, Cout);
    if (int rc = allow_big_lds<modemix_fwd_kernel>(lds)) return rc;
    hipLaunchKernelGGL(modemix_fwd_kernel, dim3(Q, modemix_slices(B, Q)), dim3(256), lds, (hipStream_t)stream, X, W, B,
                       Q, Cin, Cout, x_bstride, y_bstride, q_total_x, q_total_y, q_off, Y);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_modemix_bwd_ws_bytes(int32_t B, int32_t Q, int32_t Cin, int32_t Cout) {
    if (B <= 0 || Q <= 0 || Cin <= 0 || Cout <= 0) return 0;
    const int S = modemix_plan(B, Q, Cin, Cout).slices;
    return S > 1 ? (int64_t)S * Cin * Cout * Q * 2 * (int64_t)sizeof(float) : 0;
}

extern "C" int gt_modemix_bwd(const float* X, const float* W, const float* dY, int32_t B, int32_t Q,
                              int32_t Cin, int32_t Cout, int64_t x_bstride, int64_t y_bstride,
                              int32_t q_total_x, int32_t q_total_y, int32_t q_off, float* dX, float* dW,
                              void* ws, int64_t ws_bytes, void* stream) {
    if (!X || !W || !dY || !dX || !dW || B <= 0 || Q <= 0 || Cin <= 0 || Cout <= 0 || q_off < 0 ||
        q_off + Q > q_total_x || q_off + Q > q_total_y)
        return GT_EINVAL;
    if (misaligned<8>(W, dW)) return GT_EALIGN;
    const ModemixPlan plan = modemix_plan(B, Q, Cin, Cout);
    const int S = plan.slices;
    const int64_t nW = (int64_t)Cin * Cout * Q * 2;
    float* dWk = dW;                                       // S == 1: the kernel writes dW directly
    if (S > 1) {
        if (!ws || ws_bytes < gt_modemix_bwd_ws_bytes(B, Q, Cin, Cout)) return GT_EWS;
        if (misaligned<8>(ws)) return GT_EALIGN;
        dWk = reinterpret_cast<float*>(ws);
    }
    if (plan.bwd == GT_MODEMIX_TILED) {
        const int nit = ceil_div(Cin, MT_IT), notile = ceil_div(Cout, MT_OT);
        const int64_t gx = tiled_wgrad_blocks(Q, Cin, Cout);
        if (gx > 0x7fffffff) return GT_ENOTSUP;
        if (int rc = tiled_apply<true>(dY, W, B, Q, Cout, Cin, Cout, y_bstride, x_bstride, q_total_y, q_total_x, q_off, dX,
                                       (hipStream_t)stream))
            return rc;
        hipLaunchKernelGGL(modemix_tiled_wgrad_kernel, dim3((unsigned)gx, (unsigned)S), dim3(256), 0, (hipStream_t)stream,
                           X, dY, B, Q, Cin, Cout, x_bstride, y_bstride, q_total_x, q_total_y, q_off, nit, notile, dWk);
    } else {
        const size_t lds = modemix_bwd_lds(Cin, Cout);
        const bool few = Cin * Cout <= 8 * 256;                // weight-gradient pairs per thread: 8, else 24
        const auto kern = few ? modemix_bwd_kernel<8> : modemix_bwd_kernel<24>;
        if (int rc = few ? allow_big_lds<modemix_bwd_kernel<8>>(lds) : allow_big_lds<modemix_bwd_kernel<24>>(lds)) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)Q, (unsigned)S), dim3(256), lds, (hipStream_t)stream, X, W, dY, B, Q, Cin,
                           Cout, x_bstride, y_bstride, q_total_x, q_total_y, q_off, dX, dWk);
    }
    GT_LAUNCH_CHECK();
    if (S > 1) return gt_slab_reduce(dWk, nW, S, nW, 1.f, dW, stream);      // fixed order: deterministic
    return 0;
}
