// Spectral complex mode mixing (gfx950), forward and backward: Y[b][q][o] = sum_i X[b][q][i] W[i][o][q] over the retained
// modes q, one block per mode and batch slice.  The backward accumulates the weight gradient per batch slice in registers;
// gt_slab_reduce sums the slices in a fixed order.
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

// batch slices per mode block: enough blocks for ~3 per CU, at least 8 samples per slice
static inline int modemix_slices(int B, int Q) { return std::max(1, std::min(ceil_div(768, Q), ceil_div(B, 8))); }

}  // namespace gt

using namespace gt;

extern "C" int gt_modemix_fwd(const float* X, const float* W, int32_t B, int32_t Q, int32_t Cin, int32_t Cout,
                              int64_t x_bstride, int64_t y_bstride, int32_t q_total_x, int32_t q_total_y,
                              int32_t q_off, float* Y, void* stream) {
    if (!X || !W || !Y || B <= 0 || Q <= 0 || Cin <= 0 || Cout <= 0 || q_off < 0 ||
        q_off + Q > q_total_x || q_off + Q > q_total_y)
        return GT_EINVAL;
    if (misaligned<8>(W)) return GT_EALIGN;
    const size_t lds = ((size_t)2 * Cin * Cout + (size_t)MM_BCH * 2 * Cin) * sizeof(float);
    if (int rc = allow_big_lds<modemix_fwd_kernel>(lds)) return rc;
    hipLaunchKernelGGL(modemix_fwd_kernel, dim3(Q, modemix_slices(B, Q)), dim3(256), lds, (hipStream_t)stream, X, W, B,
                       Q, Cin, Cout, x_bstride, y_bstride, q_total_x, q_total_y, q_off, Y);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_modemix_bwd_ws_bytes(int32_t B, int32_t Q, int32_t Cin, int32_t Cout) {
    const int S = modemix_slices(B, Q);
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
    if (Cin * Cout > 24 * 256) return GT_ENOTSUP;          // 96 x 48 (ex1 as shipped) = 18 pairs per thread
    const size_t lds = ((size_t)2 * Cin * (Cout + 1) + (size_t)MM_BCH * 2 * Cin + (size_t)MM_BCH * 2 * Cout) * sizeof(float);
    const int S = modemix_slices(B, Q);
    const int64_t nW = (int64_t)Cin * Cout * Q * 2;
    float* dWk = dW;                                       // S == 1: the kernel writes dW directly
    if (S > 1) {
        if (!ws || ws_bytes < gt_modemix_bwd_ws_bytes(B, Q, Cin, Cout)) return GT_EWS;
        if (misaligned<8>(ws)) return GT_EALIGN;
        dWk = reinterpret_cast<float*>(ws);
    }
    const bool few = Cin * Cout <= 8 * 256;                // weight-gradient pairs per thread: 8, else 24
    const auto kern = few ? modemix_bwd_kernel<8> : modemix_bwd_kernel<24>;
    if (int rc = few ? allow_big_lds<modemix_bwd_kernel<8>>(lds) : allow_big_lds<modemix_bwd_kernel<24>>(lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)Q, (unsigned)S), dim3(256), lds, (hipStream_t)stream, X, W, dY, B, Q, Cin, Cout,
                       x_bstride, y_bstride, q_total_x, q_total_y, q_off, dX, dWk);
    GT_LAUNCH_CHECK();
    if (S > 1) return gt_slab_reduce(dWk, nW, S, nW, 1.f, dW, stream);      // fixed order: deterministic
    return 0;
}
