// Bilinear resize (align_corners=True) of the CNN down/up-scalers, forward and backward, with the
// NCHW <-> NHWC layout change of the scaler boundaries fused in (reference: F.interpolate at
// libs/layers.py:483-512, 658-670; the permutes at libs/model.py:675-687, 740-749).
//
// HBM-bound: every input element is read once from HBM (the 4 taps of neighbouring outputs hit L1/L2),
// every output element is written once.  A block owns a [64 channels] x [32 x-positions] tile of one
// output row; when the input and output layouts differ the tile is transposed through LDS so both the
// loads and the stores stay coalesced (x-contiguous for NCHW, channel-contiguous float4 for NHWC).
// Backward is a gather over the (contiguous) range of outputs that touch an input pixel: no atomics,
// so it is deterministic (the reference warns that F.interpolate's backward is not,
// examples/README.md:6-7).
#include "gt_resize_core.h"
#include <type_traits>

namespace gt {

constexpr int RS_TC = 64;   // channels per tile
constexpr int RS_TX = 32;   // x positions per tile

// first output index whose i0 can reach i-1 (conservative estimate, fixed up by the caller's loop)
__device__ __forceinline__ int first_out(int i, float scale, int no) {
    if (scale <= 0.f || i <= 1) return 0;
    int o = (int)((float)(i - 1) / scale) - 2;
    return max(0, min(o, no));
}
// weight of source index i in the output coordinate a
__device__ __forceinline__ float tap_weight(const Axis& a, int i) { return (a.i0 == i ? a.l0 : 0.f) + (a.i1 == i ? a.l1 : 0.f); }

struct ResizeP {
    const float* x; float* y;
    const float* gate;          // fwd: unused.  bwd: saved activated output (ReLU gate on g), may be null
    int B, C, Hi, Wi, Ho, Wo;
    float sy, sx;
    int act;                    // fwd: GT_ACT_NONE / GT_ACT_RELU applied to the output
    int xtiles;
    // optional affine term added to the resized value of channel c at output pixel q (NHWC outputs only):
    //   + bias[c] + sum_j rp_a[q*rp_lda + j] * rp_b[c*rp_ldb + j]
    const float* bias; int rp; const float* rp_a; int64_t rp_lda; const float* rp_b; int64_t rp_ldb;
    // channels-last kernels only: the INPUT side (fwd: x, bwd: dx) is a padded concatenation of three column segments of
    // segp channels each (ops.scaler_conv_chain): real channel c lives at padded column c + (segp - seg) * min(c / seg, 2);
    // seg == 0: dense.
    int seg, segp;
    // backward with segments only: the forward input itself (padded layout, the output of a ReLU): dx is zeroed where it
    // is not positive, which is the first step of its producer's backward (ops.ScalerConvChainFn) done on the way out
    const float* in_gate;
    // act == GT_ACT_SILU (channels-last kernels): fwd writes silu'(resized value) here, bwd reads it through `gate` as a factor
    float* dact;
    int gate_mul;               // bwd: in_gate is a factor (dx *= in_gate) instead of the ReLU test
};

// padded column of real channel c
__device__ __forceinline__ int seg_col(const ResizeP& p, int c) { return c + (p.segp - p.seg) * min(c / p.seg, 2); }
// 4 consecutive real channels c .. c+3 of the padded-segment pixel at px (floats)
// (c is a multiple of 4; seg and segp are even, so the pairs (c, c+1) and (c+2, c+3) never straddle a segment: two 8-byte loads)
__device__ __forceinline__ f32x4 seg_load4(const ResizeP& p, const float* __restrict__ px, int c) {
    const f32x2 a = *reinterpret_cast<const f32x2*>(px + seg_col(p, c));
    const f32x2 b = *reinterpret_cast<const f32x2*>(px + seg_col(p, c + 2));
    return f32x4{a[0], a[1], b[0], b[1]};
}

// the affine term for any rp: the route of resize_nhwc_fwd_kernel for rp > 2 (it carries rp <= 2 in registers itself)
__device__ __forceinline__ f32x4 resize_affine(const ResizeP& p, f32x4 v, int b, int c, int oy, int ox) {
    if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + c);
    if (p.rp) {
        const float* ga = p.rp_a + (((int64_t)b * p.Ho + oy) * p.Wo + ox) * p.rp_lda;
        for (int j = 0; j < p.rp; ++j) {
            const float a = ga[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = fmaf(a, p.rp_b[(int64_t)(c + t) * p.rp_ldb + j], v[t]);
        }
    }
    return v;
}

template <bool NHWC>
__device__ __forceinline__ int64_t addr(int b, int c, int y, int x, int C, int H, int W) {
    return NHWC ? (((int64_t)b * H + y) * W + x) * C + c : (((int64_t)b * C + c) * H + y) * W + x;
}

// One row of a [RS_TC channels] x [RS_TX positions] tile that a kernel computed in the other layout and staged in LDS, to
// dst at (b, c0 .., row, x0 ..): float4 channel groups (NHWC) or x-contiguous stores (NCHW).  After a __syncthreads().
template <bool NHWC>
__device__ __forceinline__ void store_tile(const float (&tile)[RS_TC][RS_TX + 1], float* dst, int b, int c0, int row, int x0,
                                           int C, int H, int W) {
    const int t = threadIdx.x;
    if (NHWC) {
        const int c_l = (t & 15) * 4, xg = t >> 4;
        const int c = c0 + c_l;
        if (c < C) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int x_l = xg + 16 * k, x = x0 + x_l;
                if (x < W) {
                    const f32x4 v = {tile[c_l][x_l], tile[c_l + 1][x_l], tile[c_l + 2][x_l], tile[c_l + 3][x_l]};
                    *reinterpret_cast<f32x4*>(dst + addr<true>(b, c, row, x, C, H, W)) = v;
                }
            }
        }
    } else {
        const int x_l = t & 31, cg = t >> 5;
        const int x = x0 + x_l;
        if (x < W) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int c_l = cg + 8 * k, c = c0 + c_l;
                if (c < C) dst[addr<false>(b, c, row, x, C, H, W)] = tile[c_l][x_l];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ forward
template <bool IN_NHWC, bool OUT_NHWC>
__global__ __launch_bounds__(256) void resize_fwd_kernel(const ResizeP p) {
    static_assert(!(IN_NHWC && OUT_NHWC), "channels-last on both sides is resize_nhwc_fwd_kernel (with the affine epilogue)");
    __shared__ float tile[RS_TC][RS_TX + 1];
    const int t = threadIdx.x;
    const int xt = blockIdx.x % p.xtiles, ct = blockIdx.x / p.xtiles;
    const int ox0 = xt * RS_TX, c0 = ct * RS_TC, oy = blockIdx.y, b = blockIdx.z;
    const Axis ay = axis_of(oy, p.sy, p.Hi);

    if (!IN_NHWC) {
        const int ox_l = t & 31, cg = t >> 5;
        const int ox = ox0 + ox_l;
        if (ox < p.Wo) {
            const Axis ax = axis_of(ox, p.sx, p.Wi);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int c_l = cg + 8 * k, c = c0 + c_l;
                if (c < p.C) {
                    const float* r0 = p.x + addr<false>(b, c, ay.i0, 0, p.C, p.Hi, p.Wi);
                    const float* r1 = p.x + addr<false>(b, c, ay.i1, 0, p.C, p.Hi, p.Wi);
                    float v = ay.l0 * (ax.l0 * r0[ax.i0] + ax.l1 * r0[ax.i1]) +
                              ay.l1 * (ax.l0 * r1[ax.i0] + ax.l1 * r1[ax.i1]);
                    if (p.act == GT_ACT_RELU) v = fmaxf(v, 0.f);
                    if (!OUT_NHWC) p.y[addr<false>(b, c, oy, ox, p.C, p.Ho, p.Wo)] = v;
                    else tile[c_l][ox_l] = v;
                }
            }
        }
    } else {                  // channels-last input: the output is channels-first, through the tile
        const int c_l = (t & 15) * 4, xg = t >> 4;
        const int c = c0 + c_l;
        if (c < p.C) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ox_l = xg + 16 * k, ox = ox0 + ox_l;
                if (ox < p.Wo) {
                    const Axis ax = axis_of(ox, p.sx, p.Wi);
                    const f32x4 v00 = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay.i0, ax.i0, p.C, p.Hi, p.Wi));
                    const f32x4 v01 = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay.i0, ax.i1, p.C, p.Hi, p.Wi));
                    const f32x4 v10 = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay.i1, ax.i0, p.C, p.Hi, p.Wi));
                    const f32x4 v11 = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay.i1, ax.i1, p.C, p.Hi, p.Wi));
                    f32x4 v = ay.l0 * (ax.l0 * v00 + ax.l1 * v01) + ay.l1 * (ax.l0 * v10 + ax.l1 * v11);
                    if (p.act == GT_ACT_RELU) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) tile[c_l + j][ox_l] = v[j];
                }
            }
        }
    }
    if (IN_NHWC == OUT_NHWC) return;
    __syncthreads();
    store_tile<OUT_NHWC>(tile, p.y, b, c0, oy, ox0, p.C, p.Ho, p.Wo);
}

// ------------------------------------------------------------------------------------------ backward
// p.x = upstream gradient g (output-shaped, layout G_NHWC), p.y = dx (input-shaped, layout DX_NHWC),
// p.gate = saved activated forward output (same shape/layout as g) or null.  Hi/Wi are the sizes of
// the FORWARD input (= dx), Ho/Wo of the forward output (= g).  blockIdx.y = input row iy.
//
// The outputs that touch input index i form a contiguous range; their weights are gathered once per
// thread (x) / per block (y) into a small register table, so the channel loop is pure load + fma.
constexpr int RS_MAXT = 6;          // taps per axis held in registers (covers up-sampling factors < 2.5)
struct Taps {
    int lo, n;
    float w[RS_MAXT];
};
__device__ __forceinline__ Taps taps_of(int i, float scale, int ni, int no) {
    Taps t;
    int lo = first_out(i, scale, no);
    while (lo < no && axis_of(lo, scale, ni).i0 < i - 1) ++lo;
    t.lo = lo;
    t.n = 0;
#pragma unroll
    for (int j = 0; j < RS_MAXT; ++j) t.w[j] = 0.f;
#pragma unroll
    for (int j = 0; j < RS_MAXT; ++j) {
        const int o = lo + j;
        if (o < no) {
            const Axis a = axis_of(o, scale, ni);
            if (a.i0 <= i) {
                t.w[j] = tap_weight(a, i);
                t.n = j + 1;
            }
        }
    }
    // more than RS_MAXT contributing outputs (very strong up-sampling): flag with n = -1
    if (lo + RS_MAXT < no && axis_of(lo + RS_MAXT, scale, ni).i0 <= i) t.n = -1;
    return t;
}

// g through the activation behind it: ReLU lets it pass where the saved output y is positive; with act == GT_ACT_SILU y is the
// saved derivative, a factor.  (Scalars are gated in the channels-first kernels only, where act is the constant GT_ACT_RELU.)
__device__ __forceinline__ float gate(float g, float y, int act) {
    if (act == GT_ACT_SILU) return g * y;
    if (!(y > 0.f)) g = 0.f;
    return g;
}
template <typename V>       // f32x2, f32x4
__device__ __forceinline__ V gate(V g, V y, int act) {
    if (act == GT_ACT_SILU) return g * y;
#pragma unroll
    for (int j = 0; j < (int)(sizeof(V) / sizeof(float)); ++j) if (!(y[j] > 0.f)) g[j] = 0.f;
    return g;
}
// The loader of the gathers below: the gated upstream gradient of channel c (NCHW) or of the channels c .. c+3 (NHWC).
// row(oy) is the offset of output row oy, (row, ox) the value at its column ox: two steps, so that the row's share of the
// address is worked out once per row and not under every tap's predicate.
template <bool NHWC>
struct GatedGrad {
    using V = std::conditional_t<NHWC, f32x4, float>;
    const ResizeP& p;
    int b, c;
    // what p.gate holds.  The kernels of gt_bilinear2d_bwd leave the default: that entry point admits no other gate, and they
    // never read p.act; resize_nhwc_bwd_kernel (gt_bilinear2d_seg_bwd: also SiLU) passes p.act
    int act = GT_ACT_RELU;
    // addr<NHWC>(b, c, oy, ox, p.C, p.Ho, p.Wo), split at the row
    __device__ __forceinline__ int64_t row(int oy) const {
        return NHWC ? ((int64_t)b * p.Ho + oy) * p.Wo : (((int64_t)b * p.C + c) * p.Ho + oy) * p.Wo;
    }
    __device__ __forceinline__ V operator()(int64_t row, int ox) const {
        const int64_t o = NHWC ? (row + ox) * p.C + c : row + ox;
        V g = *reinterpret_cast<const V*>(p.x + o);
        if (p.gate) g = gate(g, *reinterpret_cast<const V*>(p.gate + o), act);
        return g;
    }
};
// acc + w * g in the form each value type has always used here: one fmaf on scalars, multiply and add on vectors
__device__ __forceinline__ float madd(float w, float g, float acc) { return fmaf(w, g, acc); }
__device__ __forceinline__ f32x4 madd(float w, f32x4 g, f32x4 acc) { acc += w * g; return acc; }

// dx of one input cell from the register tables: sum_jy ty.w[jy] * (sum_jx tx.w[jx] * g(ty.lo + jy, tx.lo + jx))
template <typename V, typename Load>
__device__ __forceinline__ V gather_table(const Taps& ty, const Taps& tx, const Load& g_at) {
    V acc = V{};
#pragma unroll
    for (int jy = 0; jy < RS_MAXT; ++jy) {
        if (jy < ty.n) {
            const int64_t row = g_at.row(ty.lo + jy);
            V racc = V{};
#pragma unroll
            for (int jx = 0; jx < RS_MAXT; ++jx)
                if (jx < tx.n) racc = madd(tx.w[jx], g_at(row, tx.lo + jx), racc);
            acc = madd(ty.w[jy], racc, acc);
        }
    }
    return acc;
}
// the same sum over an arbitrary number of taps (an axis flagged n = -1), from the first candidates oy_lo / ox_lo on
template <typename V, typename Load>
__device__ __forceinline__ V gather_any(const ResizeP& p, int iy, int ix, int oy_lo, int ox_lo, const Load& g_at) {
    V acc = V{};
    for (int oy = oy_lo; oy < p.Ho; ++oy) {
        const Axis ay = axis_of(oy, p.sy, p.Hi);
        if (ay.i0 > iy) break;
        const int64_t row = g_at.row(oy);
        V racc = V{};
        for (int ox = ox_lo; ox < p.Wo; ++ox) {
            const Axis ax = axis_of(ox, p.sx, p.Wi);
            if (ax.i0 > ix) break;
            racc = madd(tap_weight(ax, ix), g_at(row, ox), racc);
        }
        acc = madd(tap_weight(ay, iy), racc, acc);
    }
    return acc;
}

template <bool G_NHWC, bool DX_NHWC>
__global__ __launch_bounds__(256) void resize_bwd_kernel(const ResizeP p) {
    __shared__ float tile[RS_TC][RS_TX + 1];
    const int t = threadIdx.x;
    const int xt = blockIdx.x % p.xtiles, ct = blockIdx.x / p.xtiles;
    const int ix0 = xt * RS_TX, c0 = ct * RS_TC, iy = blockIdx.y, b = blockIdx.z;
    const Taps ty = taps_of(iy, p.sy, p.Hi, p.Ho);

    if (!G_NHWC) {
        const int ix_l = t & 31, cg = t >> 5;
        const int ix = ix0 + ix_l;
        if (ix < p.Wi) {
            const Taps tx = taps_of(ix, p.sx, p.Wi, p.Wo);
            if (ty.n >= 0 && tx.n >= 0) {
                float accs[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {           // 8 independent channels in flight per lane
                    const int c = c0 + cg + 8 * k;
                    accs[k] = c < p.C ? gather_table<float>(ty, tx, GatedGrad<false>{p, b, c}) : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int c_l = cg + 8 * k, c = c0 + c_l;
                    if (c < p.C) {
                        if (!DX_NHWC) p.y[addr<false>(b, c, iy, ix, p.C, p.Hi, p.Wi)] = accs[k];
                        else tile[c_l][ix_l] = accs[k];
                    }
                }
            } else {
#pragma unroll 1
                for (int k = 0; k < 8; ++k) {           // generic path: arbitrary number of taps
                    const int c_l = cg + 8 * k, c = c0 + c_l;
                    if (c >= p.C) break;
                    const float acc = gather_any<float>(p, iy, ix, ty.lo, tx.lo, GatedGrad<false>{p, b, c});
                    if (!DX_NHWC) p.y[addr<false>(b, c, iy, ix, p.C, p.Hi, p.Wi)] = acc;
                    else tile[c_l][ix_l] = acc;
                }
            }
        }
    } else {
        const int c_l = (t & 15) * 4, xg = t >> 4;
        const int c = c0 + c_l;
        if (c < p.C) {
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                const int ix_l = xg + 16 * k, ix = ix0 + ix_l;
                if (ix >= p.Wi) break;
                const Taps tx = taps_of(ix, p.sx, p.Wi, p.Wo);
                const GatedGrad<true> g_at{p, b, c};
                f32x4 acc;
                if (ty.n >= 0 && tx.n >= 0) acc = gather_table<f32x4>(ty, tx, g_at);
                else acc = gather_any<f32x4>(p, iy, ix, ty.lo, tx.lo, g_at);
                if (DX_NHWC) {
                    *reinterpret_cast<f32x4*>(p.y + addr<true>(b, c, iy, ix, p.C, p.Hi, p.Wi)) = acc;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) tile[c_l + j][ix_l] = acc[j];
                }
            }
        }
    }
    if (G_NHWC == DX_NHWC) return;
    __syncthreads();
    store_tile<DX_NHWC>(tile, p.y, b, c0, iy, ix0, p.C, p.Hi, p.Wi);
}

// NCHW -> NCHW backward over flattened planes: a thread owns one input pixel (iy, ix) of 8 channel planes,
// so the stores of a wave are 256 contiguous bytes per plane regardless of the (odd) row length.
__global__ __launch_bounds__(256) void resize_bwd_planar_kernel(const ResizeP p) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.Hi * p.Wi) return;
    const int iy = e / p.Wi, ix = e - iy * p.Wi;
    const int b = blockIdx.z, cbase = blockIdx.y * 8;
    const Taps ty = taps_of(iy, p.sy, p.Hi, p.Ho);
    const Taps tx = taps_of(ix, p.sx, p.Wi, p.Wo);
    const int64_t plane_i = (int64_t)p.Hi * p.Wi;
    if (ty.n >= 0 && tx.n >= 0) {
        float accs[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = cbase + k;
            accs[k] = c < p.C ? gather_table<float>(ty, tx, GatedGrad<false>{p, b, c}) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (cbase + k < p.C) p.y[((int64_t)b * p.C + cbase + k) * plane_i + e] = accs[k];
    } else {
        for (int k = 0; k < 8 && cbase + k < p.C; ++k) {
            const float acc = gather_any<float>(p, iy, ix, ty.lo, tx.lo, GatedGrad<false>{p, b, cbase + k});
            p.y[((int64_t)b * p.C + cbase + k) * plane_i + e] = acc;
        }
    }
}

static int check_resize(const void* x, const void* y, int B, int C, int Hi, int Wi, int Ho, int Wo,
                        int in_nhwc, int out_nhwc) {
    if (!x || !y || B <= 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return GT_EINVAL;
    if ((in_nhwc | out_nhwc) & ~1) return GT_EINVAL;
    if (B > 65535 || Ho > 65535 || Hi > 65535) return GT_EINVAL;
    if ((in_nhwc || out_nhwc) && (C & 3)) return GT_ENOTSUP;          // NHWC side moves float4 channel groups
    if (in_nhwc && (reinterpret_cast<uintptr_t>(x) & 15)) return GT_EALIGN;
    if (out_nhwc && (reinterpret_cast<uintptr_t>(y) & 15)) return GT_EALIGN;
    return 0;
}
// ---- channels-last on both sides (the fine-grid resize of the regressor input): one thread per (pixel, 4
// channels), flat over a row, so narrow channel counts (C = 32) keep every lane busy; RPT output rows per thread
// put 4*RPT independent float4 loads in flight.
constexpr int RN_RPT = 4;
__global__ __launch_bounds__(256) void resize_nhwc_fwd_kernel(const ResizeP p) {
    const int C4 = p.C >> 2;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.Wo * C4) return;
    const int ox = e / C4, c = (e - ox * C4) * 4;
    const int oy0 = blockIdx.y * RN_RPT, b = blockIdx.z;
    const Axis ax = axis_of(ox, p.sx, p.Wi);
    Axis ay[RN_RPT];
    f32x4 v[RN_RPT][4];
    // Affine epilogue (gt_bilinear2d_fwd_affine: bias + up to two rank-1 terms, the regressor's fc(cat[x, grid]) commuted in
    // front of the resize): the bias and the weights of the thread's four channels do not depend on the row -- fetched ONCE,
    // here, and the rows' coefficients with the rows' taps, so that no load stands between the interpolation and the store
    // (resize_affine ran a dynamic loop of dependent scalar loads per row: 260 us against 118 us without the epilogue; 155 now).
    const bool rp2 = p.rp == 1 || p.rp == 2;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f}, w0 = bv, w1 = bv;
    float a0[RN_RPT], a1[RN_RPT];
    if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + c);
    if (rp2) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            w0[t] = p.rp_b[(int64_t)(c + t) * p.rp_ldb];
            w1[t] = p.rp == 2 ? p.rp_b[(int64_t)(c + t) * p.rp_ldb + 1] : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < RN_RPT; ++r) {
        const int oy = min(oy0 + r, p.Ho - 1);
        ay[r] = axis_of(oy, p.sy, p.Hi);
        a0[r] = a1[r] = 0.f;
        if (rp2) {
            const float* ga = p.rp_a + (((int64_t)b * p.Ho + oy) * p.Wo + ox) * p.rp_lda;
            a0[r] = ga[0];
            if (p.rp == 2) a1[r] = ga[1];
        }
        if (p.seg) {          // padded three-segment input: gather the four real channels (block-uniform branch)
            const int CP3 = 3 * p.segp;
            v[r][0] = seg_load4(p, p.x + addr<true>(b, 0, ay[r].i0, ax.i0, CP3, p.Hi, p.Wi), c);
            v[r][1] = seg_load4(p, p.x + addr<true>(b, 0, ay[r].i0, ax.i1, CP3, p.Hi, p.Wi), c);
            v[r][2] = seg_load4(p, p.x + addr<true>(b, 0, ay[r].i1, ax.i0, CP3, p.Hi, p.Wi), c);
            v[r][3] = seg_load4(p, p.x + addr<true>(b, 0, ay[r].i1, ax.i1, CP3, p.Hi, p.Wi), c);
            continue;
        }
        v[r][0] = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay[r].i0, ax.i0, p.C, p.Hi, p.Wi));
        v[r][1] = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay[r].i0, ax.i1, p.C, p.Hi, p.Wi));
        v[r][2] = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay[r].i1, ax.i0, p.C, p.Hi, p.Wi));
        v[r][3] = *reinterpret_cast<const f32x4*>(p.x + addr<true>(b, c, ay[r].i1, ax.i1, p.C, p.Hi, p.Wi));
    }
#pragma unroll
    for (int r = 0; r < RN_RPT; ++r) {
        const int oy = oy0 + r;
        if (oy < p.Ho) {
            f32x4 o = ay[r].l0 * (ax.l0 * v[r][0] + ax.l1 * v[r][1]) + ay[r].l1 * (ax.l0 * v[r][2] + ax.l1 * v[r][3]);
            if (rp2 || !p.rp) {                 // same operations in the same order as resize_affine
                if (p.bias) o += bv;
                if (rp2) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        o[t] = fmaf(a0[r], w0[t], o[t]);
                        if (p.rp == 2) o[t] = fmaf(a1[r], w1[t], o[t]);
                    }
                }
            } else {
                o = resize_affine(p, o, b, c, oy, ox);
            }
            if (p.act == GT_ACT_RELU) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
            } else if (p.act == GT_ACT_SILU) {          // + the derivative the backward multiplies g with
                f32x4 d;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float a, da;
                    silu_both(o[j], a, da);
                    o[j] = a; d[j] = da;
                }
                if (p.dact) *reinterpret_cast<f32x4*>(p.dact + addr<true>(b, c, oy, ox, p.C, p.Ho, p.Wo)) = d;
            }
            *reinterpret_cast<f32x4*>(p.y + addr<true>(b, c, oy, ox, p.C, p.Ho, p.Wo)) = o;
        }
    }
}

// GatedGrad for four consecutive dx columns of resize_nhwc_bwd_kernel: the channels c .. c+3 (p.seg == 0), or with padded
// segments the real channels cr[0..3] (-1: a padding column, gradient zero)
struct SegGatedGrad : GatedGrad<true> {
    const int (&cr)[4];
    __device__ __forceinline__ f32x4 operator()(int64_t row, int ox) const {
        f32x4 g;
        if (p.seg) {              // the column pairs (0,1) and (2,3) are real together or padding together
            const int64_t o = (row + ox) * p.C;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 gv = {0.f, 0.f};
                if (cr[2 * h] >= 0) {
                    gv = *reinterpret_cast<const f32x2*>(p.x + o + cr[2 * h]);
                    if (p.gate) gv = gate(gv, *reinterpret_cast<const f32x2*>(p.gate + o + cr[2 * h]), p.act);
                }
                g[2 * h] = gv[0]; g[2 * h + 1] = gv[1];
            }
        } else g = GatedGrad<true>::operator()(row, ox);
        return g;
    }
};

// gather form of the backward (no atomics), same thread mapping over an input row; falls back to the tiled
// kernel's generic loop when an axis has more than RS_MAXT contributing outputs
__global__ __launch_bounds__(256) void resize_nhwc_bwd_kernel(const ResizeP p) {
    // dx has p.C channels, or (p.seg != 0) the three padded column segments of 3 * p.segp channels: a thread owns four
    // consecutive dx columns; with segments each maps to a real channel of g or to a padding column (gradient zero)
    const int CX = p.seg ? 3 * p.segp : p.C;
    const int C4 = CX >> 2;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int iy = blockIdx.y, b = blockIdx.z;
    // The tap tables (first output, count, weights: float divisions and a dozen axis_of evaluations each) are the same for every
    // channel group of a pixel and -- along y -- for the whole block: worked out ONCE per block by the first threads and read
    // back from LDS, instead of twice by every thread (they were a large part of the kernel's instructions).
    constexpr int TXMAX = 66;                        // pixels a block's 256 four-channel groups can touch when C4 >= 4
    __shared__ Taps s_tx[TXMAX];
    __shared__ Taps s_ty;
    const int px0 = (blockIdx.x * 256) / C4;
    const bool shared_taps = C4 >= 4;
    if (shared_taps) {
        const int npx = min((blockIdx.x * 256 + 255) / C4, p.Wi - 1) - px0 + 1;
        if ((int)threadIdx.x < npx) s_tx[threadIdx.x] = taps_of(px0 + threadIdx.x, p.sx, p.Wi, p.Wo);
        if (threadIdx.x == 255) s_ty = taps_of(iy, p.sy, p.Hi, p.Ho);
        __syncthreads();
    }
    if (e >= p.Wi * C4) return;
    const int ix = e / C4, c = (e - ix * C4) * 4;
    int cr[4] = {c, c + 1, c + 2, c + 3};          // real channel of each column, -1: padding
    if (p.seg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sgi = (c + j) / p.segp, r = (c + j) - sgi * p.segp;
            const int width = sgi < 2 ? p.seg : p.C - 2 * p.seg;
            cr[j] = r < width ? sgi * p.seg + r : -1;
        }
    }
    const Taps ty = shared_taps ? s_ty : taps_of(iy, p.sy, p.Hi, p.Ho);
    const Taps tx = shared_taps ? s_tx[ix - px0] : taps_of(ix, p.sx, p.Wi, p.Wo);
    f32x4 acc = gather_table<f32x4>(ty, tx, SegGatedGrad{{p, b, c, p.act}, cr});
    const int64_t od = addr<true>(b, c, iy, ix, CX, p.Hi, p.Wi);
    if (p.in_gate) {
        const f32x4 xin = *reinterpret_cast<const f32x4*>(p.in_gate + od);
        if (p.gate_mul) acc *= xin;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (!(xin[j] > 0.f)) acc[j] = 0.f;
        }
    }
    *reinterpret_cast<f32x4*>(p.y + od) = acc;
}

// true when no input index of the axis has more than RS_MAXT contributing outputs (host-side bound:
// an input cell's support spans at most 2 * (no-1)/(ni-1) outputs)
static inline bool taps_fit(int ni, int no) {
    return ni <= 1 ? no <= RS_MAXT : 2.0 * (double)(no - 1) / (double)(ni - 1) + 2.0 <= (double)RS_MAXT;
}

}  // namespace gt

using namespace gt;

// geometry and scales of a launch; the entry points assign what is theirs (act, gate, affine, segments) by name
static ResizeP make_resize_p(const float* src, float* dst, int B, int C, int Hi, int Wi, int Ho, int Wo, int xtiles) {
    ResizeP p{};
    p.x = src; p.y = dst;
    p.B = B; p.C = C; p.Hi = Hi; p.Wi = Wi; p.Ho = Ho; p.Wo = Wo;
    p.sy = scale_of(Hi, Ho); p.sx = scale_of(Wi, Wo);
    p.xtiles = xtiles;
    return p;
}

extern "C" int gt_bilinear2d_fwd_affine(const float* x, float* y, int32_t B, int32_t C, int32_t Hi, int32_t Wi,
                                        int32_t Ho, int32_t Wo, int32_t in_nhwc, int32_t out_nhwc, int32_t act,
                                        const gt_resize_affine* aff, void* stream) {
    if (int rc = check_resize(x, y, B, C, Hi, Wi, Ho, Wo, in_nhwc, out_nhwc)) return rc;
    if (act != GT_ACT_NONE && act != GT_ACT_RELU) return GT_ENOTSUP;
    ResizeP p = make_resize_p(x, y, B, C, Hi, Wi, Ho, Wo, ceil_div(Wo, RS_TX));
    p.act = act;
    if (aff && (aff->bias || aff->rp)) {
        if (!(in_nhwc && out_nhwc)) return GT_ENOTSUP;
        if (aff->rp < 0 || aff->rp > 8 || (aff->rp && (!aff->rp_a || !aff->rp_b))) return GT_EINVAL;
        if (aff->bias && (reinterpret_cast<uintptr_t>(aff->bias) & 15)) return GT_EALIGN;
        p.bias = aff->bias; p.rp = aff->rp; p.rp_a = aff->rp_a; p.rp_lda = aff->rp_lda;
        p.rp_b = aff->rp_b; p.rp_ldb = aff->rp_ldb;
    }
    dim3 grid((unsigned)(p.xtiles * ceil_div(C, RS_TC)), (unsigned)Ho, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (!in_nhwc && !out_nhwc) hipLaunchKernelGGL((resize_fwd_kernel<false, false>), grid, dim3(256), 0, st, p);
    else if (!in_nhwc && out_nhwc) hipLaunchKernelGGL((resize_fwd_kernel<false, true>), grid, dim3(256), 0, st, p);
    else if (in_nhwc && !out_nhwc) hipLaunchKernelGGL((resize_fwd_kernel<true, false>), grid, dim3(256), 0, st, p);
    else {          // check_resize: C % 4 == 0, and Ho <= 65535 bounds the grid of RN_RPT-row groups
        dim3 ng((unsigned)ceil_div((int64_t)Wo * (C / 4), 256), (unsigned)ceil_div(Ho, RN_RPT), (unsigned)B);
        hipLaunchKernelGGL(resize_nhwc_fwd_kernel, ng, dim3(256), 0, st, p);
    }
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_bilinear2d_fwd(const float* x, float* y, int32_t B, int32_t C, int32_t Hi, int32_t Wi,
                                 int32_t Ho, int32_t Wo, int32_t in_nhwc, int32_t out_nhwc, int32_t act,
                                 void* stream) {
    return gt_bilinear2d_fwd_affine(x, y, B, C, Hi, Wi, Ho, Wo, in_nhwc, out_nhwc, act, nullptr, stream);
}

extern "C" int gt_bilinear2d_bwd(const float* g, const float* y_saved, float* dx, int32_t B, int32_t C,
                                 int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t in_nhwc,
                                 int32_t out_nhwc, int32_t act, void* stream) {
    // g (and y_saved) have the forward OUTPUT shape/layout, dx the forward INPUT shape/layout
    if (int rc = check_resize(dx, g, B, C, Hi, Wi, Ho, Wo, in_nhwc, out_nhwc)) return rc;
    if (act != GT_ACT_NONE && act != GT_ACT_RELU) return GT_ENOTSUP;
    if (act == GT_ACT_RELU && !y_saved) return GT_EINVAL;
    if (out_nhwc && y_saved && (reinterpret_cast<uintptr_t>(y_saved) & 15)) return GT_EALIGN;
    ResizeP p = make_resize_p(g, dx, B, C, Hi, Wi, Ho, Wo, ceil_div(Wi, RS_TX));
    p.act = act;
    p.gate = act == GT_ACT_RELU ? y_saved : nullptr;
    dim3 grid((unsigned)(p.xtiles * ceil_div(C, RS_TC)), (unsigned)Hi, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (!out_nhwc && !in_nhwc) {
        if (ceil_div(C, 8) > 65535) return GT_EINVAL;
        dim3 pg((unsigned)ceil_div((int64_t)Hi * Wi, 256), (unsigned)ceil_div(C, 8), (unsigned)B);
        hipLaunchKernelGGL(resize_bwd_planar_kernel, pg, dim3(256), 0, st, p);
    }
    else if (!out_nhwc && in_nhwc) hipLaunchKernelGGL((resize_bwd_kernel<false, true>), grid, dim3(256), 0, st, p);
    else if (out_nhwc && !in_nhwc) hipLaunchKernelGGL((resize_bwd_kernel<true, false>), grid, dim3(256), 0, st, p);
    else if (taps_fit(Hi, Ho) && taps_fit(Wi, Wo)) {          // (check_resize: C % 4 == 0)
        dim3 ng((unsigned)ceil_div((int64_t)Wi * (C / 4), 256), (unsigned)Hi, (unsigned)B);
        hipLaunchKernelGGL(resize_nhwc_bwd_kernel, ng, dim3(256), 0, st, p);
    } else hipLaunchKernelGGL((resize_bwd_kernel<true, true>), grid, dim3(256), 0, st, p);
    GT_LAUNCH_CHECK();
    return 0;
}

// Channels-last resize whose INPUT is the padded three-segment buffer of ops.scaler_conv_chain (gt_hip.h)
static int check_seg(int C, int seg, int segp) {
    if (seg <= 0 || (seg & 1) || segp < seg || (segp & 3) || (C & 3) || C <= 2 * seg || C - 2 * seg > segp) return GT_EINVAL;
    return 0;
}

extern "C" int gt_bilinear2d_seg_fwd(const float* x, float* y, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho,
                                     int32_t Wo, int32_t act, int32_t seg, int32_t segp, float* dact, void* stream) {
    if (int rc = check_resize(x, y, B, C, Hi, Wi, Ho, Wo, 1, 1)) return rc;
    if (int rc = check_seg(C, seg, segp)) return rc;
    if (act != GT_ACT_NONE && act != GT_ACT_RELU && act != GT_ACT_SILU) return GT_ENOTSUP;
    if (dact && (act != GT_ACT_SILU || (reinterpret_cast<uintptr_t>(dact) & 15))) return GT_EINVAL;
    if (ceil_div(Ho, RN_RPT) > 65535) return GT_EINVAL;
    ResizeP p = make_resize_p(x, y, B, C, Hi, Wi, Ho, Wo, ceil_div(Wo, RS_TX));
    p.act = act;
    p.seg = seg; p.segp = segp;
    p.dact = dact;
    dim3 ng((unsigned)ceil_div((int64_t)Wo * (C / 4), 256), (unsigned)ceil_div(Ho, RN_RPT), (unsigned)B);
    hipLaunchKernelGGL(resize_nhwc_fwd_kernel, ng, dim3(256), 0, (hipStream_t)stream, p);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_bilinear2d_seg_bwd(const float* g, const float* y_saved, float* dx, int32_t B, int32_t C, int32_t Hi,
                                     int32_t Wi, int32_t Ho, int32_t Wo, int32_t act, int32_t seg, int32_t segp,
                                     const float* x_gate, int32_t gate_mul, void* stream) {
    if (int rc = check_resize(dx, g, B, C, Hi, Wi, Ho, Wo, 1, 1)) return rc;
    if (int rc = check_seg(C, seg, segp)) return rc;
    if (act != GT_ACT_NONE && act != GT_ACT_RELU && act != GT_ACT_SILU) return GT_ENOTSUP;
    if (act != GT_ACT_NONE && !y_saved) return GT_EINVAL;          // ReLU: the activated output; SiLU: the forward's dact
    if (y_saved && (reinterpret_cast<uintptr_t>(y_saved) & 15)) return GT_EALIGN;
    if (!taps_fit(Hi, Ho) || !taps_fit(Wi, Wo)) return GT_ENOTSUP;
    ResizeP p = make_resize_p(g, dx, B, C, Hi, Wi, Ho, Wo, ceil_div(Wi, RS_TX));
    p.act = act;
    p.gate = act != GT_ACT_NONE ? y_saved : nullptr;
    p.seg = seg; p.segp = segp;
    p.in_gate = x_gate;
    p.gate_mul = gate_mul != 0;
    if (x_gate && (reinterpret_cast<uintptr_t>(x_gate) & 15)) return GT_EALIGN;
    dim3 ng((unsigned)ceil_div((int64_t)Wi * (3 * segp / 4), 256), (unsigned)Hi, (unsigned)B);
    hipLaunchKernelGGL(resize_nhwc_bwd_kernel, ng, dim3(256), 0, (hipStream_t)stream, p);
    GT_LAUNCH_CHECK();
    return 0;
}
