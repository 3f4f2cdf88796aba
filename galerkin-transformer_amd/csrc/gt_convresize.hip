// gt_conv3x3_resize_*: forward and weight-gradient backward (the bilinear rule itself: gt_resize_core.h).  First stage of the down-scaler fused into one pass (layers.py:483-495: Conv2dResBlock(in -> out, 3x3,
// padding 1, no bias) -> dropout -> act, then F.interpolate -> act):
//     y0[b,c,iy,ix] = relu( keep(b,c,iy,ix) * sum_{ci,dy,dx} W[c,ci,dy,dx] x[b,ci,iy+dy-1,ix+dx-1] )
//     y [b,c,oy,ox] = relu( bilinear(y0)[oy,ox] )
// The input has one (few) channel(s) while y0 has `out` channels at the fine resolution (651 MB at
// 141^2 x 128 x batch 64): y0 is never written -- the conv is re-evaluated at the 4 source pixels of each
// output (36 fma per output and input channel), and in backward at every fine pixel, where the gathered
// gradient is turned straight into the 3x3 weight gradient.  The dropout mask uses the linear NCHW index
// of y0, so the fused op draws exactly the mask the unfused conv -> gt_dropout_apply sequence would.
#include "gt_resize_core.h"
#include <type_traits>
#include <utility>

namespace gt {

constexpr int CR_MAXCI = 4;         // input channels supported by the fused path
constexpr int CR_CH = 16;           // output channels per block (forward)

struct ConvResizeP {
    const float* x; const float* w; float* y;          // fwd: y output.  bwd: y = saved forward output
    const float* g; float* partial;                    // bwd only
    int B, Cin, Cout, H, W, Ho, Wo;
    float sy, sx;
    DropDev drop;
    int y_nhwc;                                        // y (and g) channels-last [B, Ho, Wo, Cout] instead of channels-first
    int nstrips;                                       // bwd, channels-last: pixel strips per image (1-D grid, see kernel)
    // channels-last only, optional: the forward's decisions, 4 bits per (output pixel, channel) -- bit t: source pixel t of
    // the bilinear stencil was kept by the dropout AND positive; all four cleared when the resized value itself is <= 0 (its
    // gradient is zero then).  [B][Cout / 16][Ho * Wo] 64-bit words (a wave's 64 pixels are 512 contiguous bytes for the
    // writer and for the reader), nibble c % 16 of word c / 16.  With it the backward neither re-evaluates the convolution
    // nor re-draws the dropout mask, and does not read y.
    unsigned long long* bits;
};

__device__ __forceinline__ void load_patch(const float* __restrict__ xp, int H, int W, int iy, int ix,
                                           float (&pt)[9]) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = iy + dy - 1;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xx = ix + dx - 1;
            pt[dy * 3 + dx] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? xp[(int64_t)yy * W + xx] : 0.f;
        }
    }
}
// the same patch without branches (the backward requests 36 of these values per pixel in front of a long arithmetic block):
// the load goes to a clamped (valid) address, the select zeroes what lies outside the picture.  The forward is faster with
// the predicated form above (271 vs 353 us at B = 128), the backward with this one.
__device__ __forceinline__ void load_patch_clamped(const float* __restrict__ xp, int H, int W, int iy, int ix,
                                                   float (&pt)[9]) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = iy + dy - 1;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xx = ix + dx - 1;
            const int yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy), xc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
            const float v = xp[yc * W + xc];
            pt[dy * 3 + dx] = (yy == yc && xx == xc) ? v : 0.f;
        }
    }
}

// Parity hook (gt_debug_conv0_mask): when set, the forward records the ReLU decision it takes for every fine-grid value
// of the fused convolution it evaluates -- mask[(b * Cout + c) * H * W + pixel] = 1 (kept and positive) or 0 -- so a
// float64 checker can replay exactly these decisions (tests/test_bench_kernels_gpu.py; pixels no output touches stay as
// the caller initialised them).  One pointer load per thread when unset.
__device__ unsigned char* g_conv0_mask = nullptr;

template <int CIN, int ACT = GT_ACT_RELU>
__global__ __launch_bounds__(256) void conv_resize_fwd_kernel(const ConvResizeP p) {
    __shared__ float sw[CR_CH * CIN * 9];
    // channels-last output: the channel groups of a pixel strip are neighbouring blocks (they complete the strip's
    // 512-byte rows together); channels-first: the pixel strips of a channel group are
    const int bc = p.y_nhwc ? blockIdx.x : blockIdx.y, bx = p.y_nhwc ? blockIdx.y : blockIdx.x;
    const int c0 = bc * CR_CH, b = blockIdx.z;
    for (int i = threadIdx.x; i < CR_CH * CIN * 9; i += 256) {
        const int c = c0 + i / (CIN * 9);
        sw[i] = (c < p.Cout) ? p.w[(int64_t)c * CIN * 9 + i % (CIN * 9)] : 0.f;
    }
    __syncthreads();
    const int e = bx * 256 + threadIdx.x;
    if (e >= p.Ho * p.Wo) return;
    const int oy = e / p.Wo, ox = e - oy * p.Wo;
    const Axis ay = axis_of(oy, p.sy, p.H), ax = axis_of(ox, p.sx, p.W);
    const uint32_t key = drop_key_dev(p.drop);
    unsigned char* const dbg_mask = g_conv0_mask;
    // 3x3 input patches around the 4 source pixels, kept in registers for every output channel
    float pt[CIN][4][9];
    uint32_t toff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int iy = (t & 2) ? ay.i1 : ay.i0, ix = (t & 1) ? ax.i1 : ax.i0;
        toff[t] = (uint32_t)(iy * p.W + ix);
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
            load_patch(p.x + ((int64_t)b * CIN + ci) * p.H * p.W, p.H, p.W, iy, ix, pt[ci][t]);
    }
    const uint32_t plane = (uint32_t)(p.H * p.W);
    const float w00 = ay.l0 * ax.l0, w01 = ay.l0 * ax.l1, w10 = ay.l1 * ax.l0, w11 = ay.l1 * ax.l1;
    unsigned long long nib = 0ull;                  // p.bits: the decisions of this pixel's CR_CH = 16 channels
#pragma unroll 1
    for (int j4 = 0; j4 < CR_CH; j4 += 4) {
        if (c0 + j4 >= p.Cout) break;
        float r4[4];
        unsigned n16 = 0u;                          // the four channels' nibbles
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = j4 + jj, c = c0 + j;
            float cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float wv = sw[(j * CIN + ci) * 9 + k];           // zero for c >= Cout
#pragma unroll
                    for (int t = 0; t < 4; ++t) cv[t] = fmaf(wv, pt[ci][t][k], cv[t]);
                }
            const uint32_t cbase = ((uint32_t)b * (uint32_t)p.Cout + (uint32_t)c) * plane;   // mod 2^32, like the
#pragma unroll                                                                                // stand-alone dropout
            for (int t = 0; t < 4; ++t) {
                const float m = p.drop.thresh ? drop_mul(p.drop, key, cbase + toff[t]) : p.drop.scale;
                if (ACT == GT_ACT_SILU) cv[t] = silu_f(cv[t] * m);
                else {
                    cv[t] = fmaxf(cv[t] * m, 0.f);
                    if (dbg_mask && c < p.Cout) dbg_mask[cbase + toff[t]] = cv[t] > 0.f ? 1 : 0;
                }
            }
            // same association as the stand-alone resize: l0y*(l0x*v00 + l1x*v01) + l1y*(l0x*v10 + l1x*v11)
            const float rz = ay.l0 * (ax.l0 * cv[0] + ax.l1 * cv[1]) + ay.l1 * (ax.l0 * cv[2] + ax.l1 * cv[3]);
            r4[jj] = ACT == GT_ACT_SILU ? silu_f(rz) : fmaxf(rz, 0.f);
            const unsigned d4 = (cv[0] > 0.f ? 1u : 0u) | (cv[1] > 0.f ? 2u : 0u) | (cv[2] > 0.f ? 4u : 0u) | (cv[3] > 0.f ? 8u : 0u);
            n16 |= (r4[jj] > 0.f ? d4 : 0u) << (4 * jj);
        }
        nib |= (unsigned long long)n16 << (4 * j4);
        (void)w00; (void)w01; (void)w10; (void)w11;
        const int c = c0 + j4;
        if (p.y_nhwc) {                       // a pixel's four channels: one 16-byte store (Cout % 4 == 0 checked on the host)
            *reinterpret_cast<f32x4*>(p.y + ((int64_t)b * p.Ho * p.Wo + e) * p.Cout + c) = f32x4{r4[0], r4[1], r4[2], r4[3]};
        } else {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (c + jj < p.Cout) p.y[((int64_t)b * p.Cout + c + jj) * p.Ho * p.Wo + e] = r4[jj];
        }
    }
    if (p.bits) p.bits[((int64_t)b * (p.Cout >> 4) + bc) * (p.Ho * p.Wo) + e] = nib;   // CR_CH == 16: one word per thread
}
static_assert(CR_CH == 16, "conv_resize_fwd_kernel packs the decisions of its 16 channels into one 64-bit word");

// Backward: weight gradient only (the fused path is used when the input needs no gradient).
// Output-side formulation: with R the bilinear operator, G = g .* [y > 0], and D = keep .* [y0 > 0],
//     dW[c][ci][k] = sum_px (R^T G)[px] D[px] x[px + off_k]  =  sum_o G[o] * sum_{4 taps t} w_t D[src_t] x[src_t + off_k]
// so a thread walks OUTPUT pixels (coalesced reads of g and y, no gather, the same 3x3 patches as the forward)
// and accumulates dW for CRB_CG channels in registers over CRB_PXT pixels before one block reduction.
constexpr int CRB_PXT = 8;
constexpr int CRB_CG = 8;
static_assert(CRB_CG % 4 == 0 && CRB_CG >= 4, "the channels-last paths read a pixel's CRB_CG channels as float4 groups");
// the one-channel instance is compiled for two resident waves per SIMD
template <int CIN, bool BITS = false, int ACT = GT_ACT_RELU>
__global__ __launch_bounds__(256, (CIN == 1 ? 2 : 1)) void conv_resize_bwd_kernel(const ConvResizeP p) {
    static_assert(!BITS || CRB_CG == 8, "the recorded decisions are read as one 32-bit half word: eight channels per thread");
    static_assert(!BITS || ACT == GT_ACT_RELU, "decision bits describe ReLUs");
    __shared__ float sw[BITS ? 1 : CRB_CG * CIN * 9];
    __shared__ float red[4][CRB_CG * CIN * 9];
    // channels-first: blockIdx = (pixel strip, channel group).  channels-last: a strip's channel groups read the same
    // 512-byte rows of g and y, 32 bytes each: they are put on ONE XCD next to each other (1-D grid, block id % 8 = XCD), so
    // a row is fetched into one L2 once instead of into all eight (measured 3.3 GB -> of HBM reads for 0.8 GB of g and y)
    int bc, bx, nbx, b;
    if (p.y_nhwc) {                                 // strips numbered over the whole batch: every XCD gets work
        const int ncg = (p.Cout + CRB_CG - 1) / CRB_CG;
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        const int gs = xcd + 8 * (j / ncg);
        bc = j % ncg;
        nbx = p.nstrips;
        if (gs >= nbx * p.B) return;
        b = gs / nbx;
        bx = gs - b * nbx;
    } else {
        bc = blockIdx.y; bx = blockIdx.x; nbx = gridDim.x; b = blockIdx.z;
    }
    const int c0 = bc * CRB_CG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!BITS) {
        for (int i = threadIdx.x; i < CRB_CG * CIN * 9; i += 256) {
            const int c = c0 + i / (CIN * 9);
            sw[i] = (c < p.Cout) ? p.w[(int64_t)c * CIN * 9 + i % (CIN * 9)] : 0.f;
        }
        __syncthreads();
    }
    const uint32_t plane = (uint32_t)(p.H * p.W);
    const int oplane = p.Ho * p.Wo;
    const uint32_t key = drop_key_dev(p.drop);
    float acc[CRB_CG][CIN * 9];
#pragma unroll
    for (int j = 0; j < CRB_CG; ++j)
#pragma unroll
        for (int k = 0; k < CIN * 9; ++k) acc[j][k] = 0.f;

#pragma unroll 1
    for (int it = 0; it < CRB_PXT; ++it) {
        const int e = (bx * CRB_PXT + it) * 256 + threadIdx.x;
        if (e >= oplane) continue;
        const int oy = e / p.Wo, ox = e - oy * p.Wo;
        Axis ay = axis_of(oy, p.sy, p.H), ax = axis_of(ox, p.sx, p.W);
        float pt[CIN][4][9];
        uint32_t toff[4];
        if (BITS) {
            // The four 3x3 patches are windows of ONE 4x4 neighbourhood around (i0 - 1, i0 - 1) when i1 = i0 + 1: 16 loads
            // instead of 36.  At the last row / column i1 = i0: both taps of that axis are the same source pixel (same
            // patch, same recorded decision), so its weight moves to tap 0 and tap 1 (which would read the window one
            // further, i.e. something else) gets weight zero.
            if (ay.i1 == ay.i0) { ay.l0 += ay.l1; ay.l1 = 0.f; }
            if (ax.i1 == ax.i0) { ax.l0 += ax.l1; ax.l1 = 0.f; }
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
                const float* xp = p.x + ((int64_t)b * CIN + ci) * plane;
                float nb[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int yy = ay.i0 - 1 + r, yc = yy < 0 ? 0 : (yy >= p.H ? p.H - 1 : yy);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int xx = ax.i0 - 1 + q, xc = xx < 0 ? 0 : (xx >= p.W ? p.W - 1 : xx);
                        const float v = xp[yc * p.W + xc];
                        nb[r][q] = (yy == yc && xx == xc) ? v : 0.f;
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) pt[ci][t][dy * 3 + dx] = nb[(t >> 1) + dy][(t & 1) + dx];
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int iy = (t & 2) ? ay.i1 : ay.i0, ix = (t & 1) ? ax.i1 : ax.i0;
                toff[t] = (uint32_t)(iy * p.W + ix);
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci)
                    load_patch_clamped(p.x + ((int64_t)b * CIN + ci) * plane, p.H, p.W, iy, ix, pt[ci][t]);
            }
        }
        const float wt[4] = {ay.l0 * ax.l0, ay.l0 * ax.l1, ay.l1 * ax.l0, ay.l1 * ax.l1};
        float gl[CRB_CG], yl[CRB_CG];       // channels-last: the pixel's eight channels are 32 contiguous bytes of g and y
        uint32_t dec = 0u;                  // BITS: the forward's decisions for these eight channels, 4 bits each
        if (p.y_nhwc) {
            const int64_t o8 = ((int64_t)b * oplane + e) * p.Cout + c0;           // Cout % 8 == 0 checked on the host
#pragma unroll
            for (int h = 0; h < CRB_CG / 4; ++h) {
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.g + o8 + 4 * h);
#pragma unroll
                for (int t = 0; t < 4; ++t) gl[4 * h + t] = g4[t];
                if (!BITS && ACT == GT_ACT_RELU) {
                    const f32x4 y4 = *reinterpret_cast<const f32x4*>(p.y + o8 + 4 * h);
#pragma unroll
                    for (int t = 0; t < 4; ++t) yl[4 * h + t] = y4[t];
                }
            }
            if (BITS) {
                const unsigned long long w64 = p.bits[((int64_t)b * (p.Cout >> 4) + (c0 >> 4)) * oplane + e];
                dec = (c0 & 8) ? (uint32_t)(w64 >> 32) : (uint32_t)w64;
            }
        }
#pragma unroll          // full unroll: acc[j][..] must be statically indexed to stay in registers
        for (int j = 0; j < CRB_CG; ++j) {
            const int c = min(c0 + j, p.Cout - 1);                 // clamped: tail channels are not stored
            float go;
            float coef[4];
            if (BITS) {                     // decisions recorded by the forward (they include [y > 0]): no conv, no mask draw
                go = gl[j] * p.drop.scale;
#pragma unroll
                for (int t = 0; t < 4; ++t) coef[t] = (dec & (1u << (4 * j + t))) ? wt[t] * go : 0.f;
            } else {
                if (ACT == GT_ACT_SILU) go = p.y_nhwc ? gl[j] : p.g[((int64_t)b * p.Cout + c) * oplane + e];
                else if (p.y_nhwc) go = (yl[j] > 0.f) ? gl[j] : 0.f;
                else {
                    const int64_t o = ((int64_t)b * p.Cout + c) * oplane + e;
                    go = (p.y[o] > 0.f) ? p.g[o] : 0.f;
                }
                float cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const float wv = sw[(j * CIN + ci) * 9 + k];
#pragma unroll
                        for (int t = 0; t < 4; ++t) cv[t] = fmaf(wv, pt[ci][t][k], cv[t]);
                    }
                const uint32_t cbase = ((uint32_t)b * (uint32_t)p.Cout + (uint32_t)c) * plane;
                if (ACT == GT_ACT_SILU) {
                    // both SiLUs re-evaluated: a_t = silu(m_t conv_t), r = bilinear(a), d out / d conv_t = silu'(r) w_t m_t silu'(m_t conv_t)
                    float av[4], dav[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float m = p.drop.thresh ? drop_mul(p.drop, key, cbase + toff[t]) : p.drop.scale;
                        silu_both(cv[t] * m, av[t], dav[t]);
                        dav[t] *= m;
                    }
                    const float rz = ay.l0 * (ax.l0 * av[0] + ax.l1 * av[1]) + ay.l1 * (ax.l0 * av[2] + ax.l1 * av[3]);
                    go *= dsilu_f(rz);
#pragma unroll
                    for (int t = 0; t < 4; ++t) coef[t] = wt[t] * dav[t] * go;
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float m = p.drop.thresh ? drop_mul(p.drop, key, cbase + toff[t]) : p.drop.scale;
                        coef[t] = (cv[t] * m > 0.f) ? wt[t] * m * go : 0.f;
                    }
                }
            }
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    float a = acc[j][ci * 9 + k];
#pragma unroll
                    for (int t = 0; t < 4; ++t) a = fmaf(coef[t], pt[ci][t][k], a);
                    acc[j][ci * 9 + k] = a;
                }
        }
    }
    // wave reduction, then the 4 waves through LDS (fixed order -> deterministic)
#pragma unroll
    for (int j = 0; j < CRB_CG; ++j)
#pragma unroll
        for (int k = 0; k < CIN * 9; ++k) {
            const float v = wave_sum_lane63(acc[j][k]);      // 72 sums per lane: DPP adds (shuffles: 432 LDS round trips)
            if (lane == 63) red[wave][j * CIN * 9 + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < CRB_CG * CIN * 9) {
        const int c = c0 + threadIdx.x / (CIN * 9);
        if (c < p.Cout) {
            float* part = p.partial + ((int64_t)(b * nbx + bx) * p.Cout) * CIN * 9;
            part[(int64_t)c0 * CIN * 9 + threadIdx.x] =
                red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        }
    }
}

}  // namespace gt

using namespace gt;

static int check_conv_resize(const void* x, const void* w, const void* y, int B, int Cin, int Cout, int H, int W,
                             int Ho, int Wo, const gt_dropout* drop, int act) {
    if (!x || !w || !y || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return GT_EINVAL;
    if (Cin > CR_MAXCI || (act != GT_ACT_RELU && act != GT_ACT_SILU)) return GT_ENOTSUP;
    if (B > 65535) return GT_EINVAL;
    if (drop && drop->p > 0.f && !drop->seed) return GT_EINVAL;
    if (drop && (drop->p < 0.f || drop->p >= 1.f)) return GT_EINVAL;
    return 0;
}

// geometry, scales and dropout of a launch; the entry points assign what is theirs (y, g, partial, nstrips, bits) by name
static ConvResizeP make_conv_resize_p(const float* x, const float* w, int B, int Cin, int Cout, int H, int W, int Ho, int Wo,
                                      const gt_dropout* drop, int y_nhwc) {
    ConvResizeP p{};
    p.x = x; p.w = w;
    p.B = B; p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    p.sy = scale_of(H, Ho); p.sx = scale_of(W, Wo);
    p.drop = make_drop(drop);
    p.y_nhwc = y_nhwc;
    return p;
}

// f(std::integral_constant<int, CIN>) for the kernel instance that serves Cin input channels: 1, 2 and 3 exactly, everything
// else (check_conv_resize admits up to CR_MAXCI) the four-channel one
template <typename F>
static void with_cin(int Cin, F&& f) {
    switch (Cin) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, CR_MAXCI>{}); break;
    }
}

static int conv_resize_fwd(const float* x, const float* w, float* y, int32_t B, int32_t Cin,
                           int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                           const gt_dropout* drop, int32_t act, int y_nhwc, void* bits, void* stream) {
    if (int rc = check_conv_resize(x, w, y, B, Cin, Cout, H, W, Ho, Wo, drop, act)) return rc;
    if (y_nhwc && ((Cout & 7) || (reinterpret_cast<uintptr_t>(y) & 15))) return GT_ENOTSUP;
    if (bits && (!y_nhwc || (Cout & 15) || (reinterpret_cast<uintptr_t>(bits) & 7) || act != GT_ACT_RELU)) return GT_ENOTSUP;
    ConvResizeP p = make_conv_resize_p(x, w, B, Cin, Cout, H, W, Ho, Wo, drop, y_nhwc);
    p.y = y;
    p.bits = reinterpret_cast<unsigned long long*>(bits);
    dim3 grid((unsigned)ceil_div((int64_t)Ho * Wo, 256), (unsigned)ceil_div(Cout, CR_CH), (unsigned)B);
    if (y_nhwc) std::swap(grid.x, grid.y);
    hipStream_t st = (hipStream_t)stream;
    with_cin(Cin, [&](auto cin) {
        constexpr int CIN = decltype(cin)::value;
        if (act == GT_ACT_SILU) hipLaunchKernelGGL((conv_resize_fwd_kernel<CIN, GT_ACT_SILU>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((conv_resize_fwd_kernel<CIN>), grid, dim3(256), 0, st, p);
    });
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_debug_conv0_mask(void* mask, void* stream) {
    unsigned char* m = reinterpret_cast<unsigned char*>(mask);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GT_EINVAL;     // launches in flight keep their setting
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_conv0_mask), &m, sizeof(m), 0, hipMemcpyHostToDevice);
}

extern "C" int gt_conv3x3_resize_fwd(const float* x, const float* w, float* y, int32_t B, int32_t Cin,
                                     int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                     const gt_dropout* drop, int32_t act, void* stream) {
    return conv_resize_fwd(x, w, y, B, Cin, Cout, H, W, Ho, Wo, drop, act, 0, nullptr, stream);
}
extern "C" int gt_conv3x3_resize_fwd_nhwc(const float* x, const float* w, float* y, int32_t B, int32_t Cin,
                                          int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                          const gt_dropout* drop, int32_t act, void* relu_bits, void* stream) {
    return conv_resize_fwd(x, w, y, B, Cin, Cout, H, W, Ho, Wo, drop, act, 1, relu_bits, stream);
}
extern "C" int64_t gt_conv3x3_resize_bits_bytes(int32_t B, int32_t Cout, int32_t Ho, int32_t Wo) {
    if (B <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || (Cout & 15)) return 0;
    return (int64_t)B * Ho * Wo * (Cout / 16) * 8;
}

extern "C" int64_t gt_conv3x3_resize_bwd_ws_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W) {
    (void)H; (void)W;      // partial slabs are per (image, strip of OUTPUT pixels): bounded by the input size
    return (int64_t)B * ceil_div((int64_t)H * W, 256 * CRB_PXT) * Cout * Cin * 9 * (int64_t)sizeof(float);
}

static int conv_resize_bwd(const float* g, const float* y, const float* x, const float* w, int32_t B,
                           int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                           const gt_dropout* drop, int32_t act, float* dw, void* ws, int64_t ws_bytes, int y_nhwc,
                           const void* bits, void* stream) {
    if (bits && (!y_nhwc || (Cout & 15) || (reinterpret_cast<uintptr_t>(bits) & 7) || act != GT_ACT_RELU))
        return GT_ENOTSUP;
    const bool no_y = bits || act == GT_ACT_SILU;    // the SiLU backward re-evaluates both activations: y is not read
    if (int rc = check_conv_resize(x, w, no_y ? (const void*)g : (const void*)y, B, Cin, Cout, H, W, Ho, Wo, drop, act)) return rc;
    if (!g || !dw) return GT_EINVAL;
    if (no_y && !y) y = g;                           // not read (alignment checks below see a valid pointer)
    // channels-last: a block walks whole channel groups of CRB_CG (a build-time constant) as aligned float4s
    if (y_nhwc && ((Cout & 7) || (Cout % CRB_CG) || ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(g)) & 15)))
        return GT_ENOTSUP;
    if (!ws || ws_bytes < gt_conv3x3_resize_bwd_ws_bytes(B, Cin, Cout, H, W)) return GT_EWS;
    ConvResizeP p = make_conv_resize_p(x, w, B, Cin, Cout, H, W, Ho, Wo, drop, y_nhwc);
    p.y = const_cast<float*>(y);
    p.g = g;
    p.partial = reinterpret_cast<float*>(ws);
    p.bits = reinterpret_cast<unsigned long long*>(const_cast<void*>(bits));
    if (ceil_div((int64_t)Ho * Wo, 256 * CRB_PXT) > ceil_div((int64_t)H * W, 256 * CRB_PXT)) return GT_ENOTSUP;
    const int nx = ceil_div((int64_t)Ho * Wo, 256 * CRB_PXT);
    dim3 grid((unsigned)nx, (unsigned)ceil_div(Cout, CRB_CG), (unsigned)B);
    if (y_nhwc) {
        p.nstrips = nx;
        grid = dim3((unsigned)(ceil_div(Cout, CRB_CG) * (((int64_t)nx * B + 7) / 8 * 8)), 1u, 1u);
    }
    hipStream_t st = (hipStream_t)stream;
    with_cin(Cin, [&](auto cin) {
        constexpr int CIN = decltype(cin)::value;
        if (bits) hipLaunchKernelGGL((conv_resize_bwd_kernel<CIN, true>), grid, dim3(256), 0, st, p);
        else if (act == GT_ACT_SILU) hipLaunchKernelGGL((conv_resize_bwd_kernel<CIN, false, GT_ACT_SILU>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((conv_resize_bwd_kernel<CIN>), grid, dim3(256), 0, st, p);
    });
    GT_LAUNCH_CHECK();
    const int64_t n = (int64_t)Cout * Cin * 9;
    return gt_slab_reduce(p.partial, n, B * nx, n, 1.f, dw, stream);
}

extern "C" int gt_conv3x3_resize_bwd(const float* g, const float* y, const float* x, const float* w, int32_t B,
                                     int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                     const gt_dropout* drop, int32_t act, float* dw, void* ws, int64_t ws_bytes,
                                     void* stream) {
    return conv_resize_bwd(g, y, x, w, B, Cin, Cout, H, W, Ho, Wo, drop, act, dw, ws, ws_bytes, 0, nullptr, stream);
}
extern "C" int gt_conv3x3_resize_bwd_nhwc(const float* g, const float* y, const float* x, const float* w, int32_t B,
                                          int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                          const gt_dropout* drop, int32_t act, const void* relu_bits, float* dw,
                                          void* ws, int64_t ws_bytes, void* stream) {
    return conv_resize_bwd(g, y, x, w, B, Cin, Cout, H, W, Ho, Wo, drop, act, dw, ws, ws_bytes, 1, relu_bits, stream);
}
