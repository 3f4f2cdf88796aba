// Spatial half of the 3x3 / stride-2 transposed convolution, channels-last (gfx950): nn.ConvTranspose2d(k=3, stride=2) of the
// reference's DeConv2dBlock (libs/layers.py:515-559).  The contraction over the channels is a gt_gemm product of the caller:
//     cols[(b, iy, ix)][(ky, kx, co)] = sum_ci x[b, iy, ix, ci] w[ci, co, ky, kx]            [B H W, 9 Cout]
// and this unit moves between `cols` and the image in GATHER form.  With  oy = 2 iy - pad + ky  an output row reads the taps
// ky for which (oy + pad - ky) is even and iy = (oy + pad - ky) / 2 lies in [0, H): one tap where oy + pad is odd, two where it
// is even, likewise along x -- at most four of the nine taps per output pixel.
//   forward : y[b, oy, ox, co] = act(dropout(bias[co] + sum over those taps of cols[...]))   -- one thread per float4 of
//             channels of one output pixel, taps summed in the fixed order (ky, kx) ascending; bias, the stateless dropout
//             mask (index = the element's index in y) and the activation are applied where y is stored;
//   backward: dcols[(b, iy, ix)][(ky, kx, co)] = dy[b, 2 iy - pad + ky, 2 ix - pad + kx, co] * act' * mask (0 outside the
//             image) -- one thread per float4 of one (pixel, tap); the gate is applied where dy is gathered, from `gate` =
//             the pre-dropout sum (SiLU) or y itself (ReLU) and the mask re-drawn from (seed, salt, index);
//   dbias   : db[co] = sum over the output pixels of dy * act' * mask -- per-chunk partial rows in ws, closed by
//             gt_slab_reduce in a fixed order.  (The column sums of dcols are NOT this sum: they count an output pixel once
//             per tap that reaches it.)
// Every output value is written once by one thread; no atomics, so results are identical from run to run.
#include "gt_common.h"

namespace gt {

struct DeconvP {
    int B, H, W, C, Ho, Wo, pad;      // C = Cout
};

// d y / d (pre-dropout sum) for one element: mask * act'(mask * u)
__device__ __forceinline__ float deconv_gate(int act, float gate, float m) {
    if (act == GT_ACT_SILU) return m * dsilu_f(gate * m);      // gate = u, the sum in front of the dropout
    if (act == GT_ACT_RELU) return gate > 0.f ? m : 0.f;       // gate = y = relu(m u): positive <=> kept and u > 0
    return m;
}

__global__ __launch_bounds__(256) void deconv_gather_fwd_kernel(const float* __restrict__ cols, const float* __restrict__ bias,
                                                                float* __restrict__ y, float* __restrict__ pre, DeconvP p,
                                                                DropDev d, int act) {
    const uint32_t key = drop_key_dev(d);
    const int C4 = p.C >> 2;
    const int64_t total = (int64_t)p.B * p.Ho * p.Wo * C4, nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t ldc = 9 * (int64_t)p.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        const int c = 4 * (int)(r % C4); r /= C4;
        const int ox = (int)(r % p.Wo); r /= p.Wo;
        const int oy = (int)(r % p.Ho); r /= p.Ho;
        const int b = (int)r;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = oy + p.pad - ky;
            if (ty < 0 || (ty & 1) || (ty >> 1) >= p.H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = ox + p.pad - kx;
                if (tx < 0 || (tx & 1) || (tx >> 1) >= p.W) continue;
                const int64_t pix = ((int64_t)b * p.H + (ty >> 1)) * p.W + (tx >> 1);
                acc += *reinterpret_cast<const f32x4*>(cols + pix * ldc + (ky * 3 + kx) * p.C + c);
            }
        }
        if (bias) acc += *reinterpret_cast<const f32x4*>(bias + c);
        if (pre) reinterpret_cast<f32x4*>(pre)[i] = acc;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m = d.thresh ? drop_mul(d, key, (uint32_t)(4 * i + j)) : 1.f;
            const float v = acc[j] * m;
            o[j] = act == GT_ACT_SILU ? silu_f(v) : (act == GT_ACT_RELU ? fmaxf(v, 0.f) : v);
        }
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
}

__global__ __launch_bounds__(256) void deconv_gather_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ gate,
                                                                float* __restrict__ dcols, DeconvP p, DropDev d, int act) {
    const uint32_t key = drop_key_dev(d);
    const int C4 = p.C >> 2;
    const int64_t total = (int64_t)p.B * p.H * p.W * 9 * C4, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nth) {
        int64_t r = i;
        const int c = 4 * (int)(r % C4); r /= C4;
        const int tap = (int)(r % 9); r /= 9;
        const int ix = (int)(r % p.W); r /= p.W;
        const int iy = (int)(r % p.H); r /= p.H;
        const int b = (int)r;
        const int oy = 2 * iy - p.pad + tap / 3, ox = 2 * ix - p.pad + tap % 3;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (oy >= 0 && oy < p.Ho && ox >= 0 && ox < p.Wo) {
            const int64_t e = (((int64_t)b * p.Ho + oy) * p.Wo + ox) * p.C + c;
            const f32x4 g = *reinterpret_cast<const f32x4*>(dy + e);
            f32x4 gt4 = {0.f, 0.f, 0.f, 0.f};
            if (gate) gt4 = *reinterpret_cast<const f32x4*>(gate + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float m = d.thresh ? drop_mul(d, key, (uint32_t)(e + j)) : 1.f;
                o[j] = g[j] * deconv_gate(act, gt4[j], m);
            }
        }
        reinterpret_cast<f32x4*>(dcols)[i] = o;
    }
}

// partial[chunk][c] = sum over the output pixels q = chunk*16 + ry, stepping gridDim.y*16, of dy[q][c] * gate.  Block = 16 float4
// column groups (64 channels) x 16 pixel lanes; fixed-order LDS combine (the layout of gt_colsum's kernel).
constexpr int DC_MAXG = 512;
__global__ __launch_bounds__(256) void deconv_dbias_kernel(const float* __restrict__ dy, const float* __restrict__ gate,
                                                           float* __restrict__ partial, int64_t Q, int C, DropDev d, int act) {
    __shared__ float red[16][65];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + 4 * cx;
    const uint32_t key = drop_key_dev(d);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        for (int64_t q = (int64_t)blockIdx.y * 16 + ry; q < Q; q += (int64_t)gridDim.y * 16) {
            const int64_t e = q * C + c;
            const f32x4 g = *reinterpret_cast<const f32x4*>(dy + e);
            f32x4 gt4 = {0.f, 0.f, 0.f, 0.f};
            if (gate) gt4 = *reinterpret_cast<const f32x4*>(gate + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float m = d.thresh ? drop_mul(d, key, (uint32_t)(e + j)) : 1.f;
                s[j] += g[j] * deconv_gate(act, gt4[j], m);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[ry][4 * cx + j] = s[j];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = blockIdx.x * 64 + threadIdx.x;
        if (cc < C) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
            partial[(int64_t)blockIdx.y * C + cc] = t;
        }
    }
}

static inline int deconv_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

static inline int deconv_chunks(int64_t Q, int C) {
    const int colb = ceil_div(C, 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>({(Q + 127) / 128, (int64_t)DC_MAXG, (int64_t)std::max(1, 768 / colb)}));
}

// The shapes the transposed convolution is implemented for; fills the output size.  Cin only enters the caller's products,
// but it is refused here so that one place says what is supported.
static int deconv_shape(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pad, int32_t outpad, DeconvP* p) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || pad < 0 || outpad < 0) return GT_EINVAL;
    if (outpad > 1) return GT_EINVAL;                 // (output_padding must be smaller than the stride)
    const int64_t Ho = 2 * ((int64_t)H - 1) - 2 * (int64_t)pad + 3 + outpad, Wo = 2 * ((int64_t)W - 1) - 2 * (int64_t)pad + 3 + outpad;
    if (Ho <= 0 || Wo <= 0) return GT_EINVAL;
    if ((Cin & 3) || (Cout & 3)) return GT_ENOTSUP;   // float4 of channels everywhere
    if ((int64_t)B * Ho * Wo >= (1ll << 31) || (int64_t)B * H * W * 9 >= (1ll << 31)) return GT_ENOTSUP;
    if (p) *p = DeconvP{B, H, W, Cout, (int)Ho, (int)Wo, pad};
    return 0;
}

static int deconv_drop_check(const gt_dropout* d, int32_t act) {
    if (d && (d->p < 0.f || d->p >= 1.f || (d->p > 0.f && !d->seed))) return GT_EINVAL;
    if (act != GT_ACT_NONE && act != GT_ACT_RELU && act != GT_ACT_SILU) return GT_EINVAL;
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" int gt_deconv3x3s2_check(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pad, int32_t outpad) {
    return deconv_shape(B, H, W, Cin, Cout, pad, outpad, nullptr);
}

extern "C" int gt_deconv3x3s2_gather_fwd(const float* cols, const float* bias, float* y, float* pre, int32_t B, int32_t H,
                                         int32_t W, int32_t Cout, int32_t pad, int32_t outpad, const gt_dropout* drop,
                                         int32_t act, void* stream) {
    DeconvP p;
    if (int rc = deconv_shape(B, H, W, 4, Cout, pad, outpad, &p)) return rc;
    if (!cols || !y) return GT_EINVAL;
    if (int rc = deconv_drop_check(drop, act)) return rc;
    if (misaligned16(cols, bias, y, pre)) return GT_EALIGN;
    const int64_t n = (int64_t)B * p.Ho * p.Wo * (Cout / 4);
    hipLaunchKernelGGL(deconv_gather_fwd_kernel, dim3(deconv_grid(n)), dim3(256), 0, (hipStream_t)stream, cols, bias, y, pre, p,
                       make_drop(drop), act);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_deconv3x3s2_gather_bwd(const float* dy, const float* gate, float* dcols, int32_t B, int32_t H, int32_t W,
                                         int32_t Cout, int32_t pad, int32_t outpad, const gt_dropout* drop, int32_t act,
                                         void* stream) {
    DeconvP p;
    if (int rc = deconv_shape(B, H, W, 4, Cout, pad, outpad, &p)) return rc;
    if (!dy || !dcols || (act != GT_ACT_NONE && !gate)) return GT_EINVAL;
    if (int rc = deconv_drop_check(drop, act)) return rc;
    if (misaligned16(dy, gate, dcols)) return GT_EALIGN;
    const int64_t n = (int64_t)B * H * W * 9 * (Cout / 4);
    hipLaunchKernelGGL(deconv_gather_bwd_kernel, dim3(deconv_grid(n)), dim3(256), 0, (hipStream_t)stream, dy, gate, dcols, p,
                       make_drop(drop), act);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gt_deconv3x3s2_dbias_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout, int32_t pad, int32_t outpad) {
    DeconvP p;
    if (deconv_shape(B, H, W, 4, Cout, pad, outpad, &p)) return 0;
    return (int64_t)deconv_chunks((int64_t)B * p.Ho * p.Wo, Cout) * Cout * (int64_t)sizeof(float);
}

extern "C" int gt_deconv3x3s2_dbias(const float* dy, const float* gate, float* db, int32_t B, int32_t H, int32_t W,
                                    int32_t Cout, int32_t pad, int32_t outpad, const gt_dropout* drop, int32_t act, void* ws,
                                    int64_t ws_bytes, void* stream) {
    DeconvP p;
    if (int rc = deconv_shape(B, H, W, 4, Cout, pad, outpad, &p)) return rc;
    if (!dy || !db || (act != GT_ACT_NONE && !gate)) return GT_EINVAL;
    if (int rc = deconv_drop_check(drop, act)) return rc;
    if (misaligned16(dy, gate, ws)) return GT_EALIGN;
    const int64_t Q = (int64_t)B * p.Ho * p.Wo;
    const int chunks = deconv_chunks(Q, Cout);
    if (!ws || ws_bytes < (int64_t)chunks * Cout * (int64_t)sizeof(float)) return GT_EWS;
    float* partial = reinterpret_cast<float*>(ws);
    hipLaunchKernelGGL(deconv_dbias_kernel, dim3(ceil_div(Cout, 64), chunks), dim3(256), 0, (hipStream_t)stream, dy, gate,
                       partial, Q, Cout, make_drop(drop), act);
    GT_LAUNCH_CHECK();
    return gt_slab_reduce(partial, Cout, chunks, Cout, 1.f, db, stream);
}
