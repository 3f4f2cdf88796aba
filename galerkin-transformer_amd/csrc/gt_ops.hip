// Elementwise and reduction helpers of libgt_hip (gfx950), and the library's identity (gt_abi_version, gt_target_arch):
//   - stateless dropout (seed advance, mask apply), the fused dropout / activation pair of the conv blocks, activation backward
//   - column sums and slab reductions (deterministic two-pass); gt_slab_reduce also closes the partial sums of the head-norm,
//     Galerkin, LayerNorm and mode-mixing backwards (units of their own)
// Here as in those units: all launches go to the caller's stream; no allocation, no synchronisation.
#include "gt_common.h"

namespace gt {

__global__ void seed_advance_kernel(uint64_t* s, uint64_t inc) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *s += inc;
}

__global__ void dropout_apply_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n,
                                     DropDev d) {
    const uint32_t key = drop_key_dev(d);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = x[i] * (d.thresh ? drop_mul(d, key, (uint32_t)i) : d.scale);
}

// y = act2(drop2(act1(drop1(x)))) in one pass (BWD: gx = gy * dy/dx, recomputed from x): the elementwise tail
// of Conv2dResBlock (layers.py:88-150) and of Interp2dUpsample's conv branch (layers.py:658-668), where the
// reference runs up to four separate elementwise kernels over a [B, C, H, W] map.  Mask index = element index.
__device__ __forceinline__ void act_pair(int act, float v, float& a, float& da) {
    if (act == GT_ACT_SILU) silu_both(v, a, da);
    else if (act == GT_ACT_RELU) { a = fmaxf(v, 0.f); da = v > 0.f ? 1.f : 0.f; }
    else if (act == GT_ACT_GELU) gelu_both(v, a, da);
    else { a = v; da = 1.f; }
}
template <bool BWD>
__device__ __forceinline__ float dropact_one(float x, float gy, uint32_t idx, const DropDev& d1, uint32_t k1, int a1,
                                             const DropDev& d2, uint32_t k2, int a2) {
    const float m1 = d1.thresh ? drop_mul(d1, k1, idx) : d1.scale;
    const float m2 = d2.thresh ? drop_mul(d2, k2, idx) : d2.scale;
    float a, da, b, db;
    act_pair(a1, x * m1, a, da);
    act_pair(a2, a * m2, b, db);
    return BWD ? gy * db * m2 * da * m1 : b;
}
template <bool BWD>
__global__ __launch_bounds__(256) void dropact_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                      float* __restrict__ out, int64_t n, DropDev d1, int a1,
                                                      DropDev d2, int a2, int vec) {
    const uint32_t k1 = drop_key_dev(d1), k2 = drop_key_dev(d2);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nth) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
            f32x4 gv = {0.f, 0.f, 0.f, 0.f}, o;
            if (BWD) gv = reinterpret_cast<const f32x4*>(gy)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = dropact_one<BWD>(xv[j], gv[j], (uint32_t)(4 * i + j), d1, k1, a1, d2, k2, a2);
            reinterpret_cast<f32x4*>(out)[i] = o;
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nth)
            out[i] = dropact_one<BWD>(x[i], BWD ? gy[i] : 0.f, (uint32_t)i, d1, k1, a1, d2, k2, a2);
    } else {
        for (int64_t i = tid; i < n; i += nth)
            out[i] = dropact_one<BWD>(x[i], BWD ? gy[i] : 0.f, (uint32_t)i, d1, k1, a1, d2, k2, a2);
    }
}

// out[i] = alpha * sum_k slabs[k*stride + i].  A block owns 16 consecutive outputs; its 16 slab
// lanes each walk every 16th slab (fixed order -> deterministic), then a fixed LDS tree combines.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slabs, int64_t stride,
                                                          int n_slabs, int64_t n, float alpha,
                                                          float* __restrict__ out) {
    __shared__ float red[16][17];
    const int ox = threadIdx.x & 15, sy = threadIdx.x >> 4;
    const int64_t i = (int64_t)blockIdx.x * 16 + ox;
    float s = 0.f;
    if (i < n) {
        // 4 independent partial sums per lane keep 4 loads in flight; combined in a fixed order
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = sy;
        for (; k + 48 < n_slabs; k += 64) {
            s0 += slabs[(int64_t)k * stride + i];
            s1 += slabs[(int64_t)(k + 16) * stride + i];
            s2 += slabs[(int64_t)(k + 32) * stride + i];
            s3 += slabs[(int64_t)(k + 48) * stride + i];
        }
        for (; k < n_slabs; k += 16) s0 += slabs[(int64_t)k * stride + i];
        s = (s0 + s1) + (s2 + s3);
    }
    red[sy][ox] = s;
    __syncthreads();
    if (sy == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][ox];
        out[i] = alpha * t;
    }
}

// partial[g][n] = sum over rows r = g*16+ry, stepping gridDim.y*16, of A[r][n]*keep(r,n).
// Block = 16 float4 column groups (64 columns) x 16 row lanes; fixed-order LDS combine (deterministic).
constexpr int CS_MAXG = 512;
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ A, int64_t lda, int M,
                                                     int N, DropDev d, int vec, float* __restrict__ partial) {
    __shared__ float red[16][65];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int n = blockIdx.x * 64 + 4 * cx;
    const uint32_t key = drop_key_dev(d);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (n < N) {
        const bool full = vec && (n + 3 < N);
        for (int r = blockIdx.y * 16 + ry; r < M; r += gridDim.y * 16) {
            const float* p = A + (int64_t)r * lda + n;
            float v0, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            if (full) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(p);
                v0 = t[0]; v1 = t[1]; v2 = t[2]; v3 = t[3];
            } else {
                v0 = p[0];
                if (n + 1 < N) v1 = p[1];
                if (n + 2 < N) v2 = p[2];
                if (n + 3 < N) v3 = p[3];
            }
            if (d.thresh) {
                const uint32_t di = (uint32_t)((int64_t)r * N + n);
                v0 *= drop_mul(d, key, di); v1 *= drop_mul(d, key, di + 1);
                v2 *= drop_mul(d, key, di + 2); v3 *= drop_mul(d, key, di + 3);
            }
            s0 += v0; s1 += v1; s2 += v2; s3 += v3;
        }
    }
    red[ry][4 * cx + 0] = s0; red[ry][4 * cx + 1] = s1; red[ry][4 * cx + 2] = s2; red[ry][4 * cx + 3] = s3;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int nn = blockIdx.x * 64 + threadIdx.x;
        if (nn < N) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
            partial[(int64_t)blockIdx.y * N + nn] = t * (d.thresh ? 1.f : d.scale);
        }
    }
}

__global__ void act_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ pre,
                               float* __restrict__ dpre, int64_t n, int act) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float x = pre[i], g = dout[i];
        dpre[i] = (act == GT_ACT_SILU) ? g * dsilu_f(x) : (act == GT_ACT_RELU ? (x > 0.f ? g : 0.f) : g);
    }
}

static inline int grid_for(int64_t n, int block = 256, int cap = 4096) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, cap));
}

}  // namespace gt

using namespace gt;

extern "C" int gt_abi_version(void) { return GT_ABI_VERSION; }
extern "C" const char* gt_target_arch(void) { return "gfx950"; }

extern "C" int gt_seed_advance(uint64_t* seed, uint64_t inc, void* stream) {
    if (!seed) return GT_EINVAL;
    hipLaunchKernelGGL(seed_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, seed, inc);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_dropout_apply(const float* x, float* out, int64_t n, const gt_dropout* d, void* stream) {
    if (!x || !out || n < 0) return GT_EINVAL;
    if (d && d->p > 0.f && !d->seed) return GT_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(dropout_apply_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, out,
                       n, make_drop(d));
    GT_LAUNCH_CHECK();
    return 0;
}

static int dropact_launch(bool bwd, const float* x, const float* gy, float* out, int64_t n, const gt_dropout* d1,
                          int32_t act1, const gt_dropout* d2, int32_t act2, void* stream) {
    if (!x || !out || n < 0 || (bwd && !gy)) return GT_EINVAL;
    if ((d1 && d1->p > 0.f && !d1->seed) || (d2 && d2->p > 0.f && !d2->seed)) return GT_EINVAL;
    if (act1 < GT_ACT_NONE || act1 > GT_ACT_GELU || act2 < GT_ACT_NONE || act2 > GT_ACT_GELU) return GT_EINVAL;
    if (n == 0) return 0;
    const int vec = !misaligned16(x, gy, out);
    const int grid = grid_for((n + 3) / 4, 256, 8192);
    const auto kern = bwd ? dropact_kernel<true> : dropact_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, gy, out, n, make_drop(d1), act1, make_drop(d2), act2, vec);
    GT_LAUNCH_CHECK();
    return 0;
}
extern "C" int gt_dropact_fwd(const float* x, float* y, int64_t n, const gt_dropout* d1, int32_t act1,
                              const gt_dropout* d2, int32_t act2, void* stream) {
    return dropact_launch(false, x, nullptr, y, n, d1, act1, d2, act2, stream);
}
extern "C" int gt_dropact_bwd(const float* x, const float* gy, float* gx, int64_t n, const gt_dropout* d1,
                              int32_t act1, const gt_dropout* d2, int32_t act2, void* stream) {
    return dropact_launch(true, x, gy, gx, n, d1, act1, d2, act2, stream);
}

extern "C" int gt_slab_reduce(const float* slabs, int64_t stride, int32_t n_slabs, int64_t n, float alpha,
                              float* out, void* stream) {
    if (!slabs || !out || n_slabs <= 0 || n <= 0) return GT_EINVAL;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(ceil_div(n, 16)), dim3(256), 0, (hipStream_t)stream, slabs,
                       stride, n_slabs, n, alpha, out);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_colsum(const float* A, int64_t lda, int32_t M, int32_t N, const gt_dropout* a_drop,
                         float a_sign, float* out, void* ws, int64_t ws_bytes, void* stream) {
    if (!A || !out || M <= 0 || N <= 0) return GT_EINVAL;
    if (a_drop && a_drop->p > 0.f && !a_drop->seed) return GT_EINVAL;
    const int colb = ceil_div(N, 64);
    const int chunks = std::max(1, std::min({ceil_div(M, 128), CS_MAXG, std::max(1, 768 / colb)}));
    if (!ws || ws_bytes < (int64_t)chunks * N * (int64_t)sizeof(float)) return GT_EWS;
    float* partial = reinterpret_cast<float*>(ws);
    const int vec = !misaligned16(A) && ((lda & 3) == 0);
    hipLaunchKernelGGL(colsum_kernel, dim3(colb, chunks), dim3(256), 0, (hipStream_t)stream, A, lda, M, N,
                       make_drop(a_drop, a_sign), vec, partial);
    GT_LAUNCH_CHECK();
    return gt_slab_reduce(partial, N, chunks, N, 1.f, out, stream);
}

extern "C" int gt_act_bwd(const float* dout, const float* pre, float* dpre, int64_t n, int32_t act,
                          void* stream) {
    if (!dout || !pre || !dpre || n <= 0) return GT_EINVAL;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dout, pre,
                       dpre, n, act);
    GT_LAUNCH_CHECK();
    return 0;
}
