// Graph convolution against a dense per-channel edge tensor (gfx950): the GCN layer of the reference (GraphConvolution,
// layers.py:153-198; GCN, model.py:376-427), whose product is B*C independent n x n matrix-vector products
//     y[b,:,c] = E[b,c] s[b,:,c]                 (torch.matmul(edge, support.unsqueeze(-1)): a batched GEMM with N = 1).
// Pure streaming: 4 B C n^2 bytes of E against vectors n times smaller, so every kernel here is built around reading or
// writing E once, in its own row-major order, 1 KiB per wave instruction.
//   forward    : a block gathers the vector s[b,:,c] (n floats at stride ld) into LDS once and owns 32 rows of E[b,c]; a wave
//                takes four rows at a time (four independent 16-byte loads in flight per lane), reduces each by shuffles
//                and stores act(sum + bias).
//   bwd_data   : the transposed product dS[b,j,c] = sum_i E[b,c,i,j] g[b,i,c] WITHOUT a strided read: a block owns 256
//                columns, its four waves walk the rows i = w, w + 4, ... (eight rows in flight), each lane keeps the partial
//                sums of its four columns, and the four partial rows meet in LDS in the fixed order w = 0..3.
//   bwd_edge   : dE[b,c,i,j] = sum_{l<P} g_l[b,i,c] s_l[b,j,c] -- the rank-P update of a whole layer stack, written once.
//                A block owns 128 rows x 256 columns: the P column vectors go through LDS into registers (P x 4 per lane),
//                the P row vectors stay in LDS as [row][l] (a wave-uniform broadcast read per row), one 16-byte store per
//                lane and row.
// E arrives as up to three channel groups (dense [B, c_g, n, n] each), so the concatenation of the edge encoder's outputs
// and the split of its gradient are never made.  n % 4 == 0 with 16-byte aligned group pointers takes the 16-byte path;
// every other n (a (b,c) slice then starts off a 16-byte boundary: n^2 is odd at n = 33) takes the dword path, lane l on
// the columns l, l + 64, ... -- still whole 256-byte segments per wave instruction.  int64 offsets throughout.
// No atomics, fixed summation orders: bit-identical from run to run.  The caller's stream, no allocation, no scratch.
#include "gt_common.h"

namespace gt {

constexpr int GC_THREADS = 256;
constexpr int GC_FWD_ROWS = 32;      // rows of E per forward block: 8 per wave, four at a time
constexpr int GC_COLS = 256;         // columns per bwd_data / bwd_edge block: one 16-byte sweep of a wave
constexpr int GC_EDGE_ROWS = 128;    // rows per bwd_edge block
constexpr int GC_MAXP = GT_GRAPHCONV_MAX_PAIRS;

// the (b, c) slice of the group that holds channel c; nullptr if that group has no tensor (bwd_edge: skipped)
__device__ __forceinline__ float* gc_slice(const gt_edge_groups& eg, int b, int c, int n) {
    int g = 0, cc = c;
    if (cc >= eg.c[0]) { cc -= eg.c[0]; g = 1; if (cc >= eg.c[1]) { cc -= eg.c[1]; g = 2; } }
    float* base = g == 0 ? eg.e[0] : (g == 1 ? eg.e[1] : eg.e[2]);
    const int cg = g == 0 ? eg.c[0] : (g == 1 ? eg.c[1] : eg.c[2]);
    if (!base) return nullptr;
    return base + ((int64_t)b * cg + cc) * (int64_t)n * n;
}

template <bool VEC>
__global__ __launch_bounds__(GC_THREADS) void gc_fwd_kernel(gt_edge_groups eg, const float* __restrict__ S, int64_t lds,
                                                            const float* __restrict__ bias, float* __restrict__ Y, int64_t ldy,
                                                            int n, int act) {
    extern __shared__ float sv[];                   // s[b, :, c]
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < n; j += GC_THREADS) sv[j] = S[((int64_t)b * n + j) * lds + c];
    __syncthreads();
    const float* __restrict__ E = gc_slice(eg, b, c, n);
    const float bv = bias ? bias[c] : 0.f;
    const int wrow = blockIdx.x * GC_FWD_ROWS + wave * (GC_FWD_ROWS / 4);
#pragma unroll 1
    for (int r = 0; r < GC_FWD_ROWS / 4; r += 4) {
        const int i0 = wrow + r;
        if (i0 >= n) break;                         // wave-uniform
        const float* rp[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rp[q] = E + (int64_t)min(i0 + q, n - 1) * n;     // a row past the end re-reads the last one
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            for (int j = lane * 4; j < n; j += 4 * WAVE) {
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(sv + j);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 e = *reinterpret_cast<const f32x4*>(rp[q] + j);
                    acc[q] += e[0] * s4[0] + e[1] * s4[1] + e[2] * s4[2] + e[3] * s4[3];
                }
            }
        } else {
            for (int j = lane; j < n; j += WAVE) {
                const float s = sv[j];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += rp[q][j] * s;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = wave_sum(acc[q]);
        const float v = (lane == 0 ? acc[0] : (lane == 1 ? acc[1] : (lane == 2 ? acc[2] : acc[3]))) + bv;
        if (lane < 4 && i0 + lane < n) Y[((int64_t)b * n + i0 + lane) * ldy + c] = act == GT_ACT_RELU ? fmaxf(v, 0.f) : v;
    }
}

template <bool VEC>
__global__ __launch_bounds__(GC_THREADS) void gc_bwd_data_kernel(gt_edge_groups eg, const float* __restrict__ G, int64_t ldg,
                                                                 float* __restrict__ dS, int64_t ldds, int n) {
    extern __shared__ float gv[];                   // g[b, :, c], then the four partial rows [4][GC_COLS]
    float* red = gv + ((n + 3) & ~3);
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < n; i += GC_THREADS) gv[i] = G[((int64_t)b * n + i) * ldg + c];
    __syncthreads();
    const float* __restrict__ E = gc_slice(eg, b, c, n);
    const int j0 = blockIdx.x * GC_COLS;
    if (VEC) {
        const int j = j0 + lane * 4;                // n % 4 == 0: a lane's four columns are all inside or all outside
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (j < n) {
            const float* col = E + j;
            int i = wave;
            for (; i + 28 < n; i += 32) {           // rows i, i + 4, ..., i + 28: eight loads in flight
                f32x4 e[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = *reinterpret_cast<const f32x4*>(col + (int64_t)(i + 4 * u) * n);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += e[u] * gv[i + 4 * u];
            }
            for (; i < n; i += 4) acc += *reinterpret_cast<const f32x4*>(col + (int64_t)i * n) * gv[i];
        }
        *reinterpret_cast<f32x4*>(red + wave * GC_COLS + lane * 4) = acc;
    } else {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = wave; i < n; i += 4) {
            const float* row = E + (int64_t)i * n;
            const float g = gv[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + lane + WAVE * k;
                if (j < n) acc[k] += row[j] * g;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) red[wave * GC_COLS + lane + WAVE * k] = acc[k];
    }
    __syncthreads();
    const int j = j0 + tid;                         // one column per thread, the waves' partial sums in the order 0..3
    if (j < n)
        dS[((int64_t)b * n + j) * ldds + c] = ((red[tid] + red[GC_COLS + tid]) + red[2 * GC_COLS + tid]) + red[3 * GC_COLS + tid];
}

template <int P, bool VEC>
__global__ __launch_bounds__(GC_THREADS) void gc_bwd_edge_kernel(gt_edge_groups de, gt_graph_pairs pr, int64_t ldg, int64_t lds,
                                                                 int n, int tiles_j) {
    __shared__ float gl[GC_EDGE_ROWS][GC_MAXP];     // g_l[b, i0 + r, c] as [r][l]
    __shared__ float sl[GC_MAXP][GC_COLS];          // s_l[b, j0 + t, c]
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* __restrict__ dE = gc_slice(de, b, c, n);
    if (!dE) return;                                // this group needs no gradient (block-uniform)
    const int j0 = (blockIdx.x % tiles_j) * GC_COLS, i0 = (blockIdx.x / tiles_j) * GC_EDGE_ROWS;
    {
        const int j = j0 + tid, i = i0 + tid;
#pragma unroll
        for (int l = 0; l < P; ++l) {
            sl[l][tid] = j < n ? pr.s[l][((int64_t)b * n + j) * lds + c] : 0.f;
            if (tid < GC_EDGE_ROWS) gl[tid][l] = i < n ? pr.g[l][((int64_t)b * n + i) * ldg + c] : 0.f;
        }
    }
    __syncthreads();
    float sr[P][4];                                 // this lane's four columns of every s_l
#pragma unroll
    for (int l = 0; l < P; ++l)
#pragma unroll
        for (int k = 0; k < 4; ++k) sr[l][k] = sl[l][VEC ? lane * 4 + k : lane + WAVE * k];
    const int rows = min(GC_EDGE_ROWS, n - i0);
    for (int r = wave; r < rows; r += 4) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int l = 0; l < P; ++l) {
            const float g = gl[r][l];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] += g * sr[l][k];
        }
        float* row = dE + (int64_t)(i0 + r) * n + j0;
        if (VEC) {
            if (j0 + lane * 4 < n) *reinterpret_cast<f32x4*>(row + lane * 4) = f32x4{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + lane + WAVE * k < n) row[lane + WAVE * k] = o[k];
        }
    }
}

// ---- argument checks shared by the three entry points; 0, GT_EINVAL or GT_ENOTSUP, nothing launched on a refusal
static int gc_check(const gt_edge_groups& eg, bool need_all, int32_t B, int32_t n, int32_t C) {
    if (eg.n_groups < 1 || eg.n_groups > 3 || B <= 0 || n <= 0 || C <= 0) return GT_EINVAL;
    int64_t sum = 0;
    for (int g = 0; g < eg.n_groups; ++g) {
        if (eg.c[g] <= 0 || (need_all && !eg.e[g])) return GT_EINVAL;
        sum += eg.c[g];
    }
    if (sum != C) return GT_EINVAL;
    if (n > GT_GRAPHCONV_MAX_N || C > 65535 || B > 65535) return GT_ENOTSUP;
    return 0;
}
// groups past n_groups hold nothing the kernels may trust: clear them so that gc_slice's chain ends in the last real group
static gt_edge_groups gc_clean(gt_edge_groups eg) {
    for (int g = eg.n_groups; g < 3; ++g) { eg.e[g] = nullptr; eg.c[g] = 0; }
    return eg;
}
static bool gc_vec(const gt_edge_groups& eg, int n) {
    return (n & 3) == 0 && !misaligned16(eg.e[0], eg.e[1], eg.e[2]);
}

template <int P>
static void gc_edge_launch(bool vec, dim3 grid, hipStream_t st, const gt_edge_groups& de, const gt_graph_pairs& pr, int64_t ldg,
                           int64_t lds, int n, int tiles_j) {
    if (vec) hipLaunchKernelGGL((gc_bwd_edge_kernel<P, true>), grid, dim3(GC_THREADS), 0, st, de, pr, ldg, lds, n, tiles_j);
    else hipLaunchKernelGGL((gc_bwd_edge_kernel<P, false>), grid, dim3(GC_THREADS), 0, st, de, pr, ldg, lds, n, tiles_j);
}

}  // namespace gt

using namespace gt;

extern "C" int gt_graphconv_fwd(const gt_edge_groups* Ep, const float* S, int64_t lds, const float* bias, float* Y, int64_t ldy,
                                int32_t B, int32_t n, int32_t C, int32_t act, void* stream) {
    if (!Ep || !S || !Y || (act != GT_ACT_NONE && act != GT_ACT_RELU)) return GT_EINVAL;
    const gt_edge_groups E = *Ep;                   // (a host struct, read here: the kernels get it by value)
    if (int rc = gc_check(E, true, B, n, C)) return rc;
    if (lds < C || ldy < C) return GT_EINVAL;
    const gt_edge_groups eg = gc_clean(E);
    const dim3 grid(ceil_div(n, GC_FWD_ROWS), C, B);
    const size_t smem = (size_t)n * sizeof(float);
    if (gc_vec(eg, n))
        hipLaunchKernelGGL(gc_fwd_kernel<true>, grid, dim3(GC_THREADS), smem, (hipStream_t)stream, eg, S, lds, bias, Y, ldy, n, act);
    else
        hipLaunchKernelGGL(gc_fwd_kernel<false>, grid, dim3(GC_THREADS), smem, (hipStream_t)stream, eg, S, lds, bias, Y, ldy, n, act);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_graphconv_bwd_data(const gt_edge_groups* Ep, const float* G, int64_t ldg, float* dS, int64_t ldds, int32_t B,
                                     int32_t n, int32_t C, void* stream) {
    if (!Ep || !G || !dS) return GT_EINVAL;
    const gt_edge_groups E = *Ep;
    if (int rc = gc_check(E, true, B, n, C)) return rc;
    if (ldg < C || ldds < C) return GT_EINVAL;
    const gt_edge_groups eg = gc_clean(E);
    const dim3 grid(ceil_div(n, GC_COLS), C, B);
    const size_t smem = ((size_t)((n + 3) & ~3) + 4 * GC_COLS) * sizeof(float);
    if (gc_vec(eg, n))
        hipLaunchKernelGGL(gc_bwd_data_kernel<true>, grid, dim3(GC_THREADS), smem, (hipStream_t)stream, eg, G, ldg, dS, ldds, n);
    else
        hipLaunchKernelGGL(gc_bwd_data_kernel<false>, grid, dim3(GC_THREADS), smem, (hipStream_t)stream, eg, G, ldg, dS, ldds, n);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_graphconv_bwd_edge(const gt_edge_groups* dEp, const gt_graph_pairs* pp, int64_t ldg, int64_t lds, int32_t B, int32_t n,
                                     int32_t C, void* stream) {
    if (!dEp || !pp) return GT_EINVAL;
    const gt_edge_groups dE = *dEp;
    const gt_graph_pairs pairs = *pp;
    if (pairs.n_pairs < 1) return GT_EINVAL;
    if (pairs.n_pairs > GC_MAXP) return GT_ENOTSUP;
    if (int rc = gc_check(dE, false, B, n, C)) return rc;
    for (int l = 0; l < pairs.n_pairs; ++l)
        if (!pairs.g[l] || !pairs.s[l]) return GT_EINVAL;
    if (ldg < C || lds < C) return GT_EINVAL;
    const gt_edge_groups de = gc_clean(dE);
    if (!de.e[0] && !de.e[1] && !de.e[2]) return 0;          // no group wants a gradient
    const int tiles_j = ceil_div(n, GC_COLS);
    const dim3 grid(tiles_j * ceil_div(n, GC_EDGE_ROWS), C, B);
    const bool vec = gc_vec(de, n);
    const hipStream_t st = (hipStream_t)stream;
    switch (pairs.n_pairs) {
        case 1: gc_edge_launch<1>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        case 2: gc_edge_launch<2>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        case 3: gc_edge_launch<3>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        case 4: gc_edge_launch<4>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        case 5: gc_edge_launch<5>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        case 6: gc_edge_launch<6>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        case 7: gc_edge_launch<7>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
        default: gc_edge_launch<8>(vec, grid, st, de, pairs, ldg, lds, n, tiles_j); break;
    }
    GT_LAUNCH_CHECK();
    return 0;
}
