// Batched fp32 GEMM on the CDNA4 matrix pipe (v_mfma_f32_16x16x4_f32) with fused
// prologue (stateless dropout mask on A) and epilogue (bias, rank-p update, activation,
// aux-multiply, dropout, residual).  One kernel template serves every contraction of the
// encoder layer and the spectral decoder, forward and backward (see include/gt_hip.h).
//
// Tiling (gfx950): block = WM x WN waves of 64 lanes; each wave owns a (16*MT) x (16*NT)
// output tile as MT x NT MFMA 16x16 accumulators.  K is consumed in steps of 16 through a
// double-buffered LDS stage.  LDS images are k-major ([16][BM], [16][BN]) so that a lane's
// MT (NT) operands for one k are contiguous: one ds_read_b128 feeds 4 MFMAs.  Because the
// lane->row map of the MFMA is free, lane i takes rows {MT*i .. MT*i+MT-1}: the accumulator
// of a lane then holds NT consecutive output columns -> 16-byte global stores.
// An XOR swizzle on the column index (bits 3-4, keyed by k>>2) makes both the transposing
// ds_write_b32 of k-contiguous operands and the ds_read_b128 of the MFMA loop conflict-free.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "gt_gemm_core.h"

namespace gt {

// HEAD: instance with the fused two-layer-head epilogues instead of the general one (kept out of the
// general instances: its register footprint would cost them occupancy)
template <int LA, int LB, int MT, int NT, int WM, int WN, int BK, int HEAD = 0>
// (4 waves per SIMD requested for the 16-deep general instances: keeps the register allocation at <= 128)
__global__ __launch_bounds__(WM* WN * 64, ((HEAD == 0 && BK == 16) ? 4 : 1)) void gemm_kernel(const GemmP p) {
    constexpr int BM = WM * 16 * MT, BN = WN * 16 * NT, T = WM * WN * 64;
    constexpr int FA = BM * BK / 4, FB = BN * BK / 4;          // float4 per stage
    constexpr int NVA = (FA + T - 1) / T, NVB = (FB + T - 1) / T;
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * BM + 2 * BK * BN];
    float* sA = smem;
    float* sB = smem + 2 * BK * BM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 15, kq = lane >> 4;
    // XCD-aware tile order: blocks are dealt round-robin to the 8 XCDs (block b -> XCD b % 8), so give each
    // XCD a contiguous range of tile ids -- the N-tiles that share an A row panel then hit the same L2
    // instead of fetching the panel once per XCD (bijective for any tile count; speed only).
    int tile;
    {
        const int tiles = gridDim.x, q = tiles >> 3, r = tiles & 7;
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int z = blockIdx.z, b0 = z / p.batch1, b1 = z % p.batch1;
    const int kbeg = blockIdx.y * p.k_chunk;
    const int kend = min(p.K, kbeg + p.k_chunk);

    // operands of the K segment being loaded (uniform values; switched once when a second product follows)
    const float* A = p.A + b0 * p.a_bs0 + b1 * p.a_bs1;
    const float* Bm = p.B + b0 * p.b_bs0 + b1 * p.b_bs1;
    int64_t lda_c = p.lda, ldb_c = p.ldb;
    int kend_c = min(p.K, (int)blockIdx.y * p.k_chunk + p.k_chunk), avec_c = p.a_vec, bvec_c = p.b_vec;
    const uint32_t akey = drop_key_dev(p.a_drop);
    const int64_t adoff = (int64_t)z * p.a_drop_bstride;
    const DropDev nodrop{0u, 0u, 1.f, nullptr};

    f32x4 acc[MT][NT];
#pragma unroll
    for (int s = 0; s < MT; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 ra[NVA], rb[NVB];
    // LA == 1: a thread's float4 always covers the same 4 rows m of the tile (T is a multiple of BM/4),
    // so the row sums of A (= bias gradients in the weight-gradient use) accumulate in registers for free
    f32x4 asum = {0.f, 0.f, 0.f, 0.f};
    const bool do_acs = (LA == 1) && p.acs != nullptr && tn == 0;
    auto g2r = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const int idx = tid + i * T;
            if (FA % T == 0 || idx < FA) {
                ra[i] = gload<LA, BM, BK>(A, lda_c, m0, p.M, k0, kend_c, idx, avec_c, p.a_drop, akey,
                                          p.a_drop_ld, adoff);
                if (LA == 1 && do_acs) asum += ra[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int idx = tid + i * T;
            if (FB % T == 0 || idx < FB)
                rb[i] = gload<LB, BN, BK>(Bm, ldb_c, n0, p.N, k0, kend_c, idx, bvec_c, nodrop, 0u, 0, 0);
        }
    };
    auto r2s = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const int idx = tid + i * T;
            if (FA % T == 0 || idx < FA) sstore<LA, BM, BK>(sA + buf * BK * BM, idx, ra[i]);
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int idx = tid + i * T;
            if (FB % T == 0 || idx < FB) sstore<LB, BN, BK>(sB + buf * BK * BN, idx, rb[i]);
        }
    };

    const int nk1 = (kend > kbeg) ? (kend - kbeg + BK - 1) / BK : 0;
    const int nk = nk1 + (p.K2 > 0 ? (p.K2 + BK - 1) / BK : 0);
    auto enter_seg2 = [&]() {
        A = p.A2 + b0 * p.a2_bs0 + b1 * p.a2_bs1;
        Bm = p.B2 + b0 * p.b2_bs0 + b1 * p.b2_bs1;
        lda_c = p.lda2; ldb_c = p.ldb2; kend_c = p.K2; avec_c = p.a2_vec; bvec_c = p.b2_vec;
    };
    if (nk > 0) {
        if (nk1 == 0) { enter_seg2(); g2r(0); }
        else g2r(kbeg);
        r2s(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) {
            if (kt + 1 == nk1) enter_seg2();
            g2r(kt + 1 < nk1 ? kbeg + (kt + 1) * BK : (kt + 1 - nk1) * BK);
        }
        const float* __restrict__ cA = sA + buf * BK * BM;
        const float* __restrict__ cB = sB + buf * BK * BN;
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            const int k = 4 * ks + kq;
            const int swa = ((ks & 3) << 3) & (BM - 1), swb = ((ks & 3) << 3) & (BN - 1);
            float a[MT], b[NT];
            lds_frag<MT>(cA + k * BM + ((wm * 16 * MT + MT * li) ^ swa), a);
            lds_frag<NT>(cB + k * BN + ((wn * 16 * NT + NT * li) ^ swb), b);
#pragma unroll
            for (int s = 0; s < MT; ++s)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[s][t] = mfma16(a[s], b[t], acc[s][t]);
        }
        if (kt + 1 < nk) r2s(buf ^ 1);
        __syncthreads();
    }

    if (LA == 1 && do_acs) {        // uniform per block; smem is free after the loop's last barrier
        constexpr int Q = BM / 4, ROWS = T / Q;
        static_assert(T % Q == 0 && ROWS * BM <= 2 * BK * BM, "row-sum scratch must fit the A stage");
        *reinterpret_cast<f32x4*>(&smem[(tid / Q) * BM + 4 * (tid % Q)]) = asum;
        __syncthreads();
        if (tid < BM && m0 + tid < p.M) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) t += smem[r * BM + tid];
            p.acs[((int64_t)blockIdx.y * gridDim.z + z) * p.M + m0 + tid] = t;
        }
    }

    if (HEAD > 0) {
        head_epilogue<MT, NT, WM, WN, (HEAD > 0 ? HEAD : 1)>(p, acc, smem, m0, wm, wn, li, kq, tm);
        return;
    }
    // ------------------------------- epilogue -------------------------------------------------
    gemm_epilogue<MT, NT>(p, acc, m0 + wm * 16 * MT, n0 + wn * 16 * NT + NT * li, z, b0, b1,
                                      (int)blockIdx.y, kq);
}

// =================================================================================================
// Streamed kernel (aligned operands, 128-wide N tiles): persistent blocks, direct global->LDS loads.
//
// The v1 kernel above runs every tile as load -> MFMA -> store with all co-resident blocks in the same
// phase, so HBM and the matrix pipe take turns.  Here a block walks a list of (tile, K-slice) items as ONE
// stream of 32-deep K stages: stage g+1 is requested with `global_load_lds_dwordx4` (no VGPR staging, no
// ds_write pass) right after the barrier that publishes stage g, and the stream does not stop at a tile
// boundary -- the first stage of the next tile is in flight while the current tile's last MFMAs and its
// epilogue run, and the epilogue's stores drain under the next tile's MFMAs.
//
// LDS images (per stage, A then B), chosen so that a direct load (wave-uniform base + lane*16 B) lands
// conflict-free for the MFMA fragment reads:
//   k-contiguous operand (L==0):  [rows][32]  with the 16-byte granule g of row r stored at slot
//                                 g ^ ((r>>2)&7)           -> lane reads one float per (row, k)
//   x-contiguous operand (L==1):  [32][BX]    with column granules XOR-ed by ((k>>2)&3)<<1 (same image
//                                 as v1)                   -> lane reads MT/NT consecutive floats
// The swizzles are applied on the SOURCE address (the LDS side of a direct load is linear).
// Out-of-range rows / K-tail granules read a 16-byte device zero instead.
__device__ __attribute__((aligned(16))) float gt_zero16[4] = {0.f, 0.f, 0.f, 0.f};

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

struct SItem {
    int m0, n0, z, b0, b1, sidx, kbeg, kend, nk;
    const float* A;
    const float* B;
    int64_t adoff;
};

// second launch-bound argument = waves per SIMD the register allocation must leave room for: the LDS
// footprint admits 2 (128-row tiles) or 3 (64-row tiles) blocks per CU
template <int LA, int LB, int MT>
__global__ __launch_bounds__(256, (MT == 4 ? 2 : 3)) void gemm_stream_kernel(const GemmP p) {
    constexpr int NT = 4, WN = 2, BK = 32, T = 256;
    constexpr int BM = 32 * MT, BN = 128;
    constexpr int SA = BM * BK, SB = BN * BK, STAGE = SA + SB;
    constexpr int NIA = BM / 32, NIB = BN / 32;               // 1-KiB load instructions per wave per stage
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 15, kq = lane >> 4;
    const uint32_t akey = drop_key_dev(p.a_drop);

    const int per_xcd = (p.n_work + 7) >> 3;
    const int xcd = blockIdx.x & 7, slots = gridDim.x >> 3;
    int jpos = blockIdx.x >> 3;

    auto decode = [&](int j, SItem& it) -> bool {
        const int w = xcd * per_xcd + j;
        if (j >= per_xcd || w >= p.n_work) return false;
        const int tiles = p.tiles_m * p.tiles_n;
        const int t = w % tiles, r = w / tiles;
        it.sidx = r % p.n_split;
        it.z = r / p.n_split;
        it.m0 = (t / p.tiles_n) * BM;
        it.n0 = (t % p.tiles_n) * BN;
        it.b0 = it.z / p.batch1;
        it.b1 = it.z % p.batch1;
        it.kbeg = it.sidx * p.k_chunk;
        it.kend = min(p.K, it.kbeg + p.k_chunk);
        it.nk = (it.kend - it.kbeg + BK - 1) / BK;
        it.A = p.A + it.b0 * p.a_bs0 + it.b1 * p.a_bs1;
        it.B = p.B + it.b0 * p.b_bs0 + it.b1 * p.b_bs1;
        it.adoff = (int64_t)it.z * p.a_drop_bstride;
        return true;
    };

    // request one 32-deep stage (A and B tiles of item `it` at k0) into buffer `buf`
    auto issue = [&](const SItem& it, int k0, int buf) {
        float* sa = smem + buf * STAGE;
        float* sb = sa + SA;
#pragma unroll
        for (int i = 0; i < NIA; ++i) {
            const int q = wave * NIA + i;                      // 1-KiB chunk of the A image
            const float* src;
            if (LA == 0) {
                const int row = 8 * q + (lane >> 3), slot = lane & 7;
                const int g = slot ^ ((row >> 2) & 7);
                const int m = it.m0 + row, k = k0 + 4 * g;
                src = (m < p.M && k < it.kend) ? it.A + (int64_t)m * p.lda + k : gt_zero16;
            } else {
                constexpr int GPR = BM / 4;                    // granules per k-row
                const int e = q * 64 + lane, kr = e / GPR, pc = e % GPR;
                const int g = pc ^ ((((kr >> 2) & 3) << 1) & (GPR - 1));
                const int k = k0 + kr, m = it.m0 + 4 * g;
                src = (k < it.kend && m < p.M) ? it.A + (int64_t)k * p.lda + m : gt_zero16;
            }
            __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(sa + q * 256), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NIB; ++i) {
            const int q = wave * NIB + i;
            const float* src;
            if (LB == 0) {
                const int row = 8 * q + (lane >> 3), slot = lane & 7;
                const int g = slot ^ ((row >> 2) & 7);
                const int n = it.n0 + row, k = k0 + 4 * g;
                src = (n < p.N && k < it.kend) ? it.B + (int64_t)n * p.ldb + k : gt_zero16;
            } else {
                constexpr int GPR = BN / 4;
                const int e = q * 64 + lane, kr = e / GPR, pc = e % GPR;
                const int g = pc ^ ((((kr >> 2) & 3) << 1) & (GPR - 1));
                const int k = k0 + kr, n = it.n0 + 4 * g;
                src = (k < it.kend && n < p.N) ? it.B + (int64_t)k * p.ldb + n : gt_zero16;
            }
            __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(sb + q * 256), 16, 0, 0);
        }
    };

    SItem cur, nxt;
    bool light_wait = false;
    bool have = decode(jpos, cur);
    int g = 0;                                                 // running stage counter -> LDS buffer g&1
    if (have) issue(cur, cur.kbeg, 0);

    while (have) {
        jpos += slots;
        const bool have_next = decode(jpos, nxt);
        f32x4 acc[MT][NT];
#pragma unroll
        for (int s = 0; s < MT; ++s)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float asum[MT];
#pragma unroll
        for (int s = 0; s < MT; ++s) asum[s] = 0.f;
        const bool do_acs = (LA == 1) && p.acs != nullptr && cur.n0 == 0 && wn == 0;

        for (int kt = 0; kt < cur.nk; ++kt, ++g) {
            // stage g has landed for this wave (vmcnt) and for everybody (barrier); everybody is also done
            // reading the other buffer, which the next request overwrites.
            // Right after the epilogue of a FULL tile this wave has issued >= 4*MT output stores AFTER the
            // stage-g request; VMEM operations retire in order on gfx9-class counters, so "at most 4*MT
            // outstanding" already implies the (older) stage loads have landed -- the stores may drain under
            // the next MFMAs instead of stalling the first stage of every tile.
            if (light_wait) {
                if (MT == 4) asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
                light_wait = false;
            } else {
                asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            }
            if (kt + 1 < cur.nk) issue(cur, cur.kbeg + (kt + 1) * BK, (g + 1) & 1);
            else if (have_next) issue(nxt, nxt.kbeg, (g + 1) & 1);
            const float* __restrict__ cA = smem + (g & 1) * STAGE;
            const float* __restrict__ cB = cA + SA;
            const int kbase = cur.kbeg + kt * BK;
#pragma unroll
            for (int ks = 0; ks < BK / 4; ++ks) {
                const int k = 4 * ks + kq;
                float a[MT], b[NT];
                if (LA == 0) {
#pragma unroll
                    for (int s = 0; s < MT; ++s) {
                        const int row = wm * 16 * MT + MT * li + s;
                        a[s] = cA[row * 32 + 4 * (ks ^ ((row >> 2) & 7)) + kq];
                    }
                } else {
                    lds_frag<MT>(cA + k * BM + ((wm * 16 * MT + MT * li) ^ (((ks & 3) << 3) & (BM - 1))), a);
                }
                if (LB == 0) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int row = wn * 16 * NT + NT * li + t;
                        b[t] = cB[row * 32 + 4 * (ks ^ ((row >> 2) & 7)) + kq];
                    }
                } else {
                    lds_frag<NT>(cB + k * BN + ((wn * 16 * NT + NT * li) ^ (((ks & 3) << 3) & (BN - 1))), b);
                }
                if (p.a_drop.thresh) {                          // dropout mask on A, regenerated from its index
#pragma unroll
                    for (int s = 0; s < MT; ++s) {
                        const int m = cur.m0 + wm * 16 * MT + MT * li + s, kk = kbase + k;
                        const int64_t di = cur.adoff + (LA == 0 ? (int64_t)m * p.a_drop_ld + kk
                                                                : (int64_t)kk * p.a_drop_ld + m);
                        a[s] *= drop_mul(p.a_drop, akey, (uint32_t)di);
                    }
                }
                if (LA == 1 && do_acs) {
#pragma unroll
                    for (int s = 0; s < MT; ++s) asum[s] += a[s];
                }
#pragma unroll
                for (int s = 0; s < MT; ++s)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[s][t] = mfma16(a[s], b[t], acc[s][t]);
            }
        }

        if (LA == 1 && do_acs) {        // row sums of A: combine the 4 k-lanes; lanes kq == 0 hold MT rows each
#pragma unroll
            for (int s = 0; s < MT; ++s) {
                float v = asum[s];
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                const int m = cur.m0 + wm * 16 * MT + MT * li + s;
                if (kq == 0 && m < p.M)
                    p.acs[((int64_t)cur.sidx * p.n_batch + cur.z) * p.M + m] = v;
            }
        }
        gemm_epilogue<MT, NT>(p, acc, cur.m0 + wm * 16 * MT, cur.n0 + wn * 16 * NT + NT * li, cur.z, cur.b0, cur.b1,
                              cur.sidx, kq);
        // every row and column of this wave's sub-tile was in range => exactly 4*MT (or more, with `pre`)
        // store instructions were issued by the epilogue
        light_wait = p.light_wait && (cur.m0 + BM <= p.M) && (cur.n0 + BN <= p.N) && cur.nk > 0;
        cur = nxt;
        have = have_next;
    }
}

// out_z[m][n..n+3] = alpha * sum_s slab[s][z][m][n..n+3]   (N % 4 == 0, 16-byte aligned everything)
// Block = 32 consecutive float4 outputs x 8 slab lanes; slab lane j sums slabs j, j+8, ... in order,
// then the 8 partials are combined in a fixed order through LDS (deterministic).
__global__ __launch_bounds__(256) void splitk_reduce4_kernel(const float* __restrict__ slabs, int nsplit,
                                                             int64_t slab_stride, int M, int N4, int batch1,
                                                             float alpha, float* __restrict__ C, int64_t ldc,
                                                             int64_t c_bs0, int64_t c_bs1, int64_t total4) {
    __shared__ f32x4 part[8][32];
    const int ox = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int64_t i = (int64_t)blockIdx.x * 32 + ox;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < total4) {
        const f32x4* src = reinterpret_cast<const f32x4*>(slabs) + i;
        const int64_t st4 = slab_stride / 4;
#pragma unroll 4
        for (int k = sl; k < nsplit; k += 8) s += src[k * st4];
    }
    part[sl][ox] = s;
    __syncthreads();
    if (sl == 0 && i < total4) {
#pragma unroll
        for (int k = 1; k < 8; ++k) s += part[k][ox];
        const int n4 = (int)(i % N4);
        const int64_t r = i / N4;
        const int m = (int)(r % M);
        const int z = (int)(r / M);
        *reinterpret_cast<f32x4*>(C + (z / batch1) * c_bs0 + (z % batch1) * c_bs1 + (int64_t)m * ldc + 4 * n4) =
            alpha * s;
    }
}

// out_z[m][n] = alpha * sum_s slab[s][z][m][n]
__global__ void splitk_reduce_kernel(const float* __restrict__ slabs, int nsplit, int64_t slab_stride,
                                     int M, int N, int batch1, float alpha, float* __restrict__ C,
                                     int64_t ldc, int64_t c_bs0, int64_t c_bs1, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < nsplit; ++k) s += slabs[k * slab_stride + i];
        const int n = (int)(i % N);
        const int64_t r = i / N;
        const int m = (int)(r % M);
        const int z = (int)(r / M);
        C[(z / batch1) * c_bs0 + (z % batch1) * c_bs1 + (int64_t)m * ldc + n] = alpha * s;
    }
}

// ---- launchers: f32_launch switches on the pick the descriptor layer (gt_gemm_desc.hip) made, f32_kernel_name prints it --------
template <int LA, int LB, int BK, int HEAD>
static void launch_cfg(int cfg, dim3 grid, hipStream_t st, const GemmP& p) {
    switch (cfg) {
        case 0: hipLaunchKernelGGL((gemm_kernel<LA, LB, 4, 4, 2, 2, BK, HEAD>), grid, dim3(256), 0, st, p); break;
        case 1: hipLaunchKernelGGL((gemm_kernel<LA, LB, 2, 4, 2, 2, BK, HEAD>), grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL((gemm_kernel<LA, LB, 2, 2, 2, 2, BK, HEAD>), grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL((gemm_kernel<LA, LB, 2, 2, 4, 1, BK, HEAD>), grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL((gemm_kernel<LA, LB, 2, 1, 4, 1, BK, HEAD>), grid, dim3(256), 0, st, p); break;
    }
}

static int num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;      // MI355X
        n = v;
    }
    return n;
}

// Persistent launch: the grid never exceeds what is resident at once (a block runs until its share of the
// work list is empty, so a block waiting for a slot would serialise behind the others).
template <int LA, int LB, int MT>
static void launch_stream(hipStream_t st, const GemmP& p) {
    static const int per_cu = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gemm_stream_kernel<LA, LB, MT>, 256, 0) != hipSuccess ||
            n < 1)
            n = 1;
        return std::min(n, 4);
    }();
    int nblk = std::min(p.n_work, num_cus() * per_cu);
    if (const char* e = getenv("GT_GEMM_BLOCKS")) nblk = std::min(p.n_work, std::max(1, atoi(e)));
    nblk = ((nblk + 7) / 8) * 8;
    hipLaunchKernelGGL((gemm_stream_kernel<LA, LB, MT>), dim3(nblk), dim3(256), 0, st, p);
}

// f(LA, LB) with the two layouts as compile-time constants
template <class F>
static void with_layouts(int la, int lb, F&& f) {
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    if (la == 0 && lb == 0) f(I0{}, I0{});
    else if (la == 0) f(I0{}, I1{});
    else if (lb == 0) f(I1{}, I0{});
    else f(I1{}, I1{});
}

int f32_launch(const GemmP& p, const F32Pick& k, dim3 grid, hipStream_t st) {
    if (k.family == F32_HEAD) {     // fused two-layer head: activations [tokens, K] times nn.Linear weight [N, K] only
        if (k.LA || k.LB) return GT_ENOTSUP;
        if (k.n_out == 1) launch_cfg<0, 0, 16, 1>(k.cfg, grid, st, p);
        else launch_cfg<0, 0, 16, 4>(k.cfg, grid, st, p);
    } else {
        with_layouts(k.LA, k.LB, [&](auto la, auto lb) {
            constexpr int LA = decltype(la)::value, LB = decltype(lb)::value;
            if (k.family == F32_STREAM && k.cfg == 0) launch_stream<LA, LB, 4>(st, p);
            else if (k.family == F32_STREAM) launch_stream<LA, LB, 2>(st, p);
            else if (k.BK == 32) launch_cfg<LA, LB, 32, 0>(k.cfg, grid, st, p);
            else launch_cfg<LA, LB, 16, 0>(k.cfg, grid, st, p);
        });
    }
    GT_LAUNCH_CHECK();
    return 0;
}

const char* f32_kernel_name(const F32Pick& k) {
    static thread_local char buf[112];
    const F32Cfg& c = kF32Cfgs[k.cfg];
    if (k.family == F32_STREAM)
        snprintf(buf, sizeof(buf), "void gt::gemm_stream_kernel<%d, %d, %d>(gt::GemmP)", k.LA, k.LB, c.mt);
    else
        snprintf(buf, sizeof(buf), "void gt::gemm_kernel<%d, %d, %d, %d, %d, %d, %d, %d>(gt::GemmP)", k.LA, k.LB, c.mt, c.nt, c.wm,
                 c.wn, k.BK, k.family == F32_HEAD ? (k.n_out == 1 ? 1 : 4) : 0);
    return buf;
}

// C_z = alpha * sum over the `split` slabs [split][batch0 * batch1][M][N] in ws (what a raw split-K launch of any engine left)
int splitk_reduce_launch(const float* slabs, int split, int M, int N, int batch0, int batch1, float alpha, float* C, int64_t ldc,
                         int64_t c_bs0, int64_t c_bs1, hipStream_t st) {
    const int64_t mn = (int64_t)M * N, total = (int64_t)batch0 * batch1 * mn;
    if (((N | ldc | c_bs0 | c_bs1) & 3) == 0 && !misaligned16(C, slabs)) {
        const int64_t total4 = total / 4;
        const int blocks4 = (int)((total4 + 31) / 32);
        hipLaunchKernelGGL(splitk_reduce4_kernel, dim3(blocks4), dim3(256), 0, st, slabs, split, total, M, N / 4, batch1, alpha, C,
                           ldc, c_bs0, c_bs1, total4);
    } else {
        const int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, slabs, split, total, M, N, batch1, alpha, C, ldc,
                           c_bs0, c_bs1, total);
    }
    GT_LAUNCH_CHECK();
    return 0;
}

}  // namespace gt
