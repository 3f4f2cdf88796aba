// Split-operand GEMM (gt_x3_core.h): the LDS-staged, ring and bf16x3 packed-B kernels, and the host dispatch of every family.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "gt_x3_core.h"

namespace gt {

template <int LA, int LB, int PLANES>
__global__ __launch_bounds__(256, 2) void gemm_x3_kernel(const GemmP p) {
    constexpr int STAGE = 2 * PLANES * X3_PLANE;                          // A planes then B planes
    constexpr int SMEM = (2 * STAGE > 4 * X3_EP_STG * 4) ? 2 * STAGE : 4 * X3_EP_STG * 4;   // stages, later staging tiles
    __shared__ __attribute__((aligned(16))) char smem[SMEM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;
    // XCD-aware tile order (same map as gemm_kernel): each XCD walks a contiguous range of tile ids
    int tile;
    {
        const int tiles = gridDim.x, q = tiles >> 3, r = tiles & 7;
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
    const int m0 = tm * X3_BM, n0 = tn * X3_BN;
    const int z = blockIdx.z, b0 = z / p.batch1, b1 = z % p.batch1;
    const int kbeg = blockIdx.y * p.k_chunk;
    const int kend = min(p.K, kbeg + p.k_chunk);

    const float* A = p.A + b0 * p.a_bs0 + b1 * p.a_bs1;
    const float* Bm = p.B + b0 * p.b_bs0 + b1 * p.b_bs1;
    int64_t lda_c = p.lda, ldb_c = p.ldb;
    int kend_c = kend, avec_c = p.a_vec, bvec_c = p.b_vec;
    const uint32_t akey = drop_key_dev(p.a_drop);
    const int64_t adoff = (int64_t)z * p.a_drop_bstride;

    // staging role of this thread: one row of each operand tile, one k-half (8 consecutive k) per stage
    const int arow = (LA == 0) ? (tid >> 1) : (tid & 127), akh = (LA == 0) ? (tid & 1) : (tid >> 7);
    const int brow = (LB == 0) ? (tid >> 1) : (tid & 127), bkh = (LB == 0) ? (tid & 1) : (tid >> 7);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float ra[8], rb[8];
    float asum = 0.f;
    int ka = 0;                                   // first k of the values held in ra (for the mask index)
    const bool do_acs = (LA == 1) && p.acs != nullptr && tn == 0;
    // FAST: every element of the stage is in range along k and k-contiguous rows are 16-byte aligned -- straight-line
    // loads (row validity by pointer select), so the only vmcnt wait of an iteration sits in r2s, after the MFMAs.
    auto g2r = [&](int k0, auto fast) {
        constexpr bool FAST = decltype(fast)::value;
        const bool inside = FAST || (k0 + X3_BK <= kend_c);       // block-uniform
        ka = k0 + 8 * akh;
        x3_load8<LA>(A, lda_c, m0 + arow, p.M, ka, kend_c, inside && (FAST || LA == 1 || avec_c), ra);
        x3_load8<LB>(Bm, ldb_c, n0 + brow, p.N, k0 + 8 * bkh, kend_c, inside && (FAST || LB == 1 || bvec_c), rb);
    };
    auto r2s = [&](int buf) {                     // first use of the loaded registers: the vmcnt wait lands here
        if (p.a_drop.thresh) x3_mask8<LA>(p.a_drop, akey, p.a_drop_ld, adoff, m0 + arow, ka, ra);
        if (LA == 1 && do_acs) asum += ((ra[0] + ra[1]) + (ra[2] + ra[3])) + ((ra[4] + ra[5]) + (ra[6] + ra[7]));
        {                                         // odd operand rows enter negated (tile origins are even)
            const float sa_ = x3_alt_sign(arow), sb_ = x3_alt_sign(brow);
#pragma unroll
            for (int j = 0; j < 8; ++j) { ra[j] *= sa_; rb[j] *= sb_; }
        }
        char* st = smem + buf * STAGE;
        x3_store8<PLANES>(st, arow, akh, ra);
        x3_store8<PLANES>(st + PLANES * X3_PLANE, brow, bkh, rb);
    };
    auto compute = [&](int buf) {
        const char* sa = smem + buf * STAGE;
        const char* sb = sa + PLANES * X3_PLANE;
        bf16x8 am[2][PLANES], bn[2][PLANES];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                am[i][pl] = *reinterpret_cast<const bf16x8*>(sa + pl * X3_PLANE + (wm * 64 + 32 * i + lr) * X3_PITCH + lh * 16);
                bn[i][pl] = *reinterpret_cast<const bf16x8*>(sb + pl * X3_PLANE + (wn * 64 + 32 * i + lr) * X3_PITCH + lh * 16);
            }
        // plane pairs in increasing magnitude; the four accumulators interleave inside every pair
#pragma unroll
        for (int s = PLANES - 1; s >= 0; --s) {          // plane pairs (pa, pb) with pa + pb = s <= PLANES - 1
#pragma unroll
            for (int pa = 0; pa < PLANES; ++pa) {
                const int pb = s - pa;
                if (pb < 0 || pb >= PLANES) continue;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bn[j][pb], am[i][pa], acc[i][j]);
            }
        }
    };

    const int nk1 = (kend > kbeg) ? (kend - kbeg + X3_BK - 1) / X3_BK : 0;
    const int nk = nk1 + (p.K2 > 0 ? (p.K2 + X3_BK - 1) / X3_BK : 0);
    auto enter_seg2 = [&]() {
        A = p.A2 + b0 * p.a2_bs0 + b1 * p.a2_bs1;
        Bm = p.B2 + b0 * p.b2_bs0 + b1 * p.b2_bs1;
        lda_c = p.lda2; ldb_c = p.ldb2; kend_c = p.K2; avec_c = p.a2_vec; bvec_c = p.b2_vec;
    };
    if (nk > 0) {
        if (nk1 == 0) { enter_seg2(); g2r(0, std::false_type{}); }
        else g2r(kbeg, std::false_type{});
        r2s(0);
    }
    __syncthreads();
    // iterations whose NEXT stage is a whole one of the first product take the branch-free loop
    const bool fast_ok = (LA == 1 || p.a_vec) && (LB == 1 || p.b_vec);
    const int nfast = fast_ok ? max(0, (kend - kbeg) / X3_BK - 1) : 0;
    int kt = 0;
    for (; kt < nfast; ++kt) {
        g2r(kbeg + (kt + 1) * X3_BK, std::true_type{});
        compute(kt & 1);
        r2s((kt + 1) & 1);
        __syncthreads();
    }
    for (; kt + 1 < nk; ++kt) {                   // K tail, unaligned operands, the second product
        if (kt + 1 == nk1) enter_seg2();
        g2r(kt + 1 < nk1 ? kbeg + (kt + 1) * X3_BK : (kt + 1 - nk1) * X3_BK, std::false_type{});
        compute(kt & 1);
        r2s((kt + 1) & 1);
        __syncthreads();
    }
    if (nk > 0) compute((nk - 1) & 1);
    __syncthreads();

    if (LA == 1 && do_acs) {              // uniform per block; the stages are free after the loop's last barrier
        float* part = reinterpret_cast<float*>(smem);
        part[akh * X3_BM + arow] = asum;
        __syncthreads();
        if (tid < X3_BM && m0 + tid < p.M)
            p.acs[((int64_t)blockIdx.y * gridDim.z + z) * p.M + m0 + tid] = part[tid] + part[X3_BM + tid];
    }

    __syncthreads();                               // every wave is done with the stages: they become staging tiles
    x3_alt_undo(acc, x3_alt_sign(lr));
    x3_epilogue<2>(p, acc, m0 + wm * 64, n0 + wn * 64, lane, reinterpret_cast<float*>(smem) + wave * X3_EP_STG, z, b0, b1,
                   (int)blockIdx.y);
}

// =================================================================================================================
// Ring variant for aligned operands: the fp32 tiles go global -> LDS by direct loads (no VGPR staging, no ds_write
// pass) into a ring of R 16-deep stages, R - 1 stages in flight while one is consumed, so an HBM round trip is covered
// by ~R - 1 stage times instead of one; the exact bf16 split happens in registers on the way from LDS into the MFMA
// operands (each wave converts the two A and two B row tiles it multiplies).  One s_barrier per stage publishes the
// landed stage and frees the slot the next request overwrites.
//
// (stage images: gt_x3_core.h)
// Needs: 16-byte aligned operands and leading dimensions, K % 4 == 0 for k-contiguous operands, X % 4 == 0 for
// x-contiguous ones, no second product (the register-staged kernel above takes everything else).

// HN = head width of the fused head-norm epilogue (0 = general epilogue)
// CV = 0 plain GEMM, 1 implicit 3x3 convolution on A (forward / data gradient), 2 on B, one tap per block (weight gradient)
template <int LA, int LB, int PLANES, int R, int HN = 0, int CV = 0>
__global__ __launch_bounds__(256, (R <= 3 ? 3 : 2)) void gemm_x3r_kernel(const GemmP p) {
    __shared__ __attribute__((aligned(16))) char smem[R * X3R_STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;
    int tile, by, z;
    if (CV == 2) {
        // 1-D grid: the nine taps of one (K chunk, tile) sit next to each other on ONE XCD, so the dY and X rows they
        // share come out of that XCD's L2 instead of HBM nine times
        const int tiles = p.tiles_m * p.tiles_n;
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        const int ct = (j / 9) * 8 + xcd;
        if (ct >= p.n_split * tiles) return;
        z = j % 9; by = ct / tiles; tile = ct % tiles;
    } else {
        const int tiles = gridDim.x, q = tiles >> 3, r = tiles & 7;
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
        by = blockIdx.y; z = blockIdx.z;
    }
    const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
    const int m0 = tm * X3_BM, n0 = tn * X3_BN;
    const int b0 = z / p.batch1, b1 = z % p.batch1;
    const int kbeg = by * p.k_chunk;
    const int kend = min(p.K, kbeg + p.k_chunk);
    const float* A = p.A + b0 * p.a_bs0 + b1 * p.a_bs1;
    const float* Bm = p.B + b0 * p.b_bs0 + b1 * p.b_bs1;
    const uint32_t akey = drop_key_dev(p.a_drop);
    const int64_t adoff = (int64_t)z * p.a_drop_bstride;
    const bool do_acs = (LA == 1) && p.acs != nullptr && tn == 0 && wn == 0 && CV != 2;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float asum[2] = {0.f, 0.f};
    const float rsgn = x3_alt_sign(lr);

    const int nk = (kend > kbeg) ? (kend - kbeg + X3_BK - 1) / X3_BK : 0;
    // convolution: this lane's two pixels of the A image (fixed over the stages), and the running (tap, channel) of
    // the next stage to request (stages are requested in order)
    const float* cv_row[2] = {A, A};
    int cv_ok[2] = {0, 0}, cv_tap = 0, cv_c0 = 0;
    const int cv_cb = (p.cv_C & 31) ? 16 : 32;
    int cw_y[2] = {0, 0}, cw_x[2] = {0, 0};        // CV == 2: (y, x) of this lane's two k-rows (pixels) of the next stage
    if (CV == 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pix = (kbeg + 2 * (wave * 2 + i) + (lane >> 5)) % (p.cv_H * p.cv_W);
            cw_y[i] = pix / p.cv_W;
            cw_x[i] = pix - cw_y[i] * p.cv_W;
        }
    }
    if (CV == 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + 16 * (wave * 2 + i) + (lane >> 2);
            if (m < p.M) {
                const int pix = m % (p.cv_H * p.cv_W), y = pix / p.cv_W, x = pix - y * p.cv_W;
                int ok = 0;
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    ok |= (((unsigned)(y + t / 3 - 1) < (unsigned)p.cv_H) && ((unsigned)(x + t % 3 - 1) < (unsigned)p.cv_W)) << t;
                cv_ok[i] = ok;
                cv_row[i] = A + (int64_t)m * p.lda;
            }
        }
    }
    auto issue = [&](int s) {                      // stage s -> slot s % R : 4 load instructions per wave
        char* st = smem + (s % R) * X3R_STAGE;
        const int k0 = kbeg + s * X3_BK;
        if (CV == 1) {
            x3r_issue_conv(cv_row, cv_ok, cv_tap, cv_c0, p.cv_W, p.lda, st, wave, lane);
            cv_c0 += X3_BK;                        // channel block first, taps second, channel blocks last (gt_hip.h)
            if ((cv_c0 & (cv_cb - 1)) == 0) {
                cv_c0 -= cv_cb;
                if (++cv_tap == 9) { cv_tap = 0; cv_c0 += cv_cb; }
            }
        } else {
            x3r_issue<LA>(A, p.lda, m0, p.M, k0, kend, st, wave, lane);
        }
        if (CV == 2) {
            x3r_issue_convw(p.B, p.ldb, n0, p.N, k0, kend, cw_y, cw_x, z / 3 - 1, z % 3 - 1, p.cv_H, p.cv_W,
                            st + X3R_OP, wave, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i) {          // the next stage's pixels: 16 further along the row-major image
                cw_x[i] += X3_BK;
                if (cw_x[i] >= p.cv_W) {
                    cw_x[i] -= p.cv_W;
                    if (++cw_y[i] == p.cv_H) cw_y[i] = 0;
                }
            }
        } else {
            x3r_issue<LB>(Bm, p.ldb, n0, p.N, k0, kend, st + X3R_OP, wave, lane);
        }
    };
#pragma unroll
    for (int s = 0; s < R - 1; ++s)
        if (s < nk) issue(s);

    for (int kt = 0; kt < nk; ++kt) {
        // stages kt+1 .. min(nk-1, kt+R-2) were requested after stage kt: VMEM retires in order, so "at most
        // 4 * newer loads outstanding" means stage kt has landed for this wave; the barrier extends that to the block
        // and also says everybody is done reading slot (kt-1) % R, which the next request overwrites
        const int newer = min(nk - 1, kt + R - 2) - kt;
        if (R > 3 && newer >= 2) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        else if (newer == 1) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + R - 1 < nk) issue(kt + R - 1);

        const char* sa = smem + (kt % R) * X3R_STAGE;
        const char* sb = sa + X3R_OP;
        const int kbase = kbeg + kt * X3_BK + 8 * lh;
        bf16x8 am[2][PLANES], bn[2][PLANES];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v[8];
            const int row = wm * 64 + 32 * i + lr;
            x3r_frag<LA>(sa, row, lh, v);
            if (p.a_drop.thresh) x3_mask8<LA>(p.a_drop, akey, p.a_drop_ld, adoff, m0 + row, kbase, v);
            if (LA == 1 && do_acs) asum[i] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] *= rsgn;     // row parity = lane parity on both sides (see x3_alt_undo)
            x3r_split<PLANES>(v, am[i]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[8];
            x3r_frag<LB>(sb, wn * 64 + 32 * j + lr, lh, v);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] *= rsgn;
            x3r_split<PLANES>(v, bn[j]);
        }
#pragma unroll
        for (int s = PLANES - 1; s >= 0; --s) {          // plane pairs (pa, pb) with pa + pb = s <= PLANES - 1
#pragma unroll
            for (int pa = 0; pa < PLANES; ++pa) {
                const int pb = s - pa;
                if (pb < 0 || pb >= PLANES) continue;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bn[j][pb], am[i][pa], acc[i][j]);
            }
        }
    }

    if (LA == 1 && do_acs) {        // row sums of the (masked) A operand: combine the two k-halves of a row
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float t = asum[i] + __shfl_xor(asum[i], 32, 64);
            const int m = m0 + wm * 64 + 32 * i + lr;
            if (lh == 0 && m < p.M) p.acs[((int64_t)by * gridDim.z + z) * p.M + m] = t;
        }
    }
    x3_alt_undo(acc, rsgn);
    if (HN > 0) {
        __syncthreads();                           // every wave is done with the ring: its first slots become staging
        x3_epilogue_hn<(HN > 0 ? HN : 32), 2>(p, acc, m0 + wm * 64 + lr, n0 + wn * 64 + 4 * lh, lane,
                                               reinterpret_cast<float*>(smem) + wave * X3_HN_STG);
    } else {
        __syncthreads();                           // every wave is done with the ring: its first slots become staging
        x3_epilogue<2>(p, acc, m0 + wm * 64, n0 + wn * 64, lane, reinterpret_cast<float*>(smem) + wave * X3_EP_STG, z, b0,
                       b1, by);
    }
}

// Packed-B kernel, bf16x3 (the pack kernels, the f16x2 twin and the family's host side: gt_gemm_x3p.hip).
// BN = 128: 2 x 2 waves of 64 x 64;  BN = 64 (narrow outputs: the 42 / 44-channel convolutions of the down-scaler, padded to
// 48): 4 x 1 waves of 32 x 64 -- a wave then splits ONE 32-row tile of A per stage for its twelve MFMAs, the same split-to-
// matrix ratio as the wide tile, and a 48-column product wastes a quarter of the tile instead of five eighths.
template <int LA, int HN, int CV, int BN = 128>     // CV: 0 plain, 1 implicit 3x3 convolution on A
__global__ __launch_bounds__(256, 3) void gemm_x3p_kernel(const GemmP p) {
    constexpr int MI = BN == 64 ? 1 : 2;           // 32-row tiles of A per wave
    static_assert(BN == 128 || (BN == 64 && HN == 0 && LA == 0), "the narrow tile serves plain / convolution launches");
    constexpr int R = X3P_R, PLANES = 3;
    constexpr int STG = (HN > 0 ? X3_HN_STG : X3_EP_STG) * 4 * 4;       // bytes of epilogue staging, four waves
    constexpr int SMEM = R * X3R_OP > STG ? R * X3R_OP : STG;
    __shared__ __attribute__((aligned(16))) char smem[SMEM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = BN == 64 ? wave : wave >> 1, wn = BN == 64 ? 0 : wave & 1;
    const int wrow = BN == 64 ? wm * 32 : wm * 64; // first tile row of this wave
    const int lr = lane & 31, lh = lane >> 5;
    int tile;
    {
        const int tiles = gridDim.x, q = tiles >> 3, r = tiles & 7;
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
    const int m0 = tm * X3_BM, n0 = tn * BN;
    const int kend = p.K;
    const float* A = p.A;
    const uint32_t akey = drop_key_dev(p.a_drop);

    float bias4[4] = {0.f, 0.f, 0.f, 0.f};         // the plain epilogue's bias, fetched under the K loop
    if (HN == 0) x3_bias4(p, n0 + wn * 64, lane, bias4);
    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nk = (kend + X3_BK - 1) / X3_BK;
    // Sign alternation in this kernel (no register to spare for a per-lane sign): the M-side sign alternates per 32-ROW TILE -- a
    // compile-time constant of the unrolled tile loop for the 64-row wave tile (a source modifier of the split's first
    // instructions), the wave's parity (a scalar) for the 32-row one -- the N-side per column (x3_pack_b_kernel)
    const float tsgn = x3_alt_sign(BN == 64 ? __builtin_amdgcn_readfirstlane(wm) : 0);
    const float* cv_row[2] = {A, A};
    int cv_ok[2] = {0, 0}, cv_none[2] = {0, 0}, cv_tap = 0, cv_c0 = 0;      // cv_none: a stage past the end of K reads zeros
    const int cv_cb = (p.cv_C & 31) ? 16 : 32;
    if (CV == 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + 16 * (wave * 2 + i) + (lane >> 2);
            if (m < p.M) {
                const int pix = m % (p.cv_H * p.cv_W), y = pix / p.cv_W, x = pix - y * p.cv_W;
                int ok = 0;
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    ok |= (((unsigned)(y + t / 3 - 1) < (unsigned)p.cv_H) && ((unsigned)(x + t % 3 - 1) < (unsigned)p.cv_W)) << t;
                cv_ok[i] = ok;
                cv_row[i] = A + (int64_t)m * p.lda;
            }
        }
    }
    auto issue = [&](int s) {                      // A stage s -> slot s % R : 2 load instructions per wave
        char* st = smem + (s % R) * X3R_OP;
        if (CV == 1) {
            x3r_issue_conv(cv_row, s < nk ? cv_ok : cv_none, cv_tap, cv_c0, p.cv_W, p.lda, st, wave, lane);
            cv_c0 += X3_BK;                        // channel block first, taps second, channel blocks last (gt_hip.h)
            if ((cv_c0 & (cv_cb - 1)) == 0) {
                cv_c0 -= cv_cb;
                if (++cv_tap == 9) { cv_tap = 0; cv_c0 += cv_cb; }
            }
        } else {
            x3r_issue<LA>(A, p.lda, m0, p.M, s * X3_BK, kend, st, wave, lane);
        }
    };
    // this wave's two 32-column B fragments of stage ks: plane pl, fragment j at bbase + pl * bplane + (j * KS + ks) KiB
    // (wave-uniform address in SGPRs + the lane's 16-byte slot).  The loads are inline asm on purpose: hipcc's own
    // scoreboard answers a register load inside this loop with s_waitcnt vmcnt(0) before the MFMAs, which also drains
    // the A stage requested a moment earlier (measured in the ISA); here the wait is the counted one below.
    const int wn_u = __builtin_amdgcn_readfirstlane(wn);
    const char* bbase = reinterpret_cast<const char*>(p.Bp) + (int64_t)((n0 + wn_u * 64) >> 5) * p.bp_KS * 1024;
    const int64_t bplane = (int64_t)p.bp_NT * p.bp_KS * 1024;
    const uint32_t voff = lane * 16;
    // Two register sets for B, one stage apart: B(kt + 1) is requested at the TOP of iteration kt, before the A stage of that
    // iteration, and is consumed one iteration later.  Vector-memory loads retire in order, so a wait for B also waits for
    // every A stage requested before it: with ONE set the loads of B(kt + 1) can only go out behind the MFMAs of B(kt), and
    // their latency (plus that of the A stage requested one iteration earlier) stands in front of every stage's MFMAs --
    // load, matrix and store time of a launch add up instead of overlapping (timing ablations: 37 + 15 + 30 = 82 us).
    bf16x8 bn0[2][PLANES], bn1[2][PLANES];
    auto loadb = [&](int ks, bf16x8 (&bn)[2][PLANES]) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                const char* sp = bbase + pl * bplane + ((int64_t)j * p.bp_KS + ks) * 1024;
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(bn[j][pl]) : "v"(voff), "s"(sp));
            }
    };
    // one 32-row tile of A at a time: its fragment is split and goes through its twelve MFMAs before the next one is read
    // (the three planes of ONE tile are live, not of both: the second B set has to fit under 168 registers)
    auto stage = [&](int kt, bf16x8 (&bn)[2][PLANES]) {
        const char* sa = smem + (kt % R) * X3R_OP;
        const int kbase = kt * X3_BK + 8 * lh;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            float v[8];
            bf16x8 am[PLANES];
            const int row = wrow + 32 * i + lr;
            x3r_frag<LA>(sa, row, lh, v);
            if (p.a_drop.thresh) x3_mask8<LA>(p.a_drop, akey, p.a_drop_ld, 0, m0 + row, kbase, v);
            if (MI == 1 || (i & 1)) {             // M-side: the sign alternates per 32-row tile (see below)
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = MI == 1 ? v[q] * tsgn : -v[q];
            }
            x3r_split<PLANES>(v, am);
#pragma unroll
            for (int s = PLANES - 1; s >= 0; --s) {      // plane pairs (pa, pb) with pa + pb = s, smallest terms first
#pragma unroll
                for (int pa = 0; pa < PLANES; ++pa) {
                    const int pb = s - pa;
                    if (pb < 0 || pb >= PLANES) continue;
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bn[j][pb], am[pa], acc[i][j]);
                }
            }
        }
    };
    // Request order of a wave:  B(0) A(0) .. A(R-2) | B(1) A(R-1) | B(2) A(R) | ...   (A = 2 loads, B = 6).
    // Top of iteration kt >= 1: A(kt) and B(kt) must have landed; the only request behind B(kt) is A(kt+R-2): vmcnt(2).
    // The barrier makes every wave's pieces of A(kt) visible and frees slot (kt-1) % R for the request of A(kt+R-1).
    // Tying the set to the statement keeps its MFMAs behind the wait.  Every iteration issues the same requests -- past
    // the end of K the A loader reads the zero line into a free slot and B re-reads its last stage -- so the counts hold
    // to the last stage and no load sits under a branch: a conditional asm load makes hipcc allocate fresh registers for
    // it and COPY them into the set at the join, before the data has arrived (seen in the ISA of a first version).
#define X3P_WAIT_AB(N, bn)                                                                                             \
    asm volatile("s_waitcnt vmcnt(" #N ")\n\ts_barrier"                                                                \
                 : "+v"(bn[0][0]), "+v"(bn[0][1]), "+v"(bn[0][2]), "+v"(bn[1][0]), "+v"(bn[1][1]), "+v"(bn[1][2])      \
                 :                                                                                                     \
                 : "memory")
    const int klast = nk - 1;
    loadb(0, bn0);
#pragma unroll
    for (int s = 0; s < R - 1; ++s) issue(s);
    X3P_WAIT_AB(4, bn0);                           // iteration 0: behind A(0) are the R - 2 other stages of the prologue
    loadb(klast < 1 ? klast : 1, bn1);
    issue(R - 1);
    stage(0, bn0);
    int kt = 1;
    for (; kt + 1 < nk; kt += 2) {
        X3P_WAIT_AB(2, bn1);
        loadb(kt + 1, bn0);
        issue(kt + R - 1);
        stage(kt, bn1);
        X3P_WAIT_AB(2, bn0);
        loadb(kt + 2 < klast ? kt + 2 : klast, bn1);
        issue(kt + R);
        stage(kt + 1, bn0);
    }
    if (kt < nk) {                                 // odd stage out (nk even): nothing left to request
        X3P_WAIT_AB(2, bn1);
        stage(kt, bn1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the zero stages requested past the end of K: the ring becomes staging
#undef X3P_WAIT_AB

#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float sg = MI == 1 ? tsgn : ((i & 1) ? -1.f : 1.f);
                acc[i][j][e] *= (e & 1) ? -sg : sg;
            }
    __syncthreads();                               // every wave is done with the ring: its first slots become staging
    if constexpr (HN > 0)
        x3_epilogue_hn<(HN > 0 ? HN : 32), 2>(p, acc, m0 + wm * 64 + lr, n0 + wn * 64 + 4 * lh, lane,
                                               reinterpret_cast<float*>(smem) + wave * X3_HN_STG);
    else
        x3_epilogue<MI>(p, acc, m0 + wrow, n0 + wn * 64, lane, reinterpret_cast<float*>(smem) + wave * X3_EP_STG, 0, 0, 0, 0,
                        bias4);
}

static int x3p_launch(const GemmP& p, const X3Pick& k, dim3 grid, hipStream_t st) { X3P_LAUNCH_PICK(gemm_x3p_kernel) }

// operands the ring kernel's direct loads can take (see its header comment)
static bool x3r_ok(const GemmP& p, int layout_a, int layout_b) {
    if (p.K2 > 0 || !p.a_vec || !p.b_vec) return false;
    if ((layout_a == 0 || layout_b == 0) && (p.K & 3)) return false;
    if (layout_a == 1 && (p.M & 3)) return false;
    if (layout_b == 1 && (p.N & 3)) return false;
    return true;
}

bool x3_shape_ok(const gt_gemm_desc* d) {
    // whole 128 x 128 tiles dominate (the padding of a partial edge tile is bounded by the sizes below)
    if (d->ep_mode != GT_EP_NORMAL && d->ep_mode != GT_EP_HEADNORM) return false;
    // narrow implicit convolutions (N >= 32) ride on the 64-wide tile of the packed-B kernel
    if (d->cv_c > 0 && !d->cv_wgrad && d->N >= 32 && d->N < 96 && d->M >= 1024 && d->K >= 16) return true;
    // round 6: narrow token products too (N < 96: the 64-column remainder of a width-split 192-wide product -- ex3's d_model --
    // and the d_model = 48 / 64 products of ex4 / ex1), under exactly the conditions that put them on the packed-B kernels
    // (x3_packed_ok), whose 128 x 64 tile instance takes N <= 64; they ran on the fp32 MFMA engine until now
    if (d->cv_c == 0 && d->N >= 16 && d->N < 96 && d->M >= 16384 && d->M >= 8 * (int64_t)d->N && d->K >= 16 &&
        (d->precision == GT_PREC_BF16X3 || d->precision == GT_PREC_F16X2) &&
        (d->K & 3) == 0 && d->layout_a == 0 && d->batch0 * d->batch1 == 1 && d->K2 == 0 && !d->a_colsum && d->split_k == 1 &&
        d->ep_mode == GT_EP_NORMAL && (d->lda & 3) == 0 && (reinterpret_cast<uintptr_t>(d->A) & 15) == 0)
        return true;
    // ... and the token-contracted weight gradients of the narrow models (ex1: d_model 64, ffn 128): gemm_x3w_kernel takes
    // partial 128-blocks since round 5, a lone 32 / 64-wide block is the same code path (they ran on the fp32 engine)
    if (d->precision == GT_PREC_F16X2 && d->layout_a == 1 && d->layout_b == 1 && d->split_k == 0 && d->K >= 16384 &&
        d->M >= 32 && d->N >= 32 && (d->M & 31) == 0 && (d->N & 31) == 0 && x3w_ok(d, 2))
        return true;
    return d->M >= 96 && d->N >= 96 && d->K >= 16;
}

// the fused head-norm epilogue exists on the ring kernel, three planes, 16-byte aligned everything
bool x3_headnorm_ok(const GemmP& p, int layout_a, int layout_b, int planes) {
    if (layout_a || layout_b || planes != 3 || !x3r_ok(p, 0, 0)) return false;
    if (p.hn_dk != 16 && p.hn_dk != 32 && p.hn_dk != 64) return false;
    if (p.hn_dkr != p.hn_dk && !(p.hn_dk == 64 && p.hn_dkr == 48 && p.Bp)) return false;   // head slots: packed-B kernels only
    if (p.hn_p > 4) return false;                  // the epilogue keeps a row's coordinates in four registers
    if (!p.c_vec || (p.N & 63) || (64 / p.hn_dk) * p.hn_DP + 4 > 88) return false;      // staging row fits X3_HN_STG
    auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    return al(p.bias) && al(p.hn_gamma) && al(p.hn_beta) && al(p.hn_out) && al(p.hn_stats);
}

// The instance a launch takes, decided ONCE: x3_launch switches on the pick, x3_kernel_name prints it.  hn = slot width of the
// fused head-norm epilogue (0: none).  Returns GT_EINVAL / GT_ENOTSUP where the launch refuses; `k` is filled in either way:
// x3_kernel_name is asked with a GemmP that carries shapes and alignment only (none of the pointers and picture sizes the
// refusals look at), so it prints the pick and does NOT refuse.
static int x3_pick(const GemmP& p, int layout_a, int layout_b, int planes, int hn, unsigned split, unsigned batch, X3Pick& k) {
    k = X3Pick{X3_STAGED, layout_a, layout_b, planes, hn, 0, 128};
    if (planes < 1 || planes > 3) return GT_EINVAL;
    const int lay = layout_a * 2 + layout_b;
    if (p.Bp) {                                    // packed-B kernels (x3_packed_ok said yes)
        k.family = p.bp_f16 ? X3_PACKED_H : X3_PACKED;
        k.LB = 0;
        if (p.cv_C > 0) { k.LA = 0; k.CV = 1; }
        if (p.N <= 64 && !hn && layout_a == 0) k.BN = 64;       // narrow output: 128 x 64 tiles
        return hn && !x3_headnorm_ok(p, layout_a, 0, planes) ? GT_ENOTSUP : 0;
    }
    if (hn) {                                      // fused head-norm epilogue: ring kernel, three planes
        k = X3Pick{X3_RING, 0, 0, 3, hn, 0, 128};
        return x3_headnorm_ok(p, layout_a, layout_b, planes) ? 0 : GT_ENOTSUP;
    }
    if (p.cv_C > 0 && p.cv_wgrad) {                // convolution weight gradient: nine taps x K chunks, 1-D grid
        k = X3Pick{X3_RING, 1, 1, planes, 0, 2, 128};
        return (lay != 3 || !x3r_ok(p, 1, 1) || batch != 9 || p.cv_W < X3_BK) ? GT_ENOTSUP : 0;
    }
    if (p.cv_C > 0) {                              // implicit convolution: ring kernel
        k = X3Pick{X3_RING, 0, 0, planes, 0, 1, 128};
        return (lay != 0 || !x3r_ok(p, 0, 0) || (p.cv_C & 15) || split != 1 || batch != 1) ? GT_ENOTSUP : 0;
    }
    if (p.wg_f16) k.family = X3_WGRAD;             // GT_PREC_F16X2 weight gradient (x3w_ok said yes)
    else if (x3r_ok(p, layout_a, layout_b)) k.family = X3_RING;
    return 0;
}

// ring depth 3: 3 stages x 16 KB = 48 KB, three blocks per CU (measured 38.0 ms/step at B128 against 38.35 for depth 4,
// 64 KB and two blocks per CU)
template <int LA, int LB, int CV>
static void x3r_launch_planes(const GemmP& p, int planes, dim3 grid, hipStream_t st) {
    if (planes == 1) hipLaunchKernelGGL((gemm_x3r_kernel<LA, LB, 1, 3, 0, CV>), grid, dim3(256), 0, st, p);
    else if (planes == 2) hipLaunchKernelGGL((gemm_x3r_kernel<LA, LB, 2, 3, 0, CV>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_x3r_kernel<LA, LB, 3, 3, 0, CV>), grid, dim3(256), 0, st, p);
}
template <int LA, int LB>
static void x3s_launch_planes(const GemmP& p, int planes, dim3 grid, hipStream_t st) {
    if (planes == 1) hipLaunchKernelGGL((gemm_x3_kernel<LA, LB, 1>), grid, dim3(256), 0, st, p);
    else if (planes == 2) hipLaunchKernelGGL((gemm_x3_kernel<LA, LB, 2>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_x3_kernel<LA, LB, 3>), grid, dim3(256), 0, st, p);
}

int x3_launch(const GemmP& p, int layout_a, int layout_b, int planes, unsigned tiles, unsigned split, unsigned batch,
              hipStream_t st) {
    X3Pick k;
    const int rc = x3_pick(p, layout_a, layout_b, planes, p.ep_mode == GT_EP_HEADNORM ? p.hn_dk : 0, split, batch, k);
    if (rc) return rc;
    const dim3 grid(tiles, split, batch);
    const int lay = k.LA * 2 + k.LB;
    switch (k.family) {
    case X3_PACKED:
    case X3_PACKED_H: {
        GemmP q = p;
        dim3 g = grid;
        if (k.BN == 64) {                          // p.tiles_n counts 128-wide tiles (one): the narrow tile's are 64 wide
            q.tiles_n = (p.N + 63) / 64;
            g = dim3((unsigned)(p.tiles_m * q.tiles_n));
        }
        return k.family == X3_PACKED_H ? x3h_launch(q, k, g, st) : x3p_launch(q, k, g, st);
    }
    case X3_WGRAD:
        return x3w_launch(p, tiles, split, st);
    case X3_RING:
        if (k.HN == 16) hipLaunchKernelGGL((gemm_x3r_kernel<0, 0, 3, 3, 16>), grid, dim3(256), 0, st, p);
        else if (k.HN == 32) hipLaunchKernelGGL((gemm_x3r_kernel<0, 0, 3, 3, 32>), grid, dim3(256), 0, st, p);
        else if (k.HN) hipLaunchKernelGGL((gemm_x3r_kernel<0, 0, 3, 3, 64>), grid, dim3(256), 0, st, p);
        else if (k.CV == 2) x3r_launch_planes<1, 1, 2>(p, k.PLANES, dim3((unsigned)(72 * ((tiles * split + 7) / 8))), st);
        else if (k.CV == 1) x3r_launch_planes<0, 0, 1>(p, k.PLANES, grid, st);
        else if (lay == 0) x3r_launch_planes<0, 0, 0>(p, k.PLANES, grid, st);
        else if (lay == 1) x3r_launch_planes<0, 1, 0>(p, k.PLANES, grid, st);
        else if (lay == 2) x3r_launch_planes<1, 0, 0>(p, k.PLANES, grid, st);
        else x3r_launch_planes<1, 1, 0>(p, k.PLANES, grid, st);
        break;
    case X3_STAGED:
        if (lay == 0) x3s_launch_planes<0, 0>(p, k.PLANES, grid, st);
        else if (lay == 1) x3s_launch_planes<0, 1>(p, k.PLANES, grid, st);
        else if (lay == 2) x3s_launch_planes<1, 0>(p, k.PLANES, grid, st);
        else x3s_launch_planes<1, 1>(p, k.PLANES, grid, st);
        break;
    }
    GT_LAUNCH_CHECK();
    return 0;
}

const char* x3_kernel_name(const GemmP& p, int layout_a, int layout_b, int planes, int hn_dk) {
    static thread_local char buf[112];
    X3Pick k;
    (void)x3_pick(p, layout_a, layout_b, planes, hn_dk, 1, 1, k);      // the pick only: see x3_pick on refusals
    switch (k.family) {
    case X3_PACKED:
    case X3_PACKED_H:
        snprintf(buf, sizeof(buf), "void gt::gemm_x3%c_kernel<%d, %d, %d, %d>(gt::GemmP)", k.family == X3_PACKED_H ? 'h' : 'p', k.LA, k.HN,
                 k.CV, k.BN);
        break;
    case X3_WGRAD:
        return "void gt::gemm_x3w_kernel<2>(gt::GemmP)";
    case X3_RING:
        snprintf(buf, sizeof(buf), "void gt::gemm_x3r_kernel<%d, %d, %d, 3, %d, %d>(gt::GemmP)", k.LA, k.LB, k.PLANES, k.HN, k.CV);
        break;
    case X3_STAGED:
        snprintf(buf, sizeof(buf), "void gt::gemm_x3_kernel<%d, %d, %d>(gt::GemmP)", k.LA, k.LB, k.PLANES);
        break;
    }
    return buf;
}

}  // namespace gt
