// Token-contracted fp16 weight gradient of the split-operand GEMM (gt_x3_core.h).
#include "gt_x3_core.h"

namespace gt {

// ---------------------------------------------------------------------------------------------------------------------
// Token-contracted weight gradients in GT_PREC_F16X2:  C[M][N] = sum_k A[k][M] B[k][N]  (both operands x-contiguous
// activations, K = tokens, M / N multiples of 128), split-K slabs like the ring kernel's.  gemm_x3r_kernel<1, 1> splits both
// operands again in every wave that multiplies them (each value is split twice per block, ~10 VALU instructions per MFMA:
// 121 / 181 us for 363 / 484 MB of operands); here a stage of 32 tokens is split ONCE, by the thread that fetched it, into
// two fp16 planes in LDS ([plane][k-group of 8 tokens][row]: a fragment is one aligned ds_read_b128, consecutive rows in
// consecutive 16-byte slots), and the four waves read their fragments from there: 24 MFMAs per wave and stage against ~180
// VALU instructions per thread.  The scale is one running exponent per operand and BLOCK: every stage the block takes the
// amax of the two tiles it is about to split (wave reduce + four floats through LDS, the barrier is there anyway), lowers the
// exponent -- rescaling its accumulators -- when the scaled amax would reach 2^15, and otherwise keeps it, so nothing can
// overflow and values are resolved to 2^-22 of the largest magnitude the block has seen (the weight gradient is a sum over
// all tokens: the tensor's scale is the relevant one).  Sign alternation as everywhere: odd rows of both operands enter negated.
constexpr int X3W_KG = 4;                            // k-groups (8 tokens) per stage
constexpr int X3W_PLANE = X3W_KG * 128 * 16;         // bytes of one plane of one operand tile: 8 KB

// PF = stages of raw operand values a thread keeps in flight (registers).  With PF = 1 the next stage was requested after the
// current one had been split, i.e. its latency was covered by 24 MFMAs only (~0.3 us against >= 2 us under load): every
// stage paid most of a memory round trip, and the launch time did not move when the counters showed a quarter less traffic
// (profiles/r05_x3w_prefetch.json).  PF = 2: the request for stage s + 2 is issued when stage s has been split, a full
// stage of split + MFMA work earlier; 32 more registers (180: two blocks per CU instead of three, four stages per CU in
// flight instead of three).
// PF = 2 is the only instance; the parameter stays part of the kernel's name.
template <int PF>
__global__ __launch_bounds__(256, 2) void gemm_x3w_kernel(const GemmP p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * X3W_PLANE];      // A planes 0 / 1, B planes 0 / 1
    __shared__ float red[1][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    int tile, by;
    if (p.x3w_map) {
        // 1-D grid, 8 * ceil(n_split / 8) * tiles blocks.  Workgroups go to the eight XCDs round-robin: XCD x owns the K
        // chunks [x spx, (x + 1) spx), and the 2 - 3 output tiles of ONE chunk are consecutive workgroups of that XCD -- they
        // stream the same rows of the narrower operand at the same time, so its second (third) reader is served by the XCD's
        // L2.  With tile = blockIdx.x and chunk = blockIdx.y the tiles of a chunk sit on DIFFERENT XCDs and the counters show
        // the operand fetched once per tile (485 -> 364 MB at [128 x 256], 727 -> 498 MB at [384 x 128]).
        const int tiles = p.tiles_m * p.tiles_n, spx = (p.n_split + 7) >> 3;
        const int s = blockIdx.x >> 3;
        by = (blockIdx.x & 7) * spx + s / tiles;
        tile = s % tiles;
        if (by >= p.n_split) return;
    } else {
        const int tiles = gridDim.x, q = tiles >> 3, r = tiles & 7;
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
        by = blockIdx.y;
    }
    const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
    const int m0 = tm * 128, n0 = tn * 128;
    const int kbeg = by * p.k_chunk, kend = min(p.K, kbeg + p.k_chunk);
    const bool do_acs = p.acs != nullptr && tn == 0;

    // staging role: waves 0, 1 stage the A tile, waves 2, 3 the B tile; a thread owns rows 4 r4 .. 4 r4 + 3 of its tile and the
    // eight tokens of k-group kg: eight 16-byte loads (a wave instruction covers 512 contiguous bytes of two token rows), four
    // 8-token units to split and store
    const bool isB = wave >= 2;                        // wave-uniform
    const int st = tid & 127, r4 = st & 31, kg = st >> 5;
    const int wsw = (r4 >> 1) & 3;                     // plane-store swizzle of rows 4 r4 + c:  ((4 r4 + c) >> 3) & 3
    const int lrs = lr ^ ((lr >> 3) & 3);              // fragment-read swizzle of row .. + lr (the tile bases are multiples of 32)
    const float* Op = isB ? p.B + n0 + 4 * r4 : p.A + m0 + 4 * r4;
    const int64_t ldo = isB ? p.ldb : p.lda;
    // A whole stage (the usual case, block-uniform test): the address of a load is a wave-uniform row pointer (token k0 + e of
    // the operand: scalar registers, advanced by scalar adds) + a per-thread byte offset that never changes -- no vector
    // address arithmetic and no branch per load (the general form below cost ~10 VALU / SALU instructions per load, a
    // fifth of the split phase this kernel is bound by, in shader-clock stamps per phase)
    const uint32_t voff = (uint32_t)((8 * kg * ldo + (isB ? n0 : m0) + 4 * r4) * (int64_t)sizeof(float));
    const char* rowbase = reinterpret_cast<const char*>(isB ? p.B : p.A);
    // round 5: partial edge tiles (M, N multiples of 32, e.g. ex3's 192 / 384 / 576): a thread whose four rows lie beyond the
    // operand's width stages zeros (its rows would be the NEXT token's values)
    const bool live = (isB ? n0 : m0) + 4 * r4 < (isB ? p.N : p.M);
    auto fetch = [&](f32x4 (&v)[8], int k0) __attribute__((always_inline)) {
        if (!live) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = f32x4{0.f, 0.f, 0.f, 0.f};
            return;
        }
        if (k0 + 32 <= kend) {
            const char* b = rowbase + (int64_t)k0 * ldo * (int64_t)sizeof(float);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                v[e] = *reinterpret_cast<const f32x4*>(b + (int64_t)e * ldo * (int64_t)sizeof(float) + voff);
            return;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + 8 * kg + e;
            v[e] = *reinterpret_cast<const f32x4*>(k < kend ? Op + (int64_t)k * ldo : x3_zero);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    int ea = X3H_E0, eb = X3H_E0;                      // block-uniform running exponents of the two operands
    float asum[4] = {0.f, 0.f, 0.f, 0.f};

    // one stage: the 32 tokens [k0, k0 + 32) whose values are in v; afterwards v holds the stage PF x 32 tokens further on
    auto stage = [&](f32x4 (&v)[8], int k0) __attribute__((always_inline)) {
        // amax of the stage (the values are in registers), per operand over its two waves
        float mx = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[e][0]), fabsf(v[e][1])), fmaxf(fabsf(v[e][2]), fabsf(v[e][3]))));
        // the exponents only move when some value would reach 2^LIMIT under the current one: a wave whose lanes are all
        // below that reports 0 ("in range") without the six cross-lane exchanges of a full reduction
        {
            const int xl = (int)(__float_as_uint(mx) >> 23);
            const bool over = xl + (isB ? eb : ea) - 127 >= X3H_LIMIT;
            if (__builtin_amdgcn_ballot_w64(over) != 0ull) {           // wave-uniform
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            } else {
                mx = 0.f;
            }
        }
        if (lane == 0) red[0][wave] = mx;
        __syncthreads();                               // also: every wave is done reading the previous stage's planes
        const float ma = fmaxf(red[0][0], red[0][1]), mb = fmaxf(red[0][2], red[0][3]);
        const int xa = (int)(__float_as_uint(ma) >> 23), xb = (int)(__float_as_uint(mb) >> 23);
        int d = 0;
        if (xa + ea - 127 >= X3H_LIMIT) { d += X3H_TARGET + 127 - xa - ea; ea = X3H_TARGET + 127 - xa; }
        if (xb + eb - 127 >= X3H_LIMIT) { d += X3H_TARGET + 127 - xb - eb; eb = X3H_TARGET + 127 - xb; }
        if (d != 0) {                                  // block-uniform
            const float f = d < -126 ? 0.f : pow2_f(d);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] *= f;
        }
        const float sc = pow2_f(isB ? eb : ea);
        char* planes = smem + (isB ? 2 * X3W_PLANE : 0);
        if (do_acs && !isB) {                          // column sums of A (the bias gradient): the four rows at once, as
            const f32x4 s4 = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));   // packed adds
#pragma unroll
            for (int c = 0; c < 4; ++c) asum[c] += s4[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {                  // row 4 r4 + c: its eight tokens -> one unit per plane
            const float sv = (c & 1) ? -sc : sc;          // odd rows enter negated
            uint32_t q[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t) x3h_split_pair(v[2 * t][c], v[2 * t + 1][c], sv, q[t]);
            // slot swizzle: row R sits in slot R ^ ((R >> 3) & 3).  A thread owns the four rows 4 r4 + c (its global loads are
            // float4 over rows), so without it the eight lanes of a ds_write_b128 pass hit 16-byte slots 64 bytes apart -- two
            // bank groups, a four-way conflict on every plane store (SQ_LDS_BANK_CONFLICT: 0.59 of the kernel's LDS cycles);
            // with it those eight slots are distinct modulo 8, and so are the eight consecutive rows of a fragment read
            const int off = (kg * 128 + 4 * r4 + (c ^ wsw)) << 4;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                *reinterpret_cast<u32x4*>(planes + pl * X3W_PLANE + off) = u32x4{q[0][pl], q[1][pl], q[2][pl], q[3][pl]};
        }
        if (k0 + 32 * PF < kend) fetch(v, k0 + 32 * PF);   // the values of stage s + PF travel under PF stages of work
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {               // two MFMA k-steps of 16 tokens
            f16x8 am[2][2], bn[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const int kq = 2 * ks + lh;
                    am[i][pl] = *reinterpret_cast<const f16x8*>(smem + pl * X3W_PLANE + ((kq * 128 + wm * 64 + 32 * i + lrs) << 4));
                    bn[i][pl] = *reinterpret_cast<const f16x8*>(smem + (2 + pl) * X3W_PLANE + ((kq * 128 + wn * 64 + 32 * i + lrs) << 4));
                }
#pragma unroll
            for (int s = 1; s >= 0; --s)
#pragma unroll
                for (int pa = 0; pa < 2; ++pa) {
                    const int pb = s - pa;
                    if (pb < 0 || pb > 1) continue;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = mfma32h(bn[j][pb], am[i][pa], acc[i][j]);
                }
        }
    };

    f32x4 v0[8], v1[8];
    if (kbeg < kend) fetch(v0, kbeg);
    if (kbeg + 32 < kend) fetch(v1, kbeg + 32);
    for (int k0 = kbeg; k0 < kend; k0 += 64) {
        stage(v0, k0);
        if (k0 + 32 < kend) stage(v1, k0 + 32);        // block-uniform
    }

    if (do_acs) {                                      // row sums of A: the four k-group threads of a row
        __syncthreads();
        float* part = reinterpret_cast<float*>(smem);
        if (!isB) {
#pragma unroll
            for (int c = 0; c < 4; ++c) part[kg * 128 + 4 * r4 + c] = asum[c];
        }
        __syncthreads();
        if (tid < 128 && m0 + tid < p.M)
            p.acs[(int64_t)by * p.M + m0 + tid] = (part[tid] + part[128 + tid]) + (part[256 + tid] + part[384 + tid]);
    }
    // un-scale, undo the sign, store the slab tile: lane (lr, lh) holds row m = .. + 32 i + lr and columns .. + 32 j + 8 g + 4 lh + t
    const int et = -(ea + eb), etc = et < -126 ? -126 : (et > 126 ? 126 : et);
    const float us = pow2_f(etc) * x3_alt_sign(lr);
    if (et != etc) {                   // operands below ~2^-100 of unit scale: apply the rest of the power of two first
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = ldexpf(acc[i][j][e], et - etc);
    }
    float* C = p.C + (int64_t)by * p.c_split;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + 32 * i + lr;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * 64 + 32 * j + 8 * g + 4 * lh;
                if (m < p.M && n < p.N)
                    *reinterpret_cast<f32x4*>(C + (int64_t)m * p.ldc + n) =
                        f32x4{acc[i][j][4 * g] * us, -acc[i][j][4 * g + 1] * us, acc[i][j][4 * g + 2] * us, -acc[i][j][4 * g + 3] * us};
            }
    }
}

// the launches gemm_x3w_kernel takes: GT_PREC_F16X2, both operands x-contiguous and 16-byte aligned, M / N multiples of 32 (partial
// edge tiles stage zeros: round 5, ex3's 192 / 384 / 576-wide weights),
// a long token contraction cut into split-K slabs (raw epilogue), no batching / dropout / second product
bool x3w_ok(const gt_gemm_desc* d, int split) {
    return d->precision == GT_PREC_F16X2 && d->layout_a == 1 && d->layout_b == 1 && split > 1 && d->K >= 16384 &&
           (d->M & 31) == 0 && (d->N & 31) == 0 && d->M >= 32 && d->N >= 32 && d->batch0 * d->batch1 == 1 && d->K2 == 0 && d->cv_c == 0 &&
           !(d->a_drop.p > 0.f) && ((reinterpret_cast<uintptr_t>(d->A) | reinterpret_cast<uintptr_t>(d->B)) & 15) == 0 &&
           (d->lda & 3) == 0 && (d->ldb & 3) == 0;
}

// a 1-D grid, chunk-major within an XCD (round 6: the same time as the tile-major grid at three tiles, and the narrower
// operand is fetched once instead of once per tile -- 727 -> ~500 MB at [384 x 128])
int x3w_launch(const GemmP& p, unsigned tiles, unsigned split, hipStream_t st) {
    GemmP q = p;
    q.x3w_map = 1;
    hipLaunchKernelGGL(gemm_x3w_kernel<2>, dim3(8u * ((split + 7) / 8) * tiles), dim3(256), 0, st, q);
    GT_LAUNCH_CHECK();
    return 0;
}

}  // namespace gt
