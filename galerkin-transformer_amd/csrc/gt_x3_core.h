// Split-operand bf16-MFMA GEMM kernel: fp32 operands, fp32 accumulation, fp32-equivalent results at the bf16
// matrix rate (v_mfma_f32_32x32x16_bf16 = 16x the flops per cycle of v_mfma_f32_16x16x4_f32).
//
// Every fp32 operand value a is split EXACTLY into up to three bf16 planes while it is staged into LDS,
//     h0 = bf16_rne(a),  h1 = bf16_rne(a - h0),  h2 = bf16_rne(a - h0 - h1)         (both subtractions are exact)
// so a = h0 + h1 + h2 up to 2^-24 |a| (three 8-bit significands cover the 24 bits of an fp32).  The product of two
// split operands is accumulated plane pair by plane pair into ONE fp32 accumulator, smallest terms first:
//     PLANES = 3 (GT_PREC_BF16X3):  a2 b0 + a1 b1 + a0 b2  (2^-16)  +  a1 b0 + a0 b1  (2^-8)  +  a0 b0
//                                   -- 6 MFMAs; dropped terms a1 b2, a2 b1, a2 b2 are <= 2^-23 |a||b|, i.e. the
//                                   rounding class of an fp32 FMA chain: this is the mode that meets the 1e-5 gate.
//     PLANES = 2 (GT_PREC_BF16X2):  a1 b0 + a0 b1 + a0 b0     -- 3 MFMAs, ~2^-16 relative (between bf16 and fp32)
//     PLANES = 1 (GT_PREC_BF16)  :  a0 b0                     -- 1 MFMA, operands rounded to bf16 (throughput mode)
// A bf16 x bf16 product is exact in fp32, so the only roundings are the accumulator's.
//
// Geometry: 256 threads = 2 x 2 waves, block tile 128 x 128, wave tile 64 x 64 = 2 x 2 MFMA 32x32 accumulators.
// One LDS stage = 16 k (one MFMA k-step), double-buffered; per operand and plane an image [128 rows][16 k] bf16
// with a 48-byte row pitch: the ds_write_b128 of a staging thread (its 8 consecutive k of one row) and the
// ds_read_b128 of an MFMA lane (row = lane & 31, k-half = lane >> 5) are both bank-conflict-free.
// The MFMA's "A" operand is the N-side (weight) tile and its "B" operand the M-side tile, so the 32x32 result
// registers of a lane are ONE output row m and four groups of 4 consecutive columns n -> 16-byte stores through the
// same fused epilogue as the fp32 kernels (ep_row).
// Loader: k-contiguous operands (L = 0) are read as two float4 per thread, x-contiguous ones (L = 1) as eight
// coalesced dword loads (64 consecutive rows per wave instruction); the dropout mask of the A prologue, the
// row-sum by-product (bias gradients), split-K, batching and the second accumulated product are those of gt_gemm.
//
// This header: what more than one kernel family (gt_gemm_x3.hip, gt_gemm_x3p.hip, gt_gemm_x3w.hip) uses -- the split, the stage
// loaders, the fragment readers of the ring images and the fused epilogues.
#pragma once
#include "gt_gemm_core.h"

namespace gt {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int X3_BM = 128, X3_BN = 128, X3_BK = 16, X3_PITCH = 48;       // bytes per LDS row (16 bf16 + pad)
constexpr int X3_PLANE = X3_BM * X3_PITCH;                               // 6144 B

// two fp32 -> PLANES packed bf16 pairs (exact residual chain, see the header comment)
template <int PLANES>
__device__ __forceinline__ void split_pair(float a, float b, uint32_t (&out)[PLANES]) {
    f32x2 r = {a, b};
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) {
        const bf16x2 h = __builtin_convertvector(r, bf16x2);            // v_cvt_pk_bf16_f32 (RNE)
        out[pl] = __builtin_bit_cast(uint32_t, h);
        if (pl + 1 < PLANES) r = r - __builtin_convertvector(h, f32x2);
    }
}

// 8 consecutive k (k0 .. k0+7) of operand row x:  L == 0: base[x*ld + k],  L == 1: base[k*ld + x].
// Branch-free: out-of-range elements are redirected to a device zero, so every lane issues the same loads and no
// s_waitcnt lands between the loads and the MFMAs of the stage being computed (a divergent loader makes hipcc drain
// vmcnt at the join, i.e. BEFORE the MFMAs it should overlap with).  `whole` (block-uniform): the stage lies inside
// [.., kend) and the operand is 16-byte aligned, so a k-contiguous row is two dwordx4 loads.
// (inline: one copy per translation unit's code object.  NOT static: hipcc emits other code around an internal symbol)
inline __device__ __attribute__((aligned(16))) float x3_zero[4] = {0.f, 0.f, 0.f, 0.f};

template <int L>
__device__ __forceinline__ void x3_load8(const float* __restrict__ base, int64_t ld, int x, int X, int k0, int kend,
                                         bool whole, float (&v)[8]) {
    const bool row_ok = x < X;
    if (L == 0) {
        const float* ptr = base + (int64_t)x * ld + k0;
        if (whole) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(row_ok ? ptr : x3_zero);
            const f32x4 b = *reinterpret_cast<const f32x4*>(row_ok ? ptr + 4 : x3_zero);
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
            v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *((row_ok && k0 + j < kend) ? ptr + j : x3_zero);
        }
    } else {
        const float* ptr = base + (int64_t)k0 * ld + x;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *((row_ok && (whole || k0 + j < kend)) ? ptr + (int64_t)j * ld : x3_zero);
    }
}

// stateless dropout mask of the A prologue on the 8 staged values (same mask index as gload in gt_gemm_core.h)
template <int L>
__device__ __forceinline__ void x3_mask8(const DropDev& dd, uint32_t dkey, int64_t dld, int64_t dboff, int x, int k0,
                                         float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t di = dboff + (L == 0 ? (int64_t)x * dld + k0 + j : (int64_t)(k0 + j) * dld + x);
        v[j] *= drop_mul(dd, dkey, (uint32_t)di);
    }
}

template <int PLANES>
__device__ __forceinline__ void x3_store8(char* __restrict__ img, int row, int khalf, const float (&v)[8]) {
    uint32_t q[4][PLANES];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_pair<PLANES>(v[2 * i], v[2 * i + 1], q[i]);
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl)
        *reinterpret_cast<u32x4*>(img + pl * X3_PLANE + row * X3_PITCH + khalf * 16) =
            u32x4{q[0][pl], q[1][pl], q[2][pl], q[3][pl]};
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// Sign-alternating accumulation.  Measured on gfx950 (tools/mfma_chain_probe.hip,
// profiles/r05_mfma_chain_probe.json): the bf16 MFMA does not round its sum to nearest -- addends whose low bits fall below
// the accumulator's guard bits are chopped toward -infinity.  Per instruction that is ~2^-9 ulp, but it has ONE direction:
// a chain of six plane products per stage ends ~0.1 of its rms error below the exact sum in EVERY output element, whatever
// the operand signs (K = 1152: mean signed error -2.7e-9 sum|a||b| against an rms of 2.4e-8; negate one operand and the
// mean becomes +2.8e-9; the fp32 MFMA chain: 1e-11).  A coherent offset like that survives every later reduction over
// tokens or pixels that the zero-mean part averages away: it was the 10x excess of the default arithmetic in the
// exact-math gradient parity of the whole model.  The kernels therefore negate the operand rows of
// odd index on both sides (the M-side row in registers, the N-side row at pack / split time; the packed-B kernel, which
// has no register left for a per-lane sign, alternates its M side per 32-row tile instead), so the chain of output
// (m, n) is accumulated with the sign (-1)^(m+n), and undo it on the accumulator before the epilogue: per-element
// accuracy is unchanged, the offset alternates in a checkerboard and cancels in any sum over rows or columns.
// sign of operand row `parity & 1`
__device__ __forceinline__ float x3_alt_sign(int parity) { return (parity & 1) ? -1.f : 1.f; }
// accumulator register e of a lane = output (m = the lane's own row, n = .. + 8 (e >> 2) + 4 lh + (e & 3)): n's parity is e & 1
template <int NI, int NJ>
__device__ __forceinline__ void x3_alt_undo(f32x16 (&acc)[NI][NJ], float rsgn) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] *= (e & 1) ? -rsgn : rsgn;
}

// ---- two-term fp16 arithmetic (GT_PREC_F16X2) --------------------------------------------------------------------------
// fp32-class results from THREE products per stage instead of six: every operand value x is split as
//     h0 = f16_rne(x s),  h1 = f16_rne(x s - h0)          (s a power of two; 11 + 11 significand bits, both steps exact)
// and the products h1 g0 + h0 g1 + h0 g0 are accumulated in fp32 by v_mfma_f32_32x32x16_f16 (dropped: h1 g1 <= 2^-22).
// fp16 has five exponent bits, so the scale s must track the data; no tensor statistics are passed in for that:
//   * N side (the packed weight): x3_pack_b16_kernel takes the amax of each 32-column fragment tile when it packs it and
//     stores the tile's exponent behind the planes -- a wave-uniform factor of one accumulator column block;
//   * M side (activation rows, split in registers): a lane holds ONE row of its 32-row tile (and with the N-side tile as
//     the MFMA's first operand all sixteen accumulator registers of that lane belong to that row), so the scale is a
//     PER-ROW running exponent kept in the lane: before a stage's eight values are split the lane pair of the row takes
//     their amax; if amax 2^e would reach 2^15 the exponent is lowered to put it at 2^13 and the lane's accumulators are
//     multiplied by the same power of two (exact) -- the online-rescaling of a streaming softmax, applied to a dot
//     product.  Nothing can overflow (the check precedes the split), a row whose early stages are its largest simply
//     resolves the later ones relative to that maximum, like any fp32 accumulation does.
// The accumulators are un-scaled together with the alternating sign, before the epilogue.
constexpr int X3H_E0 = 120;                       // start exponent: any non-zero first stage sets the real one
constexpr int X3H_TARGET = 13, X3H_LIMIT = 15;    // scaled row amax is put in [2^13, 2^14) and kept below 2^15

// two fp32 times the scale -> two packed fp16 pairs (round 5: four v_fma_mix* instead of multiply + conversions, gt_common.h)
__device__ __forceinline__ void x3h_split_pair(float a, float b, float s, uint32_t (&out)[2]) {
    f16_mulsplit_pair(a, s, b, s, out[0], out[1]);
}

__device__ __forceinline__ f32x16 mfma32h(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Epilogue shared by both kernels.  Result registers of the 32x32 MFMA with the N-side tile as its A operand: lane
// (lr = lane & 31, lh = lane >> 5) holds output row  mrow + 32 i  of accumulator (i, j) and the four 4-column groups
// ncol + 32 j + 8 g .. + 3  (ncol already includes 4 * lh).
// The 32x32 MFMA leaves a lane with ONE output row and 4-column groups 32 bytes apart, so stores (and the epilogue's
// res / aux / add loads) straight from the accumulator layout touch 32-byte pieces of 32 different rows per
// instruction: rocprofv3 WRITE_SIZE showed 1.4-1.6x the algorithmic bytes on every token GEMM (profiles/
// r02m_pmc_step_summary.txt).  The wave therefore transposes its 32 x 64 row tile through a private LDS tile first:
// afterwards 16 consecutive lanes hold one row's 64 columns and every global access of the fused epilogue is a full
// 256-byte row segment.  mtile0 / ntile0: first row / column of the wave's tile.  stg: 32 x X3_EP_SW floats.
constexpr int X3_EP_SW = 68;                     // staging row pitch in floats (64 + 4: conflict-free both ways)
constexpr int X3_EP_STG = 32 * X3_EP_SW;

// The epilogue's four bias values of a lane (columns ntile0 + 4 (lane & 15) ..): a kernel that fetches them in front of
// its K loop takes one memory round trip out of every block's epilogue.
__device__ __forceinline__ void x3_bias4(const GemmP& p, int ntile0, int lane, float (&b)[4]) {
    const int nb = ntile0 + 4 * (lane & 15);
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = (p.bias && nb + t < p.N) ? p.bias[nb + t] : 0.f;
}

// Batched form of the fused epilogue for whole, 16-byte aligned tiles (every token GEMM of the hot path).  ep_row handles
// one row segment at a time behind run-time switches: each segment's res / aux load was followed by its use, and the
// s_waitcnt vmcnt(0) in front of that use also waited for the STORES of the segments before it -- sixteen store round
// trips in a row per wave.  A block of the FFN launch spent 15.6 us of its 28.7 us in the epilogue writing 64 KB, and
// 55-60 % of the resident blocks of the chip were in that state at any time (per-block wall-clock stamps, profiles/r03z_*).
// Here a wave works in batches of four segments (16 rows x 256 B): the res / aux loads of batch b + 1 are issued before
// the stores of batch b, the values of a batch are computed together, and nothing ever waits for a store.
template <int MI>
__device__ __forceinline__ void x3_epilogue_fast(const GemmP& p, const f32x16 (&acc)[MI][2], int mtile0, int nb, int lane,
                                                 float* __restrict__ stg, float* __restrict__ C, int z, int b0, int b1,
                                                 const float (&biasv)[4], uint32_t dkey) {
    constexpr int NB = 2 * MI, HB = 4;
    const int lr = lane & 31, lh = lane >> 5, c4 = lane & 15, rsub = lane >> 4;
    const float* resb = p.res ? p.res + b0 * p.r_bs0 + b1 * p.r_bs1 + nb : nullptr;
    const float* auxb = p.aux_op ? p.aux + b0 * p.aux_bs0 + b1 * p.aux_bs1 + nb : nullptr;
    f32x4 rs[HB], ax[HB];
    auto loads = [&](int b) {
        f32x4 (&r)[HB] = rs;
        f32x4 (&a)[HB] = ax;
        if (resb) {
#pragma unroll
            for (int k = 0; k < HB; ++k)
                r[k] = *reinterpret_cast<const f32x4*>(resb + (int64_t)(mtile0 + 16 * b + 4 * k + rsub) * p.ldr);
        }
        if (auxb) {
#pragma unroll
            for (int k = 0; k < HB; ++k)
                a[k] = *reinterpret_cast<const f32x4*>(auxb + (int64_t)(mtile0 + 16 * b + 4 * k + rsub) * p.ldaux);
        }
    };
    loads(0);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = b >> 1;
        if ((b & 1) == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4*>(stg + lr * X3_EP_SW + 32 * j + 8 * g + 4 * lh) =
                        f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
            // wave-private tile, LDS operations of one wave execute in order: a compiler fence + counter wait is enough
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        f32x4 v[HB];
#pragma unroll
        for (int k = 0; k < HB; ++k)
            v[k] = *reinterpret_cast<const f32x4*>(stg + (16 * (b & 1) + 4 * k + rsub) * X3_EP_SW + 4 * c4);
        if (b & 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the next tile is staged
        const int m0b = mtile0 + 16 * b + rsub;                       // row of segment k: m0b + 4 k
#pragma unroll
        for (int k = 0; k < HB; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t) v[k][t] = p.alpha * v[k][t] + biasv[t];
        if (p.act == GT_ACT_DROP_SILU) {     // dropout in front of the SiLU; `pre` = keepscale * silu'(u) (gt_hip.h, ep_row)
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                const uint32_t di = (uint32_t)(((int64_t)z * p.M + m0b + 4 * k) * p.drop_ld + p.n_off + nb);
                f32x4 df;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float ks = p.drop.thresh ? drop_mul(p.drop, dkey, di + t) : 1.f;
                    float a, da;
                    silu_both(v[k][t] * ks, a, da);
                    v[k][t] = a;
                    df[t] = ks * da;
                }
                if (p.pre) *reinterpret_cast<f32x4*>(p.pre + ((int64_t)z * p.M + m0b + 4 * k) * p.ldpre + nb) = df;
            }
        } else if (p.act == GT_ACT_SILU2) {     // silu(silu(v)); `pre` = silu'(v) silu'(silu(v)) (gt_hip.h, ep_row)
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                f32x4 df;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float a1, d1, a2, d2;
                    silu_both(v[k][t], a1, d1);
                    silu_both(a1, a2, d2);
                    v[k][t] = a2;
                    df[t] = d1 * d2;
                }
                if (p.pre) *reinterpret_cast<f32x4*>(p.pre + ((int64_t)z * p.M + m0b + 4 * k) * p.ldpre + nb) = df;
            }
        } else if (p.pre) {
#pragma unroll
            for (int k = 0; k < HB; ++k)
                *reinterpret_cast<f32x4*>(p.pre + ((int64_t)z * p.M + m0b + 4 * k) * p.ldpre + nb) = v[k];
        }
        if (p.act == GT_ACT_RELU) {
#pragma unroll
            for (int k = 0; k < HB; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t) v[k][t] = fmaxf(v[k][t], 0.f);
        } else if (p.act == GT_ACT_SILU) {
#pragma unroll
            for (int k = 0; k < HB; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t) v[k][t] = silu_f(v[k][t]);
        }
        if (auxb) {
            const f32x4 (&a)[HB] = ax;
            if (p.aux_op == GT_AUX_GT0) {
#pragma unroll
                for (int k = 0; k < HB; ++k)
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[k][t] *= a[k][t] > 0.f ? p.aux_scale : 0.f;
            } else if (p.aux_op == GT_AUX_DSILU) {
#pragma unroll
                for (int k = 0; k < HB; ++k)
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[k][t] *= dsilu_f(a[k][t]);
            } else {
#pragma unroll
                for (int k = 0; k < HB; ++k)
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[k][t] *= a[k][t] * p.aux_scale;
            }
        }
        if (p.drop.thresh && p.act != GT_ACT_DROP_SILU) {
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                const uint32_t di = (uint32_t)(((int64_t)z * p.M + m0b + 4 * k) * p.drop_ld + p.n_off + nb);
#pragma unroll
                for (int t = 0; t < 4; ++t) v[k][t] *= drop_mul(p.drop, dkey, di + t);
            }
        }
        if (resb) {
            const f32x4 (&r)[HB] = rs;
#pragma unroll
            for (int k = 0; k < HB; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t) v[k][t] = r[k][t] + p.out_scale * v[k][t];
        } else {
#pragma unroll
            for (int k = 0; k < HB; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t) v[k][t] *= p.out_scale;
        }
        if (b + 1 < NB) loads(b + 1);          // rs / ax are consumed: the next batch's loads go out in front of the stores
#pragma unroll
        for (int k = 0; k < HB; ++k) *reinterpret_cast<f32x4*>(C + (int64_t)(m0b + 4 * k) * p.ldc + nb) = v[k];
        if (p.c2) {                            // gt_gemm_desc.c_masked: the same rows under the second mask
            const uint32_t key2 = drop_key_dev(p.drop2);
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                const uint32_t di = (uint32_t)(((int64_t)z * p.M + m0b + 4 * k) * p.drop_ld + p.n_off + nb);
                f32x4 w = v[k];
                if (p.drop2.thresh) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) w[t] *= drop_mul(p.drop2, key2, di + t);
                }
                *reinterpret_cast<f32x4*>(p.c2 + (int64_t)(m0b + 4 * k) * p.ldc2 + nb) = w;
            }
        }
    }
}

template <int MI>
__device__ __forceinline__ void x3_epilogue(const GemmP& p, const f32x16 (&acc)[MI][2], int mtile0, int ntile0, int lane,
                                            float* __restrict__ stg, int z, int b0, int b1, int sidx,
                                            const float* bias_pre = nullptr) {     // bias_pre: x3_bias4() of this lane
    const int64_t coff = b0 * p.c_bs0 + b1 * p.c_bs1 + (int64_t)sidx * p.c_split;
    float* __restrict__ C = p.C + coff;
    const uint32_t dkey = drop_key_dev(p.drop);
    const int lr = lane & 31, lh = lane >> 5;
    const int c4 = lane & 15, rsub = lane >> 4;          // read side: 16 lanes per row, 4 rows per instruction
    const int nb = ntile0 + 4 * c4;
    const bool col_ok = nb < p.N, full = nb + 4 <= p.N;
    float biasv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) biasv[t] = bias_pre ? bias_pre[t] : (p.bias && nb + t < p.N) ? p.bias[nb + t] : 0.f;
    if (p.c_vec && !p.raw && !p.rp && !p.add && ntile0 + 64 <= p.N && mtile0 + 32 * MI <= p.M) {   // wave-uniform
        x3_epilogue_fast<MI>(p, acc, mtile0, nb, lane, stg, C, z, b0, b1, biasv, dkey);
        return;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<f32x4*>(stg + lr * X3_EP_SW + 32 * j + 8 * g + 4 * lh) =
                    f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        // wave-private tile, LDS operations of one wave execute in order: a compiler fence + counter wait is enough
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int r = 4 * it + rsub, m = mtile0 + 32 * i + r;
            const f32x4 t4 = *reinterpret_cast<const f32x4*>(stg + r * X3_EP_SW + 4 * c4);
            if (m < p.M && col_ok) {
                float v[4] = {t4[0], t4[1], t4[2], t4[3]};
                ep_row<4>(p, v, biasv, C, m, nb, z, b0, b1, full, dkey);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the next row tile overwrites the staging
    }
}

// GT_EP_HEADNORM epilogue (QKV projection + per-head LayerNorm + position columns, see gt_hip.h): same register map
// as x3_epilogue.  A head segment (DK columns) of output row m lies inside this wave's 64 columns and is shared by
// the lane pair (lane, lane ^ 32): each lane holds DK / 2 of its values, so the statistics are a local sum plus ONE
// cross-lane exchange.  Raw projection -> C (16-byte stores).  The head-tile rows ([pos | values | pad], DP floats per
// head, the wave's 64 / DK heads adjacent in memory) are first assembled in a wave-private LDS tile and then written
// as whole 16-byte aligned granules, a row at a time: with the coordinates in front the values sit at an 8-byte
// offset, and storing them straight from the accumulator layout (8-byte pieces of 32 different rows per instruction)
// cost 1.26 GB of HBM writes for 0.77 GB of data (rocprofv3 WRITE_SIZE, profiles/r02_pmc_step.json).
constexpr int X3_HN_STG = 32 * 88;               // floats of staging per wave: 32 rows x (4 heads x DP 20 + pad) max

template <int DK, int MI>
__device__ __forceinline__ void x3_epilogue_hn(const GemmP& p, const f32x16 (&acc)[MI][2], int mrow, int ncol, int lane,
                                               float* __restrict__ stg) {
    constexpr int NSEG = 64 / DK, GPS = DK / 8;              // segments per wave row; 4-column groups per lane per segment
    const int lr = lane & 31, lh = lane >> 5;
    const int nwave = ncol - 4 * lh;                          // first column of this wave's 64 (a multiple of 64)
    if (nwave >= p.N) return;                                 // wave-uniform: N is a multiple of 64 here
    // head slots (DK = 64 only): the head occupies the first DKR = hn_dkr (48) columns of its 64-column slot, the accumulators
    // of the 16 columns behind it are exact zeros (zero rows of the packed weight).  GPR: the lane's real 4-column groups.
    const int DKR = (DK == 64) ? p.hn_dkr : DK, GPR = DKR >> 3;
    const float inv = 1.f / (float)DKR;
    const int DP = p.hn_DP, W = NSEG * DP, sw = W + 4, W4 = W >> 2;
    const int stream = nwave / (p.hn_h * DK), head0 = (nwave / DK) % p.hn_h;
    const bool normed = (p.hn_mask >> stream) & 1;
    const bool store_raw = !((p.hn_skip_raw >> stream) & 1);   // the raw projection of this stream goes to C
    const int ni = __popc(p.hn_mask & ((1 << stream) - 1));
    // What the tile loop reads from memory (bias, the rows' coordinates) is fetched here, in front of the first store: a
    // load inside the loop is followed by its use, and the s_waitcnt vmcnt(0) in front of that use also waits for every
    // store issued before it (the serialisation x3_epilogue_fast removes from the plain epilogue).  gamma / beta stay in
    // the loop: the hot path writes plain tiles (hn_plain), and 64 more registers would spill.
    f32x4 bv[NSEG][GPS];
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg)
#pragma unroll
        for (int q = 0; q < GPS; ++q)
            bv[sg][q] = (p.bias && q < GPR) ? *reinterpret_cast<const f32x4*>(p.bias + (nwave / DK + sg) * DKR + 8 * q + 4 * lh)
                                             : f32x4{0.f, 0.f, 0.f, 0.f};
    // granule walk of the tile store below: lane's first granule (row, 16-byte column) and the step of 64 granules
    const int g_r0 = lane / W4, g_c0 = lane - g_r0 * W4, g_dr = 64 / W4, g_dc = 64 - g_dr * W4;
    const int nit = (32 * W4 + 63) >> 6, rstride = p.hn_h * DP;
    float posv[MI][4];                                        // hn_p <= 4 coordinates of this lane's rows (lane half 0 writes them)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            posv[i][jj] = (lh == 0 && jj < p.hn_p && mrow + 32 * i < p.M) ? p.hn_pos[(int64_t)(mrow + 32 * i) * p.hn_p + jj] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = mrow + 32 * i;
        const bool row_ok = m < p.M;
        float* srow = stg + lr * sw;
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) {
            const int head = head0 + sg;
            float v[GPS][4];
#pragma unroll
            for (int q = 0; q < GPS; ++q) {
                const int c = sg * DK + 8 * q;                // column offset of this group inside the wave's 64 (+ 4 lh)
                const int j = c >> 5, g = (c & 31) >> 3;
#pragma unroll
                for (int t = 0; t < 4; ++t) v[q][t] = p.alpha * acc[i][j][4 * g + t] + bv[sg][q][t];
                if (row_ok && store_raw && q < GPR)          // (column of the caller's [M, 3 h DKR] projection)
                    *reinterpret_cast<f32x4*>(p.C + (int64_t)m * p.ldc + (nwave / DK + sg) * DKR + 8 * q + 4 * lh) =
                        f32x4{v[q][0], v[q][1], v[q][2], v[q][3]};
            }
            float mu = 0.f, rstd = 1.f;
            if (normed) {                                     // wave-uniform branch: the exchange below is convergent
                float sum = 0.f;
#pragma unroll
                for (int q = 0; q < GPS; ++q)
                    if (q < GPR) sum += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
                sum = xor32_sum(sum);
                mu = sum * inv;
                float ss = 0.f;
#pragma unroll
                for (int q = 0; q < GPS; ++q)
                    if (q < GPR) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) { const float c0 = v[q][t] - mu; ss = fmaf(c0, c0, ss); }
                    }
                ss = xor32_sum(ss);
                rstd = 1.f / sqrtf(ss * inv + p.hn_eps);
            }
            float* seg = srow + sg * DP;
#pragma unroll
            for (int q = 0; q < GPS; ++q) {
                if (q >= GPR) continue;
                const int dim = 8 * q + 4 * lh;
                float y[4] = {v[q][0], v[q][1], v[q][2], v[q][3]};
                if (normed) {
                    if (p.hn_plain) {                         // the product path of the Galerkin layers: no load in the loop
#pragma unroll
                        for (int t = 0; t < 4; ++t) y[t] = (y[t] - mu) * rstd;
                    } else {
                        const f32x4 gm = *reinterpret_cast<const f32x4*>(p.hn_gamma + (ni * p.hn_h + head) * DKR + dim);
                        const f32x4 bt = *reinterpret_cast<const f32x4*>(p.hn_beta + (ni * p.hn_h + head) * DKR + dim);
#pragma unroll
                        for (int t = 0; t < 4; ++t) y[t] = (y[t] - mu) * rstd * gm[t] + bt[t];
                    }
                }
                float* dst = seg + p.hn_p + dim;
                if ((p.hn_p & 1) == 0) {                      // two 8-byte stores (the coordinates in front shift the head by
                    // hn_p floats: no 16-byte alignment).  Thirty-two rows at a pitch that is a multiple of four floats meet in
                    // eight banks: four scalar stores per group were the kernel's LDS bank conflicts (0.58 - 0.77 of its LDS cycles)
                    *reinterpret_cast<f32x2*>(dst) = f32x2{y[0], y[1]};
                    *reinterpret_cast<f32x2*>(dst + 2) = f32x2{y[2], y[3]};
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) dst[t] = y[t];
                }
            }
            if (lh == 0) {                                    // one lane of the pair: coordinates, padding, statistics
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (jj < p.hn_p) seg[jj] = posv[i][jj];
                for (int jj = p.hn_p + DKR; jj < DP; ++jj) seg[jj] = 0.f;
                if (normed && row_ok)
                    *reinterpret_cast<f32x2*>(p.hn_stats + (((int64_t)ni * p.M + m) * p.hn_h + head) * 2) = f32x2{mu, rstd};
            }
        }
        // the tile is wave-private and LDS operations of one wave execute in order: a compiler fence is enough
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the tile's rows go out as whole 16-byte granules, 64 per instruction (lane -> granule e = lane + 64 it of the
        // 32 x W4 tile, walked incrementally), three instructions' worth of LDS reads in front of their three stores:
        // the straightforward loop (a division and 64-bit address arithmetic per granule, every read waited for before
        // its store) was 45 instructions + an LDS round trip per granule, 18 times per wave
        const int mbase = mrow - lr + 32 * i;
        float* __restrict__ gtile = p.hn_out + (((int64_t)stream * p.M + mbase) * p.hn_h + head0) * DP;
        const int nrows = p.M - mbase < 32 ? p.M - mbase : 32;
        int r = g_r0, c4 = g_c0;
        for (int it = 0; it < nit; it += 3) {
            f32x4 val[3];
            int off[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                off[u] = r < nrows ? r * rstride + 4 * c4 : -1;
                if (r < 32) val[u] = *reinterpret_cast<const f32x4*>(stg + r * sw + 4 * c4);
                r += g_dr; c4 += g_dc;
                if (c4 >= W4) { c4 -= W4; ++r; }
            }
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (off[u] >= 0) *reinterpret_cast<f32x4*>(gtile + off[u]) = val[u];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads are done before the next row tile overwrites the staging
    }
}
// ---- stage images of the ring kernels (gemm_x3r_kernel, the packed-B kernels) ------------------------------------------
// LDS images of one stage (A then B, 8 KB each); a direct load writes wave-uniform base + lane * 16 B, so the images are
// lane-linear and every swizzle is applied to the SOURCE address:
//   k-contiguous operand (L == 0):  [128 rows][16 k]: the 16-byte granule g of row r sits at slot g ^ ((r >> 2) & 3);
//                                   an MFMA lane (row, k-half h) reads granules 2h and 2h + 1 (two conflict-free
//                                   ds_read_b128);
//   x-contiguous operand (L == 1):  [16 k][128 x] as in memory; a lane reads its row's 8 k as 8 ds_read_b32 (lanes of a
//                                   half-wave hit consecutive banks).
typedef __attribute__((address_space(3))) void* x3_lds_ptr;
typedef const __attribute__((address_space(1))) void* x3_glb_ptr;
constexpr int X3R_OP = X3_BM * X3_BK * 4;        // 8192 B: one operand tile of one stage
constexpr int X3R_STAGE = 2 * X3R_OP;

template <int L>
__device__ __forceinline__ void x3r_issue(const float* __restrict__ base, int64_t ld, int x0, int X, int k0, int kend,
                                          char* img, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = wave * 2 + i;                // 1-KiB piece of the 8-KiB image
        const float* src;
        if (L == 0) {
            const int row = 16 * q + (lane >> 2), slot = lane & 3;
            const int g = slot ^ ((row >> 2) & 3);
            const int x = x0 + row, k = k0 + 4 * g;
            src = (x < X && k < kend) ? base + (int64_t)x * ld + k : x3_zero;
        } else {
            const int kr = 2 * q + (lane >> 5), xx = x0 + 4 * (lane & 31), k = k0 + kr;
            src = (k < kend && xx < X) ? base + (int64_t)k * ld + xx : x3_zero;
        }
        __builtin_amdgcn_global_load_lds((x3_glb_ptr)src, (x3_lds_ptr)(img + q * 1024), 16, 0, 0);
    }
}

// this lane's 8 consecutive k (k-half lh) of tile row `row` (0..127) from a stage image
template <int L>
__device__ __forceinline__ void x3r_frag(const char* __restrict__ img, int row, int lh, float (&v)[8]) {
    if (L == 0) {
        const int s = (row >> 2) & 3;
        const f32x4 a = *reinterpret_cast<const f32x4*>(img + row * 64 + (((2 * lh) ^ s) << 4));
        const f32x4 b = *reinterpret_cast<const f32x4*>(img + row * 64 + (((2 * lh + 1) ^ s) << 4));
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
        v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
        const float* f = reinterpret_cast<const float*>(img) + (8 * lh) * X3_BM + row;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f[j * X3_BM];
    }
}

template <int PLANES>
__device__ __forceinline__ void x3r_split(const float (&v)[8], bf16x8 (&out)[PLANES]) {
    uint32_t q[4][PLANES];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_pair<PLANES>(v[2 * i], v[2 * i + 1], q[i]);
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl)
        out[pl] = __builtin_bit_cast(bf16x8, u32x4{q[0][pl], q[1][pl], q[2][pl], q[3][pl]});
}

// Implicit 3x3 convolution (gt_hip.h: cv_*): the k-contiguous A image of a stage is the 16 channels [c0, c0 + 16) of
// tap (dy, dx) of the tile's 128 pixels -- a lane's granule comes from its pixel's neighbour row, or from x3_zero
// outside the picture.  A stage never straddles two taps (cv_C % 16 == 0).  `ok` = the lane's pixel's 9 tap-valid bits.
// Stage order: the nine taps of one 32-channel block (16 when cv_C % 32 != 0) before the next block -- a pixel's 128-byte
// line is then read by its nine taps within 18 consecutive stages and stays in L2; taps-outermost measured 3.07 GB of
// fabric reads per launch for 0.39 GB of activations (rocprofv3 FETCH_SIZE x 2, profiles/r02q_pmc_step.json).
__device__ __forceinline__ void x3r_issue_conv(const float* const (&rowp)[2], const int (&ok)[2], int tap, int c0, int W,
                                               int64_t ld, char* img, int wave, int lane) {
    const int64_t shift = (int64_t)((tap / 3 - 1) * W + (tap % 3 - 1)) * ld + c0;      // ld = pixel pitch (>= channels)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = wave * 2 + i;
        const int row = 16 * q + (lane >> 2), g = (lane & 3) ^ ((row >> 2) & 3);
        const float* src = ((ok[i] >> tap) & 1) ? rowp[i] + shift + 4 * g : x3_zero;
        __builtin_amdgcn_global_load_lds((x3_glb_ptr)src, (x3_lds_ptr)(img + q * 1024), 16, 0, 0);
    }
}

// Weight-gradient flavour (cv_wgrad): the x-contiguous B image of a stage is 16 consecutive pixels p of the tap-shifted
// activations, B(p, n) = X[p + (dy, dx)][n]; rows whose neighbour falls outside the picture (or p >= kend) read zero.
// (y, x) = the lane's two pixels of the current stage; W >= 16, so one stage wraps at most one image row.
__device__ __forceinline__ void x3r_issue_convw(const float* __restrict__ X, int64_t C, int n0, int N, int k0, int kend,
                                                const int (&py)[2], const int (&px)[2], int dy, int dx, int H, int W,
                                                char* img, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = wave * 2 + i;
        const int kr = 2 * q + (lane >> 5), xx = n0 + 4 * (lane & 31), k = k0 + kr;
        const bool ok = k < kend && xx < N && (unsigned)(py[i] + dy) < (unsigned)H && (unsigned)(px[i] + dx) < (unsigned)W;
        const float* src = ok ? X + ((int64_t)k + dy * W + dx) * C + xx : x3_zero;
        __builtin_amdgcn_global_load_lds((x3_glb_ptr)src, (x3_lds_ptr)(img + q * 1024), 16, 0, 0);
    }
}

// ---- packed-B kernels: gemm_x3p_kernel (bf16x3, gt_gemm_x3.hip) and gemm_x3h_kernel (f16x2, gt_gemm_x3p.hip) -------------------
constexpr int X3P_R = 4;                          // A-ring depth of the packed-B kernel (stages of 8 KB)
// Body of a family's launcher: starts the instance KERNEL<LA, HN, CV, BN> that pick k names; every instance is named, and so
// instantiated, here, in the order the kernels have always been emitted in.
#define X3P_CASE(KERNEL, la, hn, cv, bn)                                                                               \
    if (k.LA == la && k.HN == hn && k.CV == cv && k.BN == bn) {                                                        \
        hipLaunchKernelGGL((KERNEL<la, hn, cv, bn>), grid, dim3(256), 0, st, p);                                       \
        GT_LAUNCH_CHECK();                                                                                             \
        return 0;                                                                                                      \
    }
#define X3P_LAUNCH_PICK(KERNEL)                                                                                        \
    X3P_CASE(KERNEL, 0, 0, 1, 64) X3P_CASE(KERNEL, 0, 0, 0, 64) X3P_CASE(KERNEL, 0, 0, 1, 128)                         \
    X3P_CASE(KERNEL, 0, 16, 0, 128) X3P_CASE(KERNEL, 0, 32, 0, 128) X3P_CASE(KERNEL, 0, 64, 0, 128)                    \
    X3P_CASE(KERNEL, 0, 0, 0, 128) X3P_CASE(KERNEL, 1, 0, 0, 128)                                                      \
    return GT_ENOTSUP;

}  // namespace gt
