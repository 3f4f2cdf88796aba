/*
 * gt_hip.h -- C ABI of libgt_hip.so: the MI355X (gfx950) device path for the Galerkin /
 * Fourier simple-attention encoder layer and the spectral-convolution decoder.
 *
 * Boundary contract
 *   - plain C: device pointers, sizes, POD descriptors; no torch / C++ types.
 *   - every entry point enqueues work on `stream` (a hipStream_t passed as void*) and
 *     returns immediately; no hidden synchronisation, no allocation (graph-capturable).
 *     Scratch memory is supplied by the caller (`ws`, `ws_bytes`).
 *   - all tensors are fp32, row-major, device-resident.
 *   - return value: 0 = success, >0 = hipError_t from the launch, <0 = GT_E* argument error.
 *
 * The reference (scaomath/galerkin-transformer) has no FFI of its own: its hot path is a chain
 * of ATen calls issued from Python.  Each entry point below names the reference call site(s)
 * (file:line under /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 */
#ifndef GT_HIP_H
#define GT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GT_ABI_VERSION 21

/* argument errors */
#define GT_EINVAL   (-1)   /* bad shape / flag combination            */
#define GT_EALIGN   (-2)   /* pointer or leading dimension misaligned */
#define GT_EWS      (-3)   /* scratch buffer too small                */
#define GT_ENOTSUP  (-4)   /* combination not implemented             */

/* activations */
#define GT_ACT_NONE 0
#define GT_ACT_RELU 1
#define GT_ACT_SILU 2
#define GT_ACT_GELU 3   /* erf GELU; gt_dropact_fwd / gt_dropact_bwd only (every other entry point: GT_EINVAL) */
#define GT_ACT_DROP_SILU 4   /* gt_gemm only: the dropout sits in FRONT of the SiLU -- Conv2dResBlock's conv -> dropout -> activation
                                (layers.py:139-149) with a non-ReLU activation, where the two do not commute:
                                    u = keepscale(m, n) * v;   result = silu(u);   pre[m][n] (optional) = keepscale(m, n) * silu'(u)
                                `drop` is consumed here (not applied again behind the activation), and `pre` receives the factor the
                                backward multiplies the output gradient with (GT_AUX_MUL) instead of the pre-activation */

#define GT_ACT_SILU2 5       /* gt_gemm only (ABI v21): two SiLUs in a row -- Interp2dUpsample's conv block -> activation -> activation
                                (layers.py:642-650: Conv2dResBlock's own activation, then the up-scaler's) when its dropouts are off:
                                    result = silu(silu(v));   pre[m][n] (optional) = silu'(v) * silu'(silu(v))
                                `pre` is again the factor of the backward (GT_AUX_MUL on the product that forms the result's
                                gradient); `drop` must be NULL / p = 0 (GT_EINVAL) */

/* gt_gemm_desc.aux_op: multiply the result by a function of aux[m][n] */
#define GT_AUX_NONE      0
#define GT_AUX_GT0       1   /* v *= (aux > 0) ? aux_scale : 0      (ReLU' with the dropout scale folded in) */
#define GT_AUX_DSILU     2   /* v *= d/dx silu(aux)                 (aux = saved pre-activation)             */
#define GT_AUX_MUL       3   /* v *= aux * aux_scale                (explicit multiplicative mask replay)    */

int gt_abi_version(void);
/* Name of the code object's target ("gfx950").  Does not touch the device. */
const char* gt_target_arch(void);

/* ---------------------------------------------------------------------------------------------
 * Stateless dropout.  keep(idx) = hash(seed[0], salt, idx) >= p*2^32, scale 1/(1-p).  `seed`
 * is a DEVICE pointer to one uint64 so a captured graph replays with fresh masks after the
 * host bumps it (gt_seed_advance).  The same (seed, salt, idx) regenerates the mask in backward.
 * Replaces F.dropout / nn.Dropout at layers.py:701,731,981 and model.py:125,132.
 * ------------------------------------------------------------------------------------------- */
typedef struct gt_dropout {
    float p;                    /* 0 => disabled                                   */
    uint32_t salt;              /* distinguishes call sites                        */
    const uint64_t* seed;       /* device pointer, may be NULL iff p == 0          */
} gt_dropout;

/* seed[0] += inc  (one tiny kernel; capturable) */
int gt_seed_advance(uint64_t* seed, uint64_t inc, void* stream);
/* out[i] = x[i] * keepscale(i)   -- standalone elementwise dropout, n elements, used by tests */
int gt_dropout_apply(const float* x, float* out, int64_t n, const gt_dropout* d, void* stream);

/* y[i] = act2(drop2(act1(drop1(x[i]))))  in one elementwise pass (mask index = i, the index gt_dropout_apply uses;
 * d1 / d2 may be NULL or p = 0, act* = GT_ACT_*): the tail of Conv2dResBlock (layers.py:88-150) and of
 * Interp2dUpsample's conv branch (layers.py:658-668).  Backward recomputes from x:  gx[i] = gy[i] * dy/dx. */
int gt_dropact_fwd(const float* x, float* y, int64_t n, const gt_dropout* d1, int32_t act1, const gt_dropout* d2,
                   int32_t act2, void* stream);
int gt_dropact_bwd(const float* x, const float* gy, float* gx, int64_t n, const gt_dropout* d1, int32_t act1,
                   const gt_dropout* d2, int32_t act2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched fp32 GEMM on the MFMA pipe (v_mfma_f32_16x16x4_f32) with fused prologue/epilogue.
 *
 *   for z = (b0, b1) in [0,batch0) x [0,batch1):
 *     acc[m][n] = sum_k  A_z(m,k) * keepA(m,k) * B_z(k,n)
 *     v   = alpha*acc + bias[n] + sum_{j<rp} rp_a[m][j]*rp_b[n][j] + add_z[m][n]
 *     pre[m][n] = v                                  (optional)
 *     v   = act(v) ;  v *= f(aux[m][n]) ;  v = dropout(v)          (act = GT_ACT_DROP_SILU: see there)
 *     C_z[m][n] = res_z[m][n] + out_scale*v          (res optional)
 *
 *   layout_a = 0 : A(m,k) = A[m*lda + k]     (k contiguous; activations [tokens, features])
 *   layout_a = 1 : A(m,k) = A[k*lda + m]     (m contiguous; transposed use, reduction over rows)
 *   layout_b = 0 : B(k,n) = B[n*ldb + k]     (nn.Linear weight [out, in])
 *   layout_b = 1 : B(k,n) = B[k*ldb + n]
 *
 * Replaces every nn.Linear / torch.matmul / einsum contraction on the path:
 *   layers.py:837-839 (QKV), :723,:733 (K^T V, Q M), :687,:703 (Q K^T, S V), :897 (fc),
 *   :979-987 (FFN), :1087-1098 / :1172-1189 (truncated DFT stages), model.py:615-629, and the
 *   autograd backward of each (addmm / bmm backward = the transposed layouts).
 *
 * split_k: 0 = let the library decide, 1 = never split, >1 = that many K-slices (reduced in a
 * second deterministic pass; only alpha is allowed as epilogue then).  ws/ws_bytes: scratch for
 * the slabs (gt_gemm_ws_bytes gives an upper bound).
 * ------------------------------------------------------------------------------------------- */
typedef struct gt_gemm_desc {
    int32_t M, N, K;
    int32_t layout_a, layout_b;
    int32_t batch0, batch1;
    int32_t split_k;

    const float* A; int64_t lda, a_bs0, a_bs1;
    const float* B; int64_t ldb, b_bs0, b_bs1;
    float*       C; int64_t ldc, c_bs0, c_bs1;

    /* prologue: stateless dropout mask on A.  The mask index of A's element (outer, inner) is
       z*a_drop_bstride + outer*a_drop_ld + inner  (outer = the lda-strided index).          */
    gt_dropout a_drop; float a_drop_sign; int64_t a_drop_ld, a_drop_bstride;
    /* optional by-product (layout_a = 1 only): a_colsum[m] = sum over batch and k of A_z(m,k)*keepA(m,k),
       i.e. the column sums of the [K, M] tensor behind A -- the bias gradient that goes with a weight
       gradient (autograd of nn.Linear: layers.py:811,823,964,976).  Deterministic (per-slice partials in
       `ws`, reduced in a fixed order). */
    float* a_colsum;

    /* epilogue */
    float alpha;
    const float* bias;
    int32_t rp; const float* rp_a; int64_t rp_lda, rp_a_bs0; const float* rp_b; int64_t rp_ldb;
    const float* add; int64_t ldadd, add_bs0, add_bs1;   /* full-matrix addend before the activation */
    float* pre; int64_t ldpre;                  /* batch strides = c_bs0/c_bs1 scaled by ldpre/ldc is NOT assumed: dense [batch][M][ldpre] */
    int32_t act;
    int32_t aux_op; const float* aux; int64_t ldaux, aux_bs0, aux_bs1; float aux_scale;
    gt_dropout drop;                            /* mask index = (z*M + m)*N + n */
    const float* res; int64_t ldr, r_bs0, r_bs1;
    float out_scale;

    /* Fused two-layer pointwise head  y = W2 act(W1 x + b1) + b2  with a narrow second layer (n_out <= 4):
     * SpectralRegressor / PointwiseRegressor tail, model.py:575-580, 625-629.  Needs N <= 128 (one tile
     * column), no batching, no split-K; of the epilogue fields above only alpha, bias and act are honoured.
     *   GT_EP_ROWDOT  : out2[m][o] = sum_n act(alpha*acc + bias)[m][n] * w2[o*ldw2 + n] + b2[o];  C is NOT
     *                   written -- the [M, N] hidden activation never reaches HBM.
     *   GT_EP_MLP_BWD : h = alpha*acc + bias is the recomputed pre-activation;
     *                   C[m][n] = (sum_o g2[m][o] * w2[o*ldw2 + n]) * act'(h[m][n])       (= dL/dh)
     *                   dw2[o][n] = sum_m g2[m][o] * act(h[m][n])                          (by-product)   */
    int32_t ep_mode, n_out;
    const float* w2; int64_t ldw2;
    const float* b2;        /* ROWDOT: [n_out] or NULL */
    float* out2;            /* ROWDOT: [M, n_out] */
    const float* g2;        /* MLP_BWD: [M, n_out] */
    float* dw2;             /* MLP_BWD: [n_out, N] (row stride N) */

    /* Optional second product accumulated into the same tile before the epilogue:
     *     acc += sum_{k < K2} A2_z(m,k) * B2_z(k,n)          (same layout_a / layout_b as the first product)
     * SpectralConv's  act(irfft-stage(Z) + Linear(x))  (layers.py:1172-1189, 1087-1098) becomes one launch:
     * first product = c2r DFT stage, second = the residual Linear on the block's own input rows; likewise
     * its backward  dx = rfft-stage^T(dX1) + dpre W.  No split-K, no A dropout, v1 kernel only. */
    int32_t K2;
    const float* A2; int64_t lda2, a2_bs0, a2_bs1;
    const float* B2; int64_t ldb2, b2_bs0, b2_bs1;

    /* GT_EP_HEADNORM: the packed QKV projection (layers.py:838-840) with the per-head LayerNorm + position columns of
     * gt_headnorm_fwd (layers.py:841-874) fused behind it.  C [M, N = 3*h*dk] is written as usual (the backward reads
     * the raw projection) and in the same pass every row's head segments go to hn_out [3][M][h][DP] (normalised where
     * hn_norm_mask says so, coordinates in columns [0, hn_p), zero pad) and hn_stats [#normed][M][h][2] = (mean,
     * rstd).  Runs on the split-operand ring kernel only (precision != GT_PREC_F32, 16-byte aligned operands,
     * K % 4 == 0): dk in {16, 32, 64}, hn_p <= 4, layout_a = layout_b = 0, no batching, no split-K, no other epilogue field but
     * alpha and bias; anything else returns GT_ENOTSUP and the caller runs gt_gemm + gt_headnorm_fwd. */
    const float* hn_gamma; const float* hn_beta; const float* hn_pos;
    float* hn_out; float* hn_stats;
    int32_t hn_h, hn_dk, hn_p, hn_norm_mask;
    float hn_eps;

    /* Arithmetic of the contraction (GT_PREC_*).  Operands, accumulator and result are fp32 in every mode; what
     * changes is the MFMA instruction the products run on:
     *   GT_PREC_F32    v_mfma_f32_16x16x4_f32, bit-for-bit an fp32 FMA chain (157 TFLOP/s peak);
     *   GT_PREC_BF16X3 every operand value is split exactly into three bf16 terms while it is staged
     *                  (a = h0 + h1 + h2 to 2^-24) and the six plane products down to 2^-16 are accumulated on
     *                  v_mfma_f32_32x32x16_bf16 in fp32: same rounding class as GT_PREC_F32 (the 1e-5 parity gate
     *                  holds), 16/6 of its matrix rate;
     *   GT_PREC_BF16X2 two terms / three products (~2^-16 relative);
     *   GT_PREC_BF16   operands rounded to bf16, one product: throughput mode with its own (3e-3) gate;
     *   GT_PREC_F16X2  every operand value is split into TWO fp16 terms (11 + 11 significand bits) after scaling by a
     *                  power of two that tracks the data (weights: per 32-column tile when they are packed; activation rows:
     *                  a running per-row exponent inside the kernel, the accumulator rescaled when it has to drop), three
     *                  products on v_mfma_f32_32x32x16_f16: fp32-class results at half the matrix work of GT_PREC_BF16X3.
     *                  Implemented by the packed-B kernels (a weight against >= 16384 token rows, the implicit
     *                  convolutions); every other launch of this mode runs GT_PREC_BF16X3.
     * The split kernel serves the plain-epilogue products with M, N >= 96 (whole 128 x 128 tiles); everything else
     * (fused heads, head-norm epilogue, narrow or tiny problems, the tall-skinny path) stays on the fp32 pipe in
     * every mode. */
    int32_t precision;

    /* Implicit 3x3 convolution (stride 1, zero padding 1) on channels-last activations: cv_c > 0 makes A a
     * [B, cv_h, cv_w, cv_c] image, M = B*cv_h*cv_w its pixels, K = 9*cv_c, and the contraction index
     *     k = (c / CB) * 9*CB + tap * CB + (c % CB),      CB = 32 if cv_c % 32 == 0 else 16,  tap = 3*(dy+1) + (dx+1)
     * reads A[pixel + (dy, dx)][c] (zero outside the image) -- the im2col matrix is never written; the nine taps of a
     * channel block are adjacent in k so that they hit the same cache lines back to back.  B is the filter as
     * [N][9*cv_c] in that k order (layout_b = 0): an nn.Conv2d weight [N][c][3][3] -> [N][c/CB][tap][CB]
     * for the forward product (layers.py:98-100 `nn.Conv2d(.., kernel_size=3, padding=1, bias=False)` of the scaler
     * blocks), or the tap-reversed, in/out-swapped filter for the data gradient.  Split-operand ring kernel only:
     * precision != GT_PREC_F32, layout_a = layout_b = 0, cv_c % 16 == 0, no batching, no split-K, no A dropout,
     * M, N >= 96 (N >= 32 with M >= 16384: narrow outputs run on 128 x 64 tiles of the packed-B kernel); anything else
     * returns GT_ENOTSUP (the caller then uses its library convolution).  lda > cv_c is the pixel pitch of the image:
     * the convolution then reads the cv_c-channel column slice A .. A + cv_c of a wider channels-last buffer in place
     * (lda % 4 == 0); the weight-gradient form takes ldb the same way.
     *
     * cv_wgrad != 0 selects the weight gradient of the same convolution instead:
     *     C_tap[m][n] = sum_pixels A[pixel][m] * X[pixel + (dy, dx)][n]          tap = 0..8 = the batch index
     * with A = the output gradient [pixels, M] (layout_a = 1, lda = M's row length), B = X the channels-last input
     * [B, cv_h, cv_w, cv_c] (layout_b = 1, N = cv_c), K = the pixel count, batch0 = 9, batch1 = 1, C = [9][M][N]
     * (c_bs0 = the tap stride), split_k = 0 (the library cuts K into chunks; the nine taps of a chunk run next to each
     * other on one XCD and share its L2).  cv_w >= 16, no epilogue fields. */
    int32_t cv_h, cv_w, cv_c, cv_wgrad;

    /* GT_EP_HEADNORM: streams (bit 0 Q, 1 K, 2 V) whose RAW projection is NOT written to C.  The backward needs the raw
     * rows of the normalised streams only (LayerNorm backward); a training forward passes ~hn_norm_mask & 7 and saves
     * a third of C's write traffic.  Zero (the default) writes all of C. */
    int32_t hn_skip_raw_mask;

    /* GT_EP_HEADNORM, hn_plain != 0: the head tiles of the normalised streams hold the normalised values WITHOUT the
     * LayerNorm affine (xh = (x - mean) * rstd); gamma and beta are applied by the consumers (gt_galerkin_ktv_affine
     * on load, gt_galerkin_dkv_ln_plain folded into dM), whose LayerNorm backward then needs no raw projection at all:
     * with hn_skip_raw_mask = 7 the launch writes nothing to C and C may be NULL. */
    int32_t hn_plain;

    /* Pre-packed B (round 5, ABI v19): NULL, or the buffer gt_gemm_pack_b_many filled for exactly this product (same B,
     * layout_b, ldb, N, K, precision = GT_PREC_F16X2) since B last changed -- gt_gemm then skips its own pack launch and
     * needs no workspace.  Only where gt_gemm_packed_b_bytes(d) > 0. */
    const void* b_packed;

    /* Second output (ABI v20, round 6): c_masked[m][n] = C[m][n] * keepscale_{c_mask}(m, n)  -- the finished result once more
     * under a stateless dropout mask (index (z*M + m)*N + n, the index gt_dropout_apply uses on the dense [M, N] tensor), row
     * pitch ldc_masked.  The data gradient a layer hands to the layer in front of it is needed twice there: as it is (residual
     * branch) and under that layer's output-dropout mask (nn.Dropout of model.py:125,132 backwards: it feeds three
     * contractions) -- the product that computes it writes both and the elementwise gt_dropout_apply pass between two layers'
     * backward passes disappears.  No batching, no split-K, GT_EP_NORMAL only; NULL = off. */
    float* c_masked; int64_t ldc_masked;
    gt_dropout c_mask;
} gt_gemm_desc;

#define GT_PREC_F32    0
#define GT_PREC_BF16X3 1
#define GT_PREC_BF16X2 2
#define GT_PREC_BF16   3
#define GT_PREC_F16X2  4

#define GT_EP_NORMAL  0
#define GT_EP_ROWDOT  1
#define GT_EP_MLP_BWD 2
#define GT_EP_HEADNORM 3

void    gt_gemm_desc_init(gt_gemm_desc* d);            /* zero + alpha=1, out_scale=1, batch=1 */
int64_t gt_gemm_ws_bytes(const gt_gemm_desc* d);
int     gt_gemm(const gt_gemm_desc* d, void* ws, int64_t ws_bytes, void* stream);
/* Weights packed ahead, all in one launch (the model-API counterpart of "one pack launch per step": every nn.Linear weight of
 * layers.py:811,823,964,976 feeds 2 token products per step).  gt_gemm_packed_b_bytes: size of d's packed weight if gt_gemm(d)
 * is a single packed-B launch, else 0.  gt_gemm_pack_b_many: descs[i].B -> outs[i] for n <= 64 products (GT_PREC_F16X2). */
int64_t gt_gemm_packed_b_bytes(const gt_gemm_desc* d);
int     gt_gemm_pack_b_many(const gt_gemm_desc* descs, void* const* outs, int32_t n, void* stream);
/* debugging/tests: which tile configuration and split the library picks */
int     gt_gemm_plan(const gt_gemm_desc* d, int32_t* bm, int32_t* bn, int32_t* split);
/* symbol of the kernel instance gt_gemm would launch for d, as a profiler prints it */
int     gt_gemm_kernel_name(const gt_gemm_desc* d, char* buf, int32_t n);

/* ---------------------------------------------------------------------------------------------
 * Fused FeedForward forward (ABI v20, round 6; layers.py:979-987 with the residual of model.py:131-132) in GT_PREC_F16X2:
 *     hid[t][:] = dropout_h( act( x[t] W1^T + b1 ) )             [T, f]  written to HBM (the backward reads it)
 *     out[t][:] = res[t] + dropout_o( hid[t] W2^T + b2 )         [T, d]  (res may be NULL)
 * in ONE launch: a block owns 64 token rows and keeps their hidden tile in LDS between the two contractions, so the hidden
 * activation is never read back in the forward.  The arithmetic of the two gt_gemm launches it replaces (same packed
 * planes, same product order, same dropout indices t*f + j / t*d + c): bit-identical results with GT_FFN_PRESPLIT=0 (same
 * running exponents too; no decision bits), within about 5e-7 of them in the default pre-split form.  x [T, d], W1 [f, d], W2 [d, f] dense fp32, 16-byte aligned; act = GT_ACT_RELU | GT_ACT_NONE.
 * w1_packed / w2_packed: both NULL (the call packs the weights into ws, gt_ffn_fwd_ws_bytes) or the buffers
 * gt_gemm_pack_b_many filled for the products [T, d] x W1^T and [T, f] x W2^T (gt_gemm_desc.b_packed of those).
 * Implemented for d = 128, f = 256, T >= 16384 (else GT_ENOTSUP: two gt_gemm launches do the same).
 * ------------------------------------------------------------------------------------------- */
int64_t gt_ffn_fwd_ws_bytes(int64_t T, int32_t d, int32_t f);
int gt_ffn_fwd(const float* x, int64_t T, int32_t d, int32_t f, const float* W1, const float* b1, const float* W2,
               const float* b2, const float* res, const gt_dropout* drop_h, const gt_dropout* drop_o, int32_t act,
               float* hid, float* out, void* relu_bits, const void* w1_packed, const void* w2_packed, void* ws,
               int64_t ws_bytes, void* stream);
/* relu_bits (optional, gt_ffn_bits_bytes(T) bytes, 16-byte aligned): one bit per hidden value -- kept by the dropout AND
 * positive -- in the kernel's own register layout (opaque to the caller), for gt_ffn_bwd.
 *
 * The data half of the backward (autograd of the above, nn.Linear / ReLU / nn.Dropout backwards) in the same geometry:
 *     gh[t][:] = (gm[t] W2) .* bits .* hid_scale          [T, f]  written to HBM (dW1 = gh^T x needs it)
 *     dx[t][:] = res[t] + gh[t] W1                        [T, d]  (res = the unmasked incoming gradient of a residual layer, or NULL)
 *     dx_masked = dx .* keepscale_{mask2}                 optional second output (gt_gemm_desc.c_masked's twin)
 * gm = the incoming gradient under the output-dropout mask; hid_scale = 1 / (1 - p_h).  The hidden activation itself is not
 * read (its 242 MB at B = 128 were re-read as a 1-bit decision by the unfused hidden-gradient launch).  w2_packed / w1_packed:
 * the packs of the products [T, d] x W2 (layout_b = 1, N = f) and [T, f] x W1 (layout_b = 1, N = d), or both NULL + ws
 * (gt_ffn_fwd_ws_bytes).  Same shapes as gt_ffn_fwd, else GT_ENOTSUP. */
int64_t gt_ffn_bits_bytes(int64_t T);
int gt_ffn_bwd(const float* gm, int64_t T, int32_t d, int32_t f, const float* W2, const float* W1, const void* relu_bits,
               float hid_scale, const float* res, float* gh, float* dx, float* dx_masked, const gt_dropout* mask2,
               const void* w2_packed, const void* w1_packed, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * out[n] (+)= sum_m A[m*lda + n] * keepA(m,n)  -- bias gradients.  Two deterministic passes.
 * ------------------------------------------------------------------------------------------- */
int gt_colsum(const float* A, int64_t lda, int32_t M, int32_t N, const gt_dropout* a_drop,
              float a_sign, float* out, void* ws, int64_t ws_bytes, void* stream);
/* dpre[i] = dout[i] * act'(pre[i])   (GT_ACT_*), n elements */
int gt_act_bwd(const float* dout, const float* pre, float* dpre, int64_t n, int32_t act, void* stream);
/* out[i] = alpha * sum_s slabs[s*stride + i], i < n */
int gt_slab_reduce(const float* slabs, int64_t stride, int32_t n_slabs, int64_t n, float alpha,
                   float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-head LayerNorm + position concat (layers.py:841-874).
 *   qkv   [T, 3*d]   raw projections (T = B*n tokens), d = h*dk
 *   pos   [T, p]     coordinates (p may be 0 -> pos may be NULL)
 *   gamma/beta [2][h][dk]: affine of the two normalised streams, in stream order
 *   norm_mask: bit s set => stream s (0=Q,1=K,2=V) is normalised (galerkin: K,V = 6; fourier:
 *              Q,K = 3; no attn norm: 0)
 *   out   [3][T][h][DP]  with DP = round_up(dk+p, 4); columns [0,p) = pos, [p,p+dk) = values,
 *                        rest zero.  stats [2][T][h][2] = (mean, rstd) of the normalised streams.
 * Backward: d_out -> d_qkv [T,3d], dgamma/dbeta [2][h][dk] (deterministic two-pass); with norm_mask != 0 both slots
 *   are written, a slot with no stream as zero; with norm_mask == 0 neither is touched and qkv is not read.
 * dk % 4 == 0 with 16-byte aligned operands and 3 * h * pow2(dk / 4) <= 1024 runs the three streams in one launch;
 * anything else runs the gt_headtile_* kernels below once per stream, within their limits: dk <= 256 and
 * h * pow2(ceil(dk / 4)) <= 1024, else GT_ENOTSUP.
 * ------------------------------------------------------------------------------------------- */
int gt_headnorm_fwd(const float* qkv, const float* pos, const float* gamma, const float* beta,
                    int32_t T, int32_t h, int32_t dk, int32_t p, int32_t norm_mask, float eps,
                    float* out, float* stats, void* stream);
int gt_headnorm_bwd(const float* d_out, const float* qkv, const float* gamma, const float* stats,
                    int32_t T, int32_t h, int32_t dk, int32_t p, int32_t norm_mask,
                    float* d_qkv, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes,
                    void* stream);
int64_t gt_headnorm_bwd_ws_bytes(int32_t T, int32_t h, int32_t dk);
/* ABI v21, additive: the same for ONE stream with its own row count (cross-attention, where the query rows and the key /
 * value rows differ).  X [T][ldx]: the h*dk value columns of one projection, e.g. the K or the V column block of a packed
 * [T_kv][2d] product (ldx >= h*dk).  gamma, beta [h][dk]; gamma == NULL: no norm -- copy, coordinates and zero pad, stats
 * untouched.  out [T][h][DP], stats [T][h][2] = (mean, rstd).  Backward: dX [T][lddx] receives the value columns only (the
 * rest of a wider row is left alone); dgamma, dbeta [h][dk] through per-block partials in ws summed in block order
 * (deterministic).  With gamma == NULL the backward is the scatter alone and X, stats, dgamma, dbeta, ws may be NULL.
 * dk % 4 == 0 with ldx, lddx % 4 == 0 and 16-byte aligned operands moves float4; anything else runs the same kernels on
 * scalars.  dk <= 256 and h * pow2(ceil(dk / 4)) <= 1024, else GT_ENOTSUP. */
int gt_headtile_fwd(const float* X, int64_t ldx, const float* pos, const float* gamma, const float* beta, int32_t T,
                    int32_t h, int32_t dk, int32_t p, float eps, float* out, float* stats, void* stream);
int64_t gt_headtile_bwd_ws_bytes(int32_t T, int32_t h, int32_t dk);
int gt_headtile_bwd(const float* d_out, const float* X, int64_t ldx, const float* gamma, const float* stats, int32_t T,
                    int32_t h, int32_t dk, int32_t p, float* dX, int64_t lddx, float* dgamma, float* dbeta, void* ws,
                    int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Galerkin attention core, small-matrix stage (layers.py:723-733 + :897 folded):
 *   Mt[b,h]   = mask .* ( sum_s slabs[s][b,h] ) / n          (DPxDP, the "attn_weight")
 *   P[b][h*DP + j][c] = sum_e Mt[b,h][j][e] * Wfc[c][h*Dr + e]    (Dr = dk+p unpadded)
 * so that   attn_out[b] = [Q'](n x h*DP) @ P[b]  is one GEMM.  mask: explicit tensor
 * [B,h,DP,DP] of multipliers (replay mode), or NULL with drop.p (0.5 in the reference) for the
 * stateless RNG, or both NULL/0 for identity.
 * Backward: from dPt[b][c][h*DP+j] (= d attn_out^T Q') produce
 *   dM[b,h]  = mask .* (dP_h Wfc_h) / n        and      dWfc slabs [B][d][h*Dr].
 * ------------------------------------------------------------------------------------------- */
/* K'^T V' (layers.py:723) as a streaming kernel on the head-tile layout [B*n][h][DP] (what
 * gt_headnorm_fwd writes): token rows go from HBM straight into MFMA operand registers, the dk x dk core
 * accumulates on the matrix pipe and the p-wide coordinate borders on the VALU.  Writes n_slabs partial
 * [B,h,DP,DP] slabs (token chunks) that gt_galerkin_finalize_fwd sums.  dk % 16 == 0, dk <= 96, p <= 2
 * (else GT_ENOTSUP: use gt_gemm).  gt_galerkin_ktv_slabs suggests n_slabs.
 * Chunks: chunk = round4(ceil(n / n_slabs)); slab q [n_slabs][B][h][DP][DP] sums the tokens
 * [q chunk, min(n, (q + 1) chunk)) of its sample -- a chunk is in general no multiple of the kernels' 16-token tile -- and
 * a chunk that starts at or past n is an all-zero slab.
 * Slab = [pos | K']^T [pos | V'] on the leading Dr = dk + p rows and columns, exact zeros behind them.  The coordinates
 * of BOTH operands are read from the K tile (columns 0..p-1 of Kp); the coordinate columns of Vp are not read. */
int32_t gt_galerkin_ktv_slabs(int32_t B, int32_t n);
int gt_galerkin_ktv(const float* Kp, const float* Vp, int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p,
                    float* slabs, int32_t n_slabs, void* stream);
/* The same for "plain" head tiles (gt_gemm_desc.hn_plain): K' = gamma_K xh + beta_K, V' likewise, formed while the
 * operands are loaded; gamma, beta [2][h][dk] (K then V).  NULL gamma / beta = gt_galerkin_ktv. */
int gt_galerkin_ktv_affine(const float* Kp, const float* Vp, const float* gamma, const float* beta, int32_t B, int32_t n,
                           int32_t h, int32_t dk, int32_t p, float* slabs, int32_t n_slabs, void* stream);
int gt_galerkin_finalize_fwd(const float* slabs, int32_t n_slabs, int64_t slab_stride,
                             int32_t B, int32_t h, int32_t DP, int32_t Dr, int32_t d, int32_t n_tokens,
                             const float* mask, const gt_dropout* drop, const float* Wfc,
                             float* Mt, float* P, float* Pv, int32_t pos_dim, void* stream);
/* (Pv, optional: the value rows pos_dim .. Dr-1 of every head's block of P once more, compact [B][h (Dr - pos_dim)][d] --
 * the B operand of the backward's dQ product.) */
int gt_galerkin_finalize_bwd(const float* dPt, const float* Mt, const float* mask,
                             const gt_dropout* drop, const float* Wfc,
                             int32_t B, int32_t h, int32_t DP, int32_t Dr, int32_t d, int32_t n_tokens,
                             float* dM, float* dWfc_slabs, void* stream);

/* dK'[t] = V'[t] dM^T,  dV'[t] = K'[t] dM  for every token of every (batch, head): the backward of
 * M = K'^T V' (layers.py:723) as one streaming pass over the head tiles [B*n][h][DP] (dM [B,h,DP,DP]).
 * DP in {20, 36, 52}, else GT_ENOTSUP (two batched gt_gemm launches do the same). */
int gt_galerkin_dkv(const float* Kp, const float* Vp, const float* dM, float* dKp, float* dVp, int32_t B,
                    int32_t n, int32_t h, int32_t DP, void* stream);

/* The same two products with the per-head LayerNorm backward of gt_headnorm_bwd (norm_mask = K and V, layers.py:841-874
 * backwards) applied on the way out: dK', dV' are never written.  Writes all three blocks of d_qkv [B*n][3 h dk] (K, V:
 * LayerNorm backward of the products; Q: dQp [B*n][h][DP] with its coordinate / pad columns dropped -- or, with
 * dQp = NULL, left to the caller, whose dQ product can write the value columns straight into the Q block) and
 * dgamma / dbeta [2][h][dk] (K then V).  qkv = the raw projection, gamma [2][h][dk], stats [2][B*n][h][2] as
 * gt_headnorm_fwd left them.  DP = round4(dk + p) in {20, 36, 52} and dk % 4 == 0, else GT_ENOTSUP (gt_galerkin_dkv +
 * gt_headnorm_bwd do the same in two passes). */
int64_t gt_galerkin_dkv_ln_ws_bytes(int32_t B, int32_t h, int32_t dk);
int gt_galerkin_dkv_ln(const float* Kp, const float* Vp, const float* dM, const float* dQp, const float* qkv,
                       const float* gamma, const float* stats, int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p,
                       float* d_qkv, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, void* stream);
/* The same on "plain" head tiles: beta [2][h][dk] given, qkv unused (may be NULL); gamma moves onto the rows of dM, beta dM
 * is added to the products, the tiles themselves are the xh of the LayerNorm backward. */
int gt_galerkin_dkv_ln_plain(const float* Kp, const float* Vp, const float* dM, const float* dQp, const float* qkv,
                             const float* gamma, const float* beta, const float* stats, int32_t B, int32_t n, int32_t h,
                             int32_t dk, int32_t p, float* d_qkv, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * The softmax pair of the 'linear' / 'global' attention family (layers.py:719-722; ABI v21, additive):
 *     Q~ = softmax(Q', dim=-1)  over the Dr = dk + p columns of every (token, head)      -- "feature" softmax
 *     K~ = softmax(K', dim=-2)  over the n tokens of every (batch, head, column < Dr)    -- "token" softmax
 * on the head-tile layout [B*n][h][DP], DP = round4(Dr), that gt_headnorm_fwd writes.  The coordinate columns take part,
 * the pad columns Dr..DP-1 do not and are written as exact zeros.  The rest of the family is the Galerkin path on
 * (Q~, K~, V'): gt_galerkin_ktv, the finalize pair, the Q~ P product, gt_galerkin_dkv.
 *     feature softmax: rows = B*n*h segments of DP floats; one pass forward, one backward
 *                      dX = Y .* (dY - sum_c Y .* dY)   from the OUTPUT Y (Q' is not needed)
 *     token softmax:   a statistics pass (running max / sum per column and chunk of 128 tokens, partials in ws) and an
 *                      applying pass that merges the partials in a fixed order; the backward likewise:
 *                      c = sum_t Y .* dY per column,  dX = Y .* (dY - c).   ws >= the ws_bytes query.
 * The row maximum is subtracted before every exponential; no atomics: results are bit-identical from run to run.
 * In place is allowed (Y == X; dX == dY).  fp32 in every precision mode.
 * dk in {16, 32, 48, 64, 96} and p in {0, 1, 2} (the head tiles of the Galerkin path), any n >= 1; else GT_ENOTSUP.
 * ------------------------------------------------------------------------------------------- */
int gt_feature_softmax_fwd(const float* X, float* Y, int64_t rows, int32_t dk, int32_t p, void* stream);
int gt_feature_softmax_bwd(const float* Y, const float* dY, float* dX, int64_t rows, int32_t dk, int32_t p,
                           void* stream);
int64_t gt_token_softmax_ws_bytes(int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p);
int gt_token_softmax_fwd(const float* X, float* Y, int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p,
                         void* ws, int64_t ws_bytes, void* stream);
int gt_token_softmax_bwd(const float* Y, const float* dY, float* dX, int32_t B, int32_t n, int32_t h, int32_t dk,
                         int32_t p, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token-axis ("instance") norm of a K or V head tile: norm_type='instance' of the Galerkin family (layers.py:842-854,
 * nn.InstanceNorm1d(d_k, affine=True) per head; ABI v21, additive).  For every (sample, head, value channel c):
 *     y[t] = (x[t] - mean_t x) * rstd * gamma[head][c] + beta[head][c],   rstd = 1 / sqrt(biased var_t x + eps)
 * over the n tokens, on the head-tile layout [B*n][h][DP], DP = round4(dk + p).  The p coordinate columns are copied
 * through, the pad columns are written as exact zeros (forward and backward).  gamma, beta, dgamma, dbeta: [h][dk];
 * stats [B][h][dk][2] = (mean, rstd), written by the forward and read by the backward.
 *     forward : per-chunk Welford (mean, M2) partials in ws, merged in chunk order with the pairwise update (never
 *               E[x^2] - mean^2), then the applying pass
 *     backward: xh = (x - mean) rstd from the RAW input X and stats (never Y / gamma: a zero weight is legal);
 *               dX = rstd gamma (dY - mean_t dY - xh mean_t(dY xh)),  dgamma = sum_{b,t} dY xh,  dbeta = sum_{b,t} dY,
 *               chunks, then samples, summed in order.  dgamma / dbeta may be NULL (not wanted).
 * No atomics: bit-identical from run to run.  In place is allowed (Y == X; dX == dY).  fp32 in every precision mode.
 * dk in {16, 32, 48, 64, 96} and p in {0, 1, 2}, else GT_ENOTSUP (the ws query returns 0); the forward refuses n == 1
 * (GT_EINVAL).  ws >= gt_token_norm_ws_bytes, which serves both directions.
 * ------------------------------------------------------------------------------------------- */
int64_t gt_token_norm_ws_bytes(int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p);
int gt_token_norm_fwd(const float* X, const float* gamma, const float* beta, float eps, float* Y, float* stats,
                      int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p, void* ws, int64_t ws_bytes, void* stream);
int gt_token_norm_bwd(const float* X, const float* dY, const float* gamma, const float* stats, float* dX,
                      float* dgamma, float* dbeta, int32_t B, int32_t n, int32_t h, int32_t dk, int32_t p, void* ws,
                      int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d of the FeedForward hidden activation: batch_norm=True of FeedForward (layers.py:979-987,
 * nn.BatchNorm1d(dim_feedforward) on the transposed hidden tensor; ABI v21, additive).  X is the dense [T][f] hidden
 * matrix, T = B n token rows; one mean and one BIASED variance per column c over all T rows:
 *     z[t][c] = (x[t][c] - mean[c]) * rstd[c] * gamma[c] + beta[c],   rstd = 1 / sqrt(var + eps)
 *     training != 0: batch statistics; running_mean <- (1 - m) running_mean + m mean and
 *                    running_var <- (1 - m) running_var + m var T / (T - 1), in place, when the pointers are given
 *     training == 0: mean / var are running_mean / running_var (required), nothing is updated
 * gamma, beta, running_*, bvar, dgamma, dbeta: [f].  stats [f][2] = (mean, rstd) and bvar [f] (the biased variance, in
 * eval mode a copy of running_var) are written by the forward; the backward reads stats.
 *     forward : per-chunk Welford (mean, M2) partials relative to row 0 of the column, in ws; merged with the pairwise
 *               update (never E[x^2] - mean^2) in two levels, each in a fixed order: the chunks of a group of 64 in chunk
 *               order, then the groups in group order; then the applying pass.  The chunk length follows T (32 .. 128 rows,
 *               longer beyond 4096 chunks), so no merge runs over more than 64 items
 *     backward: xh = (x - mean) rstd from the RAW input X and stats (never z / gamma: a zero weight is legal);
 *               dbeta = s1 = sum_t dZ, dgamma = s2 = sum_t dZ xh, summed in the same two levels (either may be NULL);
 *               d = rstd gamma (dZ - s1/T - xh s2/T) in training mode, d = rstd gamma dZ in eval mode, and the store
 *               carries the gate of what sits in front of the norm, gate_op of the gt_gemm_desc.aux_op vocabulary:
 *                 GT_AUX_NONE   dX = d
 *                 GT_AUX_GT0    dX = X > 0 ? d gate_scale : 0     (ReLU, dropout scale folded in; X is read anyway)
 *                 GT_AUX_DSILU  dX = d silu'(gate_aux) mask       (gate_aux [T][f] = saved pre-activation; gate_drop, optional:
 *                               mask index = the flat element index t f + c, the one gt_dropout_apply uses)
 *               gate_drop with another gate: GT_EINVAL.  GT_AUX_MUL: GT_ENOTSUP.
 * No atomics: bit-identical from run to run.  In place is allowed (Z == X; dX == dZ).  fp32 in every precision mode; the
 * caller's stream, no allocation, no host read-back.  f % 4 != 0: GT_ENOTSUP (the ws query returns 0); X, dZ, gate_aux, Z,
 * dX, stats, ws off a 16-byte boundary: GT_EALIGN; T < 2 in training mode: GT_EINVAL before anything is launched (one
 * value per channel has no variance; torch refuses it too).  ws >= gt_batchnorm_ws_bytes, which serves both directions.
 * ------------------------------------------------------------------------------------------- */
int64_t gt_batchnorm_ws_bytes(int64_t T, int32_t f);
int gt_batchnorm_fwd(const float* X, const float* gamma, const float* beta, float eps, float* running_mean,
                     float* running_var, float momentum, int32_t training, float* Z, float* stats, float* bvar, int64_t T,
                     int32_t f, void* ws, int64_t ws_bytes, void* stream);
int gt_batchnorm_bwd(const float* X, const float* dZ, const float* gamma, const float* stats, float* dX, float* dgamma,
                     float* dbeta, int64_t T, int32_t f, int32_t training, int32_t gate_op, const float* gate_aux,
                     float gate_scale, const gt_dropout* gate_drop, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused Fourier-type attention (layers.py:672-705):  out = ((Q' K'^T) * scale .* mask) V'  on the head-tile
 * layout [B*n][h][DP], without writing the n x n score matrix: score tiles are scaled, masked (stateless
 * dropout with mask index ((b*h+head)*n + query)*n + key -- the index the materialising gt_gemm path uses --
 * or an explicit [B,h,n,n] mask) and consumed in registers.  One entry point, three uses:
 *     forward        F1 = Q',  F2 = NULL, T1 = K', T2 = V',  owner_is_key = 0  ->  O1 = out
 *     d/dQ'          F1 = dO,  F2 = NULL, T1 = V', T2 = K',  owner_is_key = 0  ->  O1 = dQ'
 *     d/dV', d/dK'   F1 = K',  F2 = V',   T1 = Q', T2 = dO,  owner_is_key = 1  ->  O1 = dV', O2 = dK'
 * gt_fourier_attn: DP in {20, 36, 52}, else GT_ENOTSUP.  gt_fourier_attn_wide: the same pass, arguments and contracts for
 * the 64- and 96-wide heads, DP in {68, 100}, else GT_ENOTSUP (additive, same ABI; each entry point refuses the other's
 * widths).  A width neither takes has no fused fp32 kernel: materialise through gt_gemm.
 * ------------------------------------------------------------------------------------------- */
int gt_fourier_attn(const float* F1, const float* F2, const float* T1, const float* T2, float* O1, float* O2,
                    int32_t B, int32_t n, int32_t h, int32_t DP, float scale, const float* mask,
                    const gt_dropout* drop, int32_t owner_is_key, void* stream);
int gt_fourier_attn_wide(const float* F1, const float* F2, const float* T1, const float* T2, float* O1, float* O2,
                         int32_t B, int32_t n, int32_t h, int32_t DP, float scale, const float* mask,
                         const gt_dropout* drop, int32_t owner_is_key, void* stream);

/* The same operator (layers.py:672-705, the three uses above) in the two-term fp16 arithmetic (GT_PREC_F16X2: three products
 * per contraction on v_mfma_f32_16x16x32_f16, fp32 accumulation, fp32-class results) -- ABI v19.  The head tiles are split
 * ONCE per use into "images": per (batch, head, tile of 32 token rows) the two fp16 planes in MFMA fragment order, in the
 * layout of each of the two products, with the tile's power-of-two exponent and its largest row norm in a header.
 *     gt_fourier16_image_bytes   size of ONE tensor's image block (header + images) for head tiles [B*n][h][DP]
 *     gt_fourier16_presplit      X0..X3 (up to four head-tile tensors, NULL-terminated) -> image blocks I0..I3, one launch
 *     gt_fourier16_attn          as gt_fourier_attn with F1, F2, T1, T2 = image blocks of the tensors named there
 * DP in {20, 36, 52, 68, 100} (d_k = 16 / 32 / 48 / 64 / 96 with one or two coordinate columns; 68 and 100 are additive, same
 * ABI: older libraries answer them with 0 / GT_ENOTSUP), else GT_ENOTSUP and gt_fourier16_image_bytes returns 0.  A width
 * that is a multiple of 32 has no instance (the image layout needs a partial last k-step). */
int64_t gt_fourier16_image_bytes(int32_t B, int32_t n, int32_t h, int32_t DP);
int gt_fourier16_presplit(const float* X0, const float* X1, const float* X2, const float* X3, void* I0, void* I1, void* I2,
                          void* I3, int32_t B, int32_t n, int32_t h, int32_t DP, void* stream);
int gt_fourier16_attn(const void* F1, const void* F2, const void* T1, const void* T2, float* O1, float* O2, int32_t B,
                      int32_t n, int32_t h, int32_t DP, float scale, const float* mask, const gt_dropout* drop,
                      int32_t block16, int32_t owner_is_key, void* stream);
/* block16 != 0 (p must be 0.5 -- the reference's always-on F.dropout(p_attn), layers.py:700-701): the attention-score mask
 * is drawn per 4 x 4 block of the [n x n] matrix of each (batch, head): ONE hash per block,
 *     x = fmix32( (((b h + head) nq4 + (query >> 2)) nq4 + (key >> 2)) * 0x9e3779b1 + key(seed, salt) ),  nq4 = ceil(n / 4),
 *     keep(query, key) = bit 16 + 4 (query & 3) + (key & 3) of x,
 * instead of one hash per element (block16 = 0: the index documented at gt_fourier_attn).  gt_dropout_block16 applies the
 * same mask (and the 1 / (1 - p) rescale) in place to a materialised score matrix S [BH][n][n]: the path that returns the
 * attention weights runs it behind its score gt_gemm, so both paths draw one mask. */
int gt_dropout_block16(float* S, int64_t BH, int32_t n, const gt_dropout* drop, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax attention (layers.py:672-705, attention_type='softmax'; additive, same ABI) on the head-tile layout [B*n][h][DP]:
 *     S = Q' K'^T * scale,  P = softmax(S, over the keys),  Pm = P .* m,  O = Pm V'
 * m multiplies P AFTER the softmax and never enters the row sum: a stateless dropout (keep / (1 - p), mask index
 * ((b*h+head)*n + query)*n + key, the index documented at gt_fourier_attn; one hash per element), an explicit [B,h,n,n] mask
 * (which wins over `drop`), or 1.  fp32 (v_mfma_f32_16x16x4_f32, hardware exp2) in every precision mode.
 *
 * Fused route -- the n x n matrix is never written; gt_fourier_attn's kernel plus a running row maximum, a running row sum
 * and a rescale.  Rows of the last stream tile at or beyond n are excluded from the maximum and the sum.
 *     gt_softmax_attn_fwd      -> O, and L[0][b,h,q] = max_k S + log sum_k exp(S - max)         L: [2][B][h][n]
 *                                 L[1] = the rounding residual of L[0], (max - L[0]) + log sum: the backward evaluates
 *                                 exp((S - L[0]) - L[1]), so that scores of any size lose nothing through the statistic
 *     gt_softmax_attn_bwd_q    -> dQ', and D[b,h,q] = sum_c dO[q,c] O[q,c]                     D: [B][h][n]
 *     gt_softmax_attn_bwd_kv   -> dK', dV'   (reads the L of the forward and the D of bwd_q: call it after bwd_q)
 * with P = exp(S - L) recomputed (the scale multiplies the finished sum in all three passes: their S are bit-identical),  dPm = dO V'^T,  dV' = Pm^T dO,  dS = P .* (m .* dPm - D),  dQ' = dS K' * scale,
 * dK' = dS^T Q' * scale.  Zero pad columns of the inputs give exactly zero pad columns in dQ', dK', dV'.
 * DP in {20, 36, 52}, else GT_ENOTSUP.  Tiles and outputs 16-byte aligned.  No atomics: bit-identical from run to run.
 *     gt_softmax_attn_wide_fwd / _wide_bwd_q / _wide_bwd_kv: the same three passes, arguments and contracts for the 64- and
 *     96-wide heads, DP in {68, 100}, else GT_ENOTSUP (the narrow entry points keep returning GT_ENOTSUP at these widths).
 *     One block per CU (68 / 100 KiB of LDS stream tiles per block).
 *     gt_softmax_attn_nopos_fwd / _nopos_bwd_q / _nopos_bwd_kv: the same three passes, arguments and contracts on TAIL-FREE head
 *     tiles, exactly DP = d_k floats wide with no coordinate and no pad columns (the classic Transformer layer,
 *     ops.multihead_attention): DP in {16, 32, 48, 64, 96}, else GT_ENOTSUP.  Every column of the tile is a value column and
 *     takes part in both products; L and its residual are written as by gt_softmax_attn_fwd.
 *
 * Materialised route (the caller wants Pm back): S by gt_gemm, then one wave per row of the [rows][n] matrix:
 *     gt_row_softmax_fwd       P = softmax(S) (maximum subtracted), Pm = P .* m;  P == S and (no mask, no dropout) Pm == P allowed
 *     gt_row_softmax_bwd       dS = P .* (m .* dPm - sum_k P m dPm);  dS == dPm allowed
 * Mask index of element (row, k): (row0 + row)*n + k -- with rows = B*h*n and row0 = 0 the index of the fused route, so both
 * routes draw one mask; `mask` (explicit) is indexed row*n + k.
 * ------------------------------------------------------------------------------------------- */
int gt_softmax_attn_fwd(const float* Q, const float* K, const float* V, float* O, float* L, int32_t B, int32_t n, int32_t h,
                        int32_t DP, float scale, const float* mask, const gt_dropout* drop, void* stream);
int gt_softmax_attn_bwd_q(const float* dO, const float* O, const float* Q, const float* K, const float* V, const float* L,
                          float* D, float* dQ, int32_t B, int32_t n, int32_t h, int32_t DP, float scale, const float* mask,
                          const gt_dropout* drop, void* stream);
int gt_softmax_attn_bwd_kv(const float* K, const float* V, const float* Q, const float* dO, const float* L, const float* D,
                           float* dK, float* dV, int32_t B, int32_t n, int32_t h, int32_t DP, float scale, const float* mask,
                           const gt_dropout* drop, void* stream);
int gt_softmax_attn_wide_fwd(const float* Q, const float* K, const float* V, float* O, float* L, int32_t B, int32_t n,
                             int32_t h, int32_t DP, float scale, const float* mask, const gt_dropout* drop, void* stream);
int gt_softmax_attn_wide_bwd_q(const float* dO, const float* O, const float* Q, const float* K, const float* V, const float* L,
                               float* D, float* dQ, int32_t B, int32_t n, int32_t h, int32_t DP, float scale,
                               const float* mask, const gt_dropout* drop, void* stream);
int gt_softmax_attn_wide_bwd_kv(const float* K, const float* V, const float* Q, const float* dO, const float* L,
                                const float* D, float* dK, float* dV, int32_t B, int32_t n, int32_t h, int32_t DP, float scale,
                                const float* mask, const gt_dropout* drop, void* stream);
int gt_softmax_attn_nopos_fwd(const float* Q, const float* K, const float* V, float* O, float* L, int32_t B, int32_t n,
                              int32_t h, int32_t DP, float scale, const float* mask, const gt_dropout* drop, void* stream);
int gt_softmax_attn_nopos_bwd_q(const float* dO, const float* O, const float* Q, const float* K, const float* V, const float* L,
                                float* D, float* dQ, int32_t B, int32_t n, int32_t h, int32_t DP, float scale,
                                const float* mask, const gt_dropout* drop, void* stream);
int gt_softmax_attn_nopos_bwd_kv(const float* K, const float* V, const float* Q, const float* dO, const float* L,
                                 const float* D, float* dK, float* dV, int32_t B, int32_t n, int32_t h, int32_t DP, float scale,
                                 const float* mask, const gt_dropout* drop, void* stream);
int gt_row_softmax_fwd(const float* S, float* P, float* Pm, int64_t rows, int32_t n, int64_t row0, const float* mask,
                       const gt_dropout* drop, void* stream);
int gt_row_softmax_bwd(const float* P, const float* dPm, float* dS, int64_t rows, int32_t n, int64_t row0, const float* mask,
                       const gt_dropout* drop, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Random-feature attention (examples/ex1_burgers_random_fourier_features.py, attention_type 'rfa' / 'favor'; additive, same
 * ABI): ONE head of width d with m = d features, Om [d][m/2] the random projection, s = d^(-1/4):
 *     u(z)  = (s z) Om
 *     rfa   : phi(z) = sqrt(2/m) [cos u, sin u]
 *     favor : phi(z) = [exp(u - c), exp(-u - c)],  c = |s z|^2 / 2 + log(m) / 2
 *     KVa   = phi(K)^T [V, 1]                     [B][m][d + 4]: columns < d are KV, column d is sum_tokens phi(K),
 *                                                  columns d + 1 .. d + 3 are written as zeros
 *     den   = phi(Q) . KVa[:, d] + eps,   out = phi(Q) KVa[:, :d] / den           (no 1/n, no dropout)
 * Q, K, V are column blocks of row-major matrices with leading dimension ld (the packed projection [B*n][3d]: ld = 3d);
 * dQ, dK, dV go to column blocks with leading dimension ldg.  out, dOut [B*n][d] and den [B*n] are dense.  fp32 on
 * v_mfma_f32_16x16x4_f32 with library exp / sin / cos in every precision mode; phi and u are never written to memory.
 *     gt_rfattn_kv      -> KVa                                   one slab per 256 tokens and sample, merged in a fixed order
 *     gt_rfattn_q       -> out, den
 *     gt_rfattn_bwd_q   -> dQ, dKVa = phi(Q)^T [dOut / den, -(dOut . out) / den]      (slabs as gt_rfattn_kv)
 *     gt_rfattn_bwd_kv  -> dK, dV from dKVa                      (call it after gt_rfattn_bwd_q)
 * gt_rfattn_slabs(n): slabs per sample; gt_rfattn_ws_bytes: scratch of gt_rfattn_kv / gt_rfattn_bwd_q, 0 with one slab (ws may
 * then be NULL).  Tokens at or beyond n leave no trace in KVa, dKVa.  No atomics: bit-identical from run to run.  Plain
 * pointers, the caller's stream, no allocation.  d in {32, 64, 96}, any n >= 1, B <= 65535, else GT_ENOTSUP; another kind, a
 * NULL tensor, a non-positive size: GT_EINVAL; a tensor off a 16-byte (den: 4-byte) boundary, ld or ldg < d or not a
 * multiple of 4: GT_EALIGN; ws too small: GT_EWS.  All decided from the arguments alone, nothing launched. */
#define GT_RFATTN_RFA   0
#define GT_RFATTN_FAVOR 1
int32_t gt_rfattn_slabs(int32_t n);
int64_t gt_rfattn_ws_bytes(int32_t B, int32_t n, int32_t d);
int gt_rfattn_kv(const float* K, const float* V, int64_t ld, const float* omega, float* KVa, int32_t B, int32_t n, int32_t d,
                 int32_t kind, void* ws, int64_t ws_bytes, void* stream);
int gt_rfattn_q(const float* Q, int64_t ld, const float* omega, const float* KVa, float* out, float* den, int32_t B, int32_t n,
                int32_t d, int32_t kind, float eps, void* stream);
int gt_rfattn_bwd_q(const float* Q, int64_t ld, const float* omega, const float* KVa, const float* dOut, const float* out,
                    const float* den, float* dQ, int64_t ldg, float* dKVa, int32_t B, int32_t n, int32_t d, int32_t kind,
                    void* ws, int64_t ws_bytes, void* stream);
int gt_rfattn_bwd_kv(const float* K, const float* V, int64_t ld, const float* omega, const float* dKVa, float* dK, float* dV,
                     int64_t ldg, int32_t B, int32_t n, int32_t d, int32_t kind, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Truncated-DFT stages along the contiguous grid axis of SpectralConv2d (layers.py:1176 rfft2 and :1187
 * irfft2 restricted to the kept modes; the residual nn.Linear of :1128 / :1196 rides on the synthesis).
 * One batch item = one grid line; all tensors dense fp32:
 *     analysis    Y[b] (P x C)  = F^T X[b]                 F [n, P],  X [nb, n, C],  Y [nb, P, C]
 *     synthesis   Y[b] (n x Co) = act( F Z[b] + X2[b] W2 + bias ),   pre (optional) = the argument of act
 *                 F [n, P], Z [nb, P, Co], X2 [nb, n, C2], W2 [C2, Co], bias [Co] or NULL, Y / pre [nb, n, Co]
 * The backward of one is the other with the transposed basis (spectral.py).  Implemented for C = Co = C2 =
 * 32 channels, P = 2*modes <= 32 (synthesis: P % 4 == 0), n <= 224; anything else returns GT_ENOTSUP and the
 * caller runs the same product through gt_gemm.
 * ------------------------------------------------------------------------------------------- */
int gt_dft_analysis(const float* F, const float* X, float* Y, int32_t nb, int32_t n, int32_t P, int32_t C,
                    void* stream);
int gt_dft_synthesis(const float* F, const float* Z, float* Y, int32_t nb, int32_t n, int32_t P, int32_t Co,
                     const float* X2, const float* W2, int32_t C2, const float* bias, int32_t act, float* pre,
                     void* stream);
/* ABI v21: the same with  Y *= silu'(out_gate)  on the store (out_gate [nb, n, Co]; act must be GT_ACT_NONE, pre NULL).  In the
 * backward of a SpectralConv2d stack (model.py:569-572 backwards) the synthesis of layer l + 1 forms the gradient of layer l's
 * activated output: with out_gate = layer l's saved pre-activation it hands over the gradient of the pre-activation, and
 * layer l's own gt_act_bwd pass disappears. */
int gt_dft_synthesis_gated(const float* F, const float* Z, float* Y, int32_t nb, int32_t n, int32_t P, int32_t Co,
                           const float* X2, const float* W2, int32_t C2, const float* bias, int32_t act, float* pre,
                           const float* out_gate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused pointwise regression head  out[t] = w2 . act(W1 x[t] + b1) + b2  (model.py:575-580, 625-629: the
 * Linear(K -> N), activation, Linear(N -> n_out) tail of SpectralRegressor at every fine-grid point) and its
 * complete backward in one pass over x: the [T, N] hidden activation and dL/dh never reach HBM.
 *     X [T, K] dense, W1 [N, K], b1 [N] or NULL, w2 [n_out, N], b2 [n_out] or NULL, out [T, n_out]
 *     backward: g [T, n_out] = dL/dout  ->  dX [T, K] (or NULL), dW1 [N, K], db1 [N] / dw2 [n_out, N] /
 *     db2 [n_out] (each may be NULL); ws >= gt_mlp_head_bwd_ws_bytes(T) bytes of scratch (deterministic
 *     fixed-order reduction).  Implemented for K = 32, N = 128, n_out = 1 (else GT_ENOTSUP: use gt_gemm's
 *     ep_mode GT_EP_ROWDOT / GT_EP_MLP_BWD path, which covers N <= 128, n_out <= 4).
 *     precision: GT_PREC_F16X2 = two fp16 terms per operand, three products on the fp16 matrix pipe (per-row / per-tensor
 *     / running power-of-two exponents, gt_head.hip); any other GT_PREC_* = the fp32-MFMA kernels (exact fp32 products).
 * ------------------------------------------------------------------------------------------- */
int gt_mlp_head_fwd(const float* X, int64_t T, int32_t K, int32_t N, int32_t n_out, const float* W1,
                    const float* b1, const float* w2, const float* b2, int32_t act, int32_t precision, float* out,
                    void* stream);
int64_t gt_mlp_head_bwd_ws_bytes(int64_t T);
int gt_mlp_head_bwd(const float* X, int64_t T, int32_t K, int32_t N, int32_t n_out, const float* W1,
                    const float* b1, const float* w2, int32_t act, int32_t precision, const float* g, float* dX,
                    float* dW1, float* db1, float* dw2, float* db2, void* ws, int64_t ws_bytes, void* stream);
/* ABI v21: dX *= silu'(dx_gate) on the store (dx_gate [T, K] = the pre-activation of the layer whose SiLU produced X, e.g.
 * the last SpectralConv2d in front of the head, model.py:572-575); NULL = gt_mlp_head_bwd. */
int gt_mlp_head_bwd_gated(const float* X, int64_t T, int32_t K, int32_t N, int32_t n_out, const float* W1,
                          const float* b1, const float* w2, int32_t act, int32_t precision, const float* g, float* dX,
                          const float* dx_gate, float* dW1, float* db1, float* dw2, float* db2, void* ws, int64_t ws_bytes,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row LayerNorm over the feature axis (model.py:128-129,134-135 when layer_norm=True).
 * ------------------------------------------------------------------------------------------- */
int gt_layernorm_fwd(const float* x, const float* gamma, const float* beta, int32_t T, int32_t d,
                     float eps, float* y, float* stats /* [T][2] mean,rstd */, void* stream);
int gt_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* stats,
                     int32_t T, int32_t d, float* dx, float* dgamma, float* dbeta,
                     void* ws, int64_t ws_bytes, void* stream);
int64_t gt_layernorm_bwd_ws_bytes(int32_t T, int32_t d);

/* ---------------------------------------------------------------------------------------------
 * Spectral mode mixing (layers.py:1066-1075, 1143-1151): per retained mode q, complex
 *   Y[b][ri][q][o] = sum_i X[b][ri'][q][i] (x) W[i][o][q]      (complex product, real-pair weights)
 * X, Y layout: [B][2][Q][C] (re plane, im plane), Q = number of retained modes, C channels.
 * W layout:    [Cin][Cout][Q][2]  (the reference's parameter layout; for 2-D the two corner
 *              blocks are passed as two calls or as Q = modes*modes each via `w_qstride`).
 * Backward: dX from dY and W ;  dW from X and dY (summed over the batch).
 * Any positive B, Q, Cin, Cout runs.  Two routes, picked per direction by gt_modemix_plan (host only, touches no device;
 * the two launchers and the workspace query all ask it, so they cannot disagree):
 *   GT_MODEMIX_RESIDENT  the whole [Cin][Cout] slice of a mode in LDS, one block per (mode, batch slice).
 *                        Forward: where (2 Cin Cout + 16 Cin) * 4 bytes <= 160 KiB.  Backward: where Cin * Cout <= 6144
 *                        and (2 Cin (Cout + 1) + 16 Cin + 16 Cout) * 4 bytes <= 160 KiB.
 *   GT_MODEMIX_TILED     everywhere else: a block owns 4 adjacent modes and a 32-channel output tile (weight gradient: a
 *                        32 x 32 channel tile), the contraction goes through LDS in chunks; LDS and registers do not
 *                        depend on the widths.  fp32 FMA chains, no atomics.
 * Workspace: the backward's dW is summed over `bwd_slices` batch slices; the per-slice partials go through ws
 * (gt_modemix_bwd_ws_bytes = bwd_slices * Cin * Cout * Q * 2 * 4, or 0 when bwd_slices == 1) and are summed in a fixed order.
 * Resident: slices = min(ceil(768 / Q), ceil(B / 8)).  Tiled: 1 once (mode groups x channel tiles) fill the chip (>= 256
 * blocks), else min(ceil(512 / blocks), ceil(B / 8)).
 * ------------------------------------------------------------------------------------------- */
enum { GT_MODEMIX_RESIDENT = 0, GT_MODEMIX_TILED = 1 };
/* ABI v21 (additive): the route of each direction and the batch slices of the backward; any out pointer may be NULL. */
int gt_modemix_plan(int32_t B, int32_t Q, int32_t Cin, int32_t Cout, int32_t* fwd_route, int32_t* bwd_route,
                    int32_t* bwd_slices);
int gt_modemix_fwd(const float* X, const float* W, int32_t B, int32_t Q, int32_t Cin, int32_t Cout,
                   int64_t x_bstride, int64_t y_bstride, int32_t q_total_x, int32_t q_total_y,
                   int32_t q_off, float* Y, void* stream);
int64_t gt_modemix_bwd_ws_bytes(int32_t B, int32_t Q, int32_t Cin, int32_t Cout);
int gt_modemix_bwd(const float* X, const float* W, const float* dY, int32_t B, int32_t Q,
                   int32_t Cin, int32_t Cout, int64_t x_bstride, int64_t y_bstride,
                   int32_t q_total_x, int32_t q_total_y, int32_t q_off,
                   float* dX, float* dW, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=True (F.interpolate at layers.py:483-512, 658-670), with the
 * channels-first <-> channels-last change of the scaler boundaries (model.py:675-687, 740-749)
 * fused in.  x: [B,C,Hi,Wi] (in_nhwc=0) or [B,Hi,Wi,C] (in_nhwc=1); y likewise with Ho,Wo and
 * out_nhwc.  act: GT_ACT_NONE or GT_ACT_RELU applied to the resized output.  NHWC sides need
 * C % 4 == 0 and 16-byte aligned pointers.
 * Backward: g, y_saved (the activated forward output; only read when act == GT_ACT_RELU) have the
 * forward OUTPUT shape/layout, dx the forward INPUT shape/layout.  Gather formulation: no atomics,
 * bitwise deterministic.
 * ------------------------------------------------------------------------------------------- */
int gt_bilinear2d_fwd(const float* x, float* y, int32_t B, int32_t C, int32_t Hi, int32_t Wi,
                      int32_t Ho, int32_t Wo, int32_t in_nhwc, int32_t out_nhwc, int32_t act,
                      void* stream);
/* Same, plus an affine term per output pixel q and channel c (NHWC in and out only):
 *     y = act( resize(x) + bias[c] + sum_j rp_a[q*rp_lda + j] * rp_b[c*rp_ldb + j] )
 * This is what makes  fc(cat[upsample(x), grid])  (model.py:740-749 followed by model.py:615-617)
 * computable as  upsample(x W_x^T) + grid W_g^T + b : the pointwise Linear commutes with the bilinear
 * interpolation (its weights sum to one), so the Linear runs at the coarse resolution and only the
 * freq_dim-channel result is interpolated. */
typedef struct gt_resize_affine {
    const float* bias;                 /* [C] or NULL */
    int32_t rp;                        /* 0..8 */
    const float* rp_a; int64_t rp_lda; /* [B*Ho*Wo, rp] */
    const float* rp_b; int64_t rp_ldb; /* [C, rp] */
} gt_resize_affine;
int gt_bilinear2d_fwd_affine(const float* x, float* y, int32_t B, int32_t C, int32_t Hi, int32_t Wi,
                             int32_t Ho, int32_t Wo, int32_t in_nhwc, int32_t out_nhwc, int32_t act,
                             const gt_resize_affine* aff, void* stream);
int gt_bilinear2d_bwd(const float* g, const float* y_saved, float* dx, int32_t B, int32_t C,
                      int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t in_nhwc,
                      int32_t out_nhwc, int32_t act, void* stream);
/* Channels-last resize whose INPUT is the padded three-segment buffer the down-scaler's convolution chain writes
 * (Interp2dEncoder, layers.py:497-512: cat[x1, x2, x3] -> F.interpolate -> activation): x [B, Hi, Wi, 3*segp] holds the
 * C real channels in three column segments of segp channels each -- real channel c at column c + (segp - seg) * min(c / seg, 2),
 * i.e. segment widths seg, seg, C - 2*seg, zeros behind them -- and y [B, Ho, Wo, C] is dense.  The concatenation is never
 * materialised.  Backward: g, y_saved dense like y; dx in the padded layout (padding columns get zero); x_gate (optional)
 * = the forward input x itself when it is the output of a ReLU: dx is zeroed where x <= 0, i.e. the gradient leaves
 * already multiplied by the derivative of the ReLU that produced x (one elementwise pass less in its producer).
 * ABI v20 -- act = GT_ACT_SILU (Interp2dEncoder's default activation_type, layers.py:446-456; ex3's down-scaler): the forward
 * also writes dact [B, Ho, Wo, C] = silu'(resized value) and the backward takes THAT buffer as y_saved (its gradient is
 * g * dact); gate_mul != 0 makes x_gate a multiplicative factor (dx *= x_gate: the keepscale * silu' buffer a
 * GT_ACT_DROP_SILU product left in `pre`) instead of the ReLU test. */
int gt_bilinear2d_seg_fwd(const float* x, float* y, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho,
                          int32_t Wo, int32_t act, int32_t seg, int32_t segp, float* dact, void* stream);
int gt_bilinear2d_seg_bwd(const float* g, const float* y_saved, float* dx, int32_t B, int32_t C, int32_t Hi,
                          int32_t Wi, int32_t Ho, int32_t Wo, int32_t act, int32_t seg, int32_t segp,
                          const float* x_gate, int32_t gate_mul, void* stream);

/* ---------------------------------------------------------------------------------------------
 * First stage of the CNN down-scaler in one pass (layers.py:483-495 with Conv2dResBlock :88-150):
 *     y = relu( resize( relu( dropout( conv3x3(x; w), p ) ), (Ho, Wo) ) )
 * x [B,Cin,H,W] (Cin <= 4), w [Cout,Cin,3,3] (padding 1, stride 1, no bias), y [B,Cout,Ho,Wo], all
 * channels-first.  The Cout-channel fine-resolution map is never materialised.  The dropout mask is
 * indexed by the linear NCHW index of the (virtual) conv output, i.e. identical to running
 * gt_dropout_apply on it.  act: GT_ACT_RELU, or (ABI v20) GT_ACT_SILU = the same pass with SiLU on both sides of the resize
 * (Interp2dEncoder's default activation_type='silu', layers.py:446-456: ex3's down-scaler); the SiLU backward re-evaluates
 * the convolution at the four source pixels (no decision bits: relu_bits must be NULL) and does not read y.
 * Backward produces the weight gradient only (dw [Cout,Cin,3,3]; two-pass deterministic reduction
 * through ws); callers that need d/dx use the unfused operators.
 * ------------------------------------------------------------------------------------------- */
int gt_conv3x3_resize_fwd(const float* x, const float* w, float* y, int32_t B, int32_t Cin, int32_t Cout,
                          int32_t H, int32_t W, int32_t Ho, int32_t Wo, const gt_dropout* drop, int32_t act,
                          void* stream);
int gt_conv3x3_resize_bwd(const float* g, const float* y, const float* x, const float* w, int32_t B,
                          int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                          const gt_dropout* drop, int32_t act, float* dw, void* ws, int64_t ws_bytes,
                          void* stream);
int64_t gt_conv3x3_resize_bwd_ws_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W);
/* The same with y (and g, y of the backward) channels-last [B, Ho, Wo, Cout]: what the channels-last convolution chain
 * of the down-scaler consumes. */
int gt_conv3x3_resize_fwd_nhwc(const float* x, const float* w, float* y, int32_t B, int32_t Cin, int32_t Cout,
                               int32_t H, int32_t W, int32_t Ho, int32_t Wo, const gt_dropout* drop, int32_t act,
                               void* relu_bits, void* stream);
int gt_conv3x3_resize_bwd_nhwc(const float* g, const float* y, const float* x, const float* w, int32_t B,
                               int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                               const gt_dropout* drop, int32_t act, const void* relu_bits, float* dw, void* ws,
                               int64_t ws_bytes, void* stream);
/* relu_bits (optional, NULL = off; Cout % 16 == 0, 8-byte aligned, gt_conv3x3_resize_bits_bytes() bytes): the forward
 * records 4 bits per (output pixel, channel) -- source pixel t of the bilinear stencil kept by the dropout AND positive,
 * all four cleared when the resized value is <= 0 -- and the backward, handed the same buffer, takes its decisions from
 * there: it neither re-evaluates the convolution at the four source pixels nor re-draws the mask, and does not read y
 * (y may be NULL then).  Same weight gradient bit for bit decisions, half the instructions, 0.45 instead of 0.81 GB read. */
int64_t gt_conv3x3_resize_bits_bytes(int32_t B, int32_t Cout, int32_t Ho, int32_t Wo);

/* ---------------------------------------------------------------------------------------------
 * Weight gradient of a NARROW channels-last 3x3 convolution (padding 1, stride 1, no bias): the three convolutions of the
 * down-scaler's chain, reference libs/layers.py:463-482 (Interp2dEncoder conv1 / conv2 / conv3 = Conv2dResBlock,
 * layers.py:88-150), whose weight gradients autograd would compute with cudnn/MIOpen's conv2d weight backward:
 *     dw[co][ci][ky][kx] = alpha * sum_{b,y,x} gy[(b H + y) W + x][co] * x[(b H + y + ky - 1) W + x + kx - 1][ci]
 * gy / x: channels-last images with pixel pitches ldg >= Cout / ldx >= Cin (a column segment of a wider buffer is read in
 * place), 16-byte aligned, pitches multiples of 4.  dw: [Cout][Cin][3][3], the reference's layout.  precision: GT_PREC_BF16X3
 * (three bf16 planes, six products) or GT_PREC_F16X2 (two fp16 planes under one running power-of-two scale per operand and
 * block, three products); each operand value is split once per block (gt_convw.hip).
 * GT_ENOTSUP unless (Cout == 48, Cin % 16 == 0: the down-scaler's padded narrow convolutions) or (Cout % 64 == 0,
 * Cin % 32 == 0: the up-scaler's 128 -> 128 convolution).  Rows wider than 80 pixels are worked in equal x-segments of at
 * most 80 (round 5: the 113 / 114-pixel rows of the 211 x 211 configuration).  Deterministic: partial results per (image, row
 * chunk, segment) in ws
 * (>= gt_conv3x3_wgrad_nhwc_ws_bytes), summed in a fixed order.
 * ------------------------------------------------------------------------------------------- */
int gt_conv3x3_wgrad_nhwc(const float* gy, int64_t ldg, const float* x, int64_t ldx, float* dw, int32_t B, int32_t H,
                          int32_t W, int32_t Cin, int32_t Cout, float alpha, int32_t precision, void* ws, int64_t ws_bytes,
                          void* stream);
int64_t gt_conv3x3_wgrad_nhwc_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout);

/* Parity hook for the fused convolution's ReLU (reference: Conv2dResBlock's activation, layers.py:139-149, which the fused
 * pass never materialises): with a device buffer `mask` [B, Cout, H, W] of bytes registered, every following
 * gt_conv3x3_resize_fwd(_nhwc) records the decision it takes for each fine-grid value it evaluates (1: kept by the dropout
 * and positive, 0: not; values no output pixel touches keep what the caller stored).  NULL switches it off.  The pointer is
 * a process-wide device variable: tests only. */
int gt_debug_conv0_mask(void* mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step on ONE flat fp32 bucket: what utils_ft.py:676-681 does per batch
 * (nn.utils.clip_grad_norm_(model.parameters(), grad_clip); optimizer.step() with torch.optim.Adam), as three
 * launches for the whole model.  Norm, step count and learning rate are read from DEVICE memory (no host sync; one
 * captured launch serves every iteration).
 *   gt_grad_sqnorm    out[0] = sum_i (scale * g[i])^2            (deterministic two-pass; ws >= gt_grad_sqnorm_ws_bytes())
 *   gt_adam_clip_step g' = gscale * clip * g + weight_decay * p,  clip = min(1, max_norm / (sqrt(sqnorm[0]) + 1e-6))
 *                     (max_norm <= 0: no clipping, sqnorm may be NULL);
 *                     m = beta1 m + (1-beta1) g';  v = beta2 v + (1-beta2) g'^2;  t = step[0] (already incremented:
 *                     bump it with gt_seed_advance before the call);
 *                     p -= lr[0] / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)      -- torch.optim.Adam.
 *   beta1_dev (optional device scalar) overrides beta1: OneCycleLR cycles Adam's beta1 together with the rate.
 *   gscale folds the 1/world of the gradient average after a sum-all-reduce (pass the same factor as `scale` to
 *   gt_grad_sqnorm so that the norm is the norm of the averaged gradient).  All pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int64_t gt_grad_sqnorm_ws_bytes(void);
int gt_grad_sqnorm(const float* g, int64_t n, float scale, float* out, void* ws, int64_t ws_bytes, void* stream);
int gt_adam_clip_step(float* p, const float* g, float* m, float* v, int64_t n, const float* sqnorm, float gscale,
                      float max_norm, const float* lr, float beta1, float beta2, float eps, float weight_decay,
                      const uint64_t* step, const float* beta1_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 2-D training objective, per sample (ft.py:983-1105, WeightedL2Loss2d.forward without its alpha term and `weights`;
 * ABI v21, additive).  P, T [N][n][n] prediction and target, G [N][n][n][2] target gradient (optional), K N n n coefficient
 * values (optional, needs G; absent = 1).  Even dilation d < n, s = d / 2, m = n - d, M = n n:
 *     A = sum T^2     E = sum (P - T)^2     Gs = sum_{i,j,c} K G_c^2
 *     Dx P[i][j] = (P[i+s][j] - P[i-s][j]) / (d h),  Dy P[i][j] = (P[i][j+s] - P[i][j-s]) / (d h)   for s <= i, j < n - s
 *     R  = sum over those (i, j) and c of (K[i][j] (G_c[i][j] - D_c P[i][j]))^2
 *     L2 = A / M + eps      H1 = Gs / M + eps  (1 without G)
 *     loss = beta (E / M) / L2      reg = gamma h (R / (2 m^2)) / H1
 *   gt_h1loss2d_fwd    one streaming pass: per-block partial sums of (A, E, Gs, R) into ws.  want_reg == 0: R is not formed;
 *                      G == NULL: Gs neither (want_reg != 0 then: GT_EINVAL)
 *   gt_h1loss2d_final  merges the partials of each sample in block order, in double, and writes loss, L2, H1 [N] and, unless
 *                      NULL, reg [N].  has_g: whether the forward had G.  Same N, n and ws as the forward, same stream
 *   gt_h1loss2d_bwd    dP [N][n][n], dense, from the upstream gradients gl, gr [N] of loss and reg (either may be NULL = 0) and
 *                      the L2, H1 the final pass wrote.  With r_c = K^2 (D_c P - G_c) on s <= i, j < n - s and 0 elsewhere:
 *                        dP[i][j] = gl beta 2 / (M L2) (P - T)[i][j]
 *                                 + gr gamma h 2 / (2 m^2 H1) / (d h) (r_x[i-s][j] - r_x[i+s][j] + r_y[i][j-s] - r_y[i][j+s])
 *                      a gather: every pixel recomputes the at most four residuals it feeds
 * P is read with the pixel pitch ldp >= 1 in floats (the callers pass channel 0 of an [N][n][n][c] tensor); T, G, K, dP are
 * dense.  fp32 in every precision mode, the merge in double; no atomics: bit-identical from run to run.  The caller's
 * stream, no allocation, no host read-back.  16-byte accesses where a tensor is 16-byte aligned (P: and ldp == 1), scalar
 * ones otherwise.  n <= d, odd d, h <= 0, N < 1, K without G: GT_EINVAL; a pointer off a 4-byte (ws: 16-byte) boundary:
 * GT_EALIGN; ws < gt_h1loss2d_ws_bytes(N, n): GT_EWS.
 * ------------------------------------------------------------------------------------------- */
int64_t gt_h1loss2d_ws_bytes(int32_t N, int32_t n);
int gt_h1loss2d_fwd(const float* P, int64_t ldp, const float* T, const float* G, const float* K, int32_t N, int32_t n,
                    int32_t dilation, float h, int32_t want_reg, void* ws, int64_t ws_bytes, void* stream);
int gt_h1loss2d_final(int32_t N, int32_t n, int32_t dilation, float h, float beta, float gamma, float eps, int32_t has_g,
                      float* loss, float* reg, float* L2, float* H1, const void* ws, int64_t ws_bytes, void* stream);
int gt_h1loss2d_bwd(const float* P, int64_t ldp, const float* T, const float* G, const float* K, const float* L2,
                    const float* H1, const float* gl, const float* gr, int32_t N, int32_t n, int32_t dilation, float h,
                    float beta, float gamma, float* dP, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 1-D training objective, per sample (ft.py:898-980, WeightedL2Loss.forward without its alpha term, its noise and its
 * orthogonaliser; ABI v21, additive).  P, T [N][L] prediction and target, G [N][L] target derivative (optional).  Even
 * dilation d < L, s = d / 2:
 *     A = sum T^2     E = sum (P - T)^2     Gs = sum G^2
 *     D P[c] = (P[c+s] - P[c-s]) / (d h)  and  R = sum (G[c] - D P[c])^2   over s <= c < L - s
 *     L2 = h A      H1 = h Gs  (1 without G)                              -- no eps, as the reference
 *     loss = beta h E / L2      reg = gamma_h h R / H1                    -- gamma_h: the class stores gamma h
 *   gt_h1loss1d_fwd    one streaming pass: per-block partial sums of (A, E, Gs, R) into ws.  want_reg == 0: R is not formed;
 *                      G == NULL: Gs neither (want_reg != 0 then: GT_EINVAL)
 *   gt_h1loss1d_final  merges the partials of each sample in block order, in double, and writes loss, L2, H1 [N] and, unless
 *                      NULL, reg [N].  has_g: whether the forward had G.  Same N, L and ws as the forward, same stream
 *   gt_h1loss1d_bwd    dP [N][L], dense, from the upstream gradients gl, gr [N] of loss and reg (either may be NULL = 0) and
 *                      the L2, H1 the final pass wrote.  With r[c] = D P[c] - G[c] on s <= c < L - s and 0 elsewhere:
 *                        dP[i] = gl beta h 2 / L2 (P - T)[i] + gr gamma_h h 2 / H1 / (d h) (r[i-s] - r[i+s])
 *                      a gather: every element recomputes the at most two residuals it feeds
 * P is read with the element pitch ldp >= 1 in floats (the callers pass channel 0 of an [N][L][c] tensor); T, G, dP are
 * dense.  fp32, the merge in double; no atomics: bit-identical from run to run.  The caller's stream, no allocation, no host
 * read-back.  16-byte accesses where a tensor is 16-byte aligned (P: and ldp == 1), scalar ones otherwise.  L <= d, odd d,
 * h <= 0, N < 1: GT_EINVAL; a pointer off a 4-byte (ws: 16-byte) boundary: GT_EALIGN; ws < gt_h1loss1d_ws_bytes(N, L): GT_EWS;
 * more than 2^31 - 1 blocks (N ceil((L / 4 + 2) / 512)): GT_ENOTSUP.
 * ------------------------------------------------------------------------------------------- */
int64_t gt_h1loss1d_ws_bytes(int32_t N, int32_t L);
int gt_h1loss1d_fwd(const float* P, int64_t ldp, const float* T, const float* G, int32_t N, int32_t L, int32_t dilation,
                    float h, int32_t want_reg, void* ws, int64_t ws_bytes, void* stream);
int gt_h1loss1d_final(int32_t N, int32_t L, int32_t dilation, float h, float beta, float gamma_h, int32_t has_g, float* loss,
                      float* reg, float* L2, float* H1, const void* ws, int64_t ws_bytes, void* stream);
int gt_h1loss1d_bwd(const float* P, int64_t ldp, const float* T, const float* G, const float* L2, const float* H1,
                    const float* gl, const float* gr, int32_t N, int32_t L, int32_t dilation, float h, float beta,
                    float gamma_h, float* dP, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 'conv' scaler modes (DownScaler / UpScaler with downsample_mode / upsample_mode = 'conv', model.py:653-662, 709-726;
 * ABI v21, additive).
 *
 * y = act(avgpool2x2(x)): nn.AvgPool2d(2) and the activation behind it in Conv2dEncoder (layers.py:329-341).  x [B,C,H,W]
 * (in_nhwc = 0) or [B,H,W,C]; y likewise with Ho = H / 2, Wo = W / 2 (floor: an odd trailing row / column is not read) and
 * out_nhwc.  act: GT_ACT_NONE | GT_ACT_RELU | GT_ACT_SILU.  Backward: dx (x's shape and layout) = 0.25 act'(pooled) dy at the
 * four contributors, zeros in a dropped row / column; `pooled` is recomputed from x.  Every value is written once, no
 * atomics.  float4 / float2 accesses where both sides are channels-last with C % 4 == 0, or both channels-first with
 * W % 4 == 0, and the pointers are 16-byte aligned; scalar ones otherwise.  H < 2, W < 2 or another act: GT_EINVAL.
 * ------------------------------------------------------------------------------------------- */
int gt_avgpool2_act_fwd(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t in_nhwc,
                        int32_t out_nhwc, int32_t act, void* stream);
int gt_avgpool2_act_bwd(const float* x, const float* dy, float* dx, int32_t B, int32_t C, int32_t H, int32_t W,
                        int32_t in_nhwc, int32_t out_nhwc, int32_t act, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spatial half of nn.ConvTranspose2d(Cin, Cout, kernel_size=3, stride=2, padding=pad, output_padding=outpad) on channels-last
 * images (DeConv2dBlock, layers.py:515-559):  y[b,oy,ox,co] = bias[co] + sum x[b,iy,ix,ci] w[ci,co,ky,kx],  oy = 2 iy - pad + ky,
 * Ho = 2 (H - 1) - 2 pad + 3 + outpad (Wo likewise).  The channel contraction is the caller's gt_gemm product
 *     cols[(b,iy,ix)][(ky*3 + kx)*Cout + co] = sum_ci x[b,iy,ix,ci] w[ci,co,ky,kx]          dense [B H W][9 Cout]
 * and these entry points move between cols and the image in gather form (an output row reads the taps ky with
 * (oy + pad - ky) even and (oy + pad - ky) / 2 in [0, H): at most four of the nine taps per output pixel):
 *   gt_deconv3x3s2_gather_fwd  y = act(dropout(bias + gathered sum)), dense [B,Ho,Wo,Cout]; the mask index of an element is
 *                              its index in y.  pre (optional, y's shape): the sum in front of the dropout -- what the
 *                              backward of GT_ACT_SILU needs.  bias may be NULL.
 *   gt_deconv3x3s2_gather_bwd  dcols [B H W][9 Cout] = dy * act' * mask gathered the other way, 0 where the tap leaves the
 *                              image.  gate: `pre` for GT_ACT_SILU, y for GT_ACT_RELU, ignored (may be NULL) for GT_ACT_NONE;
 *                              the mask is re-drawn from (seed, salt, index).  The caller's products finish the job:
 *                              dx = dcols W^T, dW = x^T dcols.
 *   gt_deconv3x3s2_dbias       db[co] = sum over the output pixels of dy * act' * mask; partial rows in ws
 *                              (>= gt_deconv3x3s2_dbias_ws_bytes), reduced in a fixed order.
 *   gt_deconv3x3s2_check       0 if the shape is implemented; touches no device.
 * Each value is written once by one thread in a fixed summation order: no atomics, bit-identical from run to run.  The
 * caller's stream, no allocation.  Cin % 4 != 0, Cout % 4 != 0 or 2^31 pixels: GT_ENOTSUP; a non-positive size (the output's
 * included), pad < 0, outpad outside {0, 1}, another act, p outside [0, 1): GT_EINVAL; a pointer off a 16-byte boundary:
 * GT_EALIGN; ws too small: GT_EWS.
 * ------------------------------------------------------------------------------------------- */
int gt_deconv3x3s2_check(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pad, int32_t outpad);
int gt_deconv3x3s2_gather_fwd(const float* cols, const float* bias, float* y, float* pre, int32_t B, int32_t H, int32_t W,
                              int32_t Cout, int32_t pad, int32_t outpad, const gt_dropout* drop, int32_t act, void* stream);
int gt_deconv3x3s2_gather_bwd(const float* dy, const float* gate, float* dcols, int32_t B, int32_t H, int32_t W, int32_t Cout,
                              int32_t pad, int32_t outpad, const gt_dropout* drop, int32_t act, void* stream);
int64_t gt_deconv3x3s2_dbias_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout, int32_t pad, int32_t outpad);
int gt_deconv3x3s2_dbias(const float* dy, const float* gate, float* db, int32_t B, int32_t H, int32_t W, int32_t Cout,
                         int32_t pad, int32_t outpad, const gt_dropout* drop, int32_t act, void* ws, int64_t ws_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Graph convolution against a dense per-channel edge tensor: the product of the reference's GraphConvolution
 * (layers.py:153-198, torch.matmul(edge, support.unsqueeze(-1)): B C independent n x n matrix-vector products) and of its
 * autograd backward, for the GCN feature extractor (model.py:376-427).  ABI v21, additive.
 *
 * The edge tensor E [B, C, n, n] arrives as 1..3 CHANNEL GROUPS: dense [B, c_g, n, n] tensors e[g] with sum c_g = C, group 0
 * holding the channels 0 .. c_0 - 1 and so on -- the outputs of the edge encoder as they are, never concatenated.  The
 * vectors S, Y, G, dS are token-major [B, n, C] with a leading dimension >= C (the column c of row (b, i) at (b n + i) ld + c),
 * so the products h W around them are plain row-major GEMMs.  The two descriptors are HOST structs handed over by pointer, as
 * gt_dropout is; they are read during the call and reach the kernels by value, so they may be reused or freed on return.
 *   gt_graphconv_fwd       Y[b,i,c] = act(sum_j E[b,c,i,j] S[b,j,c] + bias[c]);  act: GT_ACT_NONE | GT_ACT_RELU, bias may be NULL.
 *   gt_graphconv_bwd_data  dS[b,j,c] = sum_i E[b,c,i,j] G[b,i,c]: the transposed product, E read in its row-major order.
 *   gt_graphconv_bwd_edge  dE_g[b,c,i,j] = sum_{l < n_pairs} g[l][b,i,c] s[l][b,j,c]: the rank-P update of a stack of P layers
 *                          that share E, written once.  All g[l] share ldg, all s[l] share lds.  A group whose e[g] is NULL is
 *                          skipped (its channels are still counted): the raw Laplacian when the edge input needs no gradient.
 * Every n from 1 to GT_GRAPHCONV_MAX_N; 16-byte accesses when n % 4 == 0 and the group pointers are 16-byte aligned, dword
 * accesses otherwise (a (b, c) slice starts at element (b c_g + c) n^2: off a 16-byte boundary for most other n).  64-bit
 * offsets.  fp32, no atomics, fixed summation orders: bit-identical from run to run.  The caller's stream, no allocation, no
 * scratch.  n_groups outside 1..3, c_g <= 0, sum c_g != C, a leading dimension < C, B / n / C / n_pairs < 1, a NULL tensor
 * or descriptor (fwd / bwd_data: any group; bwd_edge: any g[l], s[l] with l < n_pairs), another act: GT_EINVAL.  n > GT_GRAPHCONV_MAX_N,
 * n_pairs > GT_GRAPHCONV_MAX_PAIRS, B or C > 65535: GT_ENOTSUP, decided from the arguments alone, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define GT_GRAPHCONV_MAX_N     8192
#define GT_GRAPHCONV_MAX_PAIRS 8
typedef struct gt_edge_groups {
    float* e[3];                /* group tensors (read-only for fwd / bwd_data); entries past n_groups are ignored */
    int32_t c[3];               /* channels per group */
    int32_t n_groups;           /* 1..3 */
} gt_edge_groups;
typedef struct gt_graph_pairs {
    const float* g[GT_GRAPHCONV_MAX_PAIRS];   /* output gradients G_l [B, n, C], leading dimension ldg */
    const float* s[GT_GRAPHCONV_MAX_PAIRS];   /* supports S_l = h_l W_l [B, n, C], leading dimension lds */
    int32_t n_pairs;
} gt_graph_pairs;
int gt_graphconv_fwd(const gt_edge_groups* E, const float* S, int64_t lds, const float* bias, float* Y, int64_t ldy, int32_t B,
                     int32_t n, int32_t C, int32_t act, void* stream);
int gt_graphconv_bwd_data(const gt_edge_groups* E, const float* G, int64_t ldg, float* dS, int64_t ldds, int32_t B, int32_t n,
                          int32_t C, void* stream);
int gt_graphconv_bwd_edge(const gt_edge_groups* dE, const gt_graph_pairs* pairs, int64_t ldg, int64_t lds, int32_t B, int32_t n, int32_t C,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused masked graph attention: the reference's GraphAttention (layers.py:201-257) and its autograd backward, for the GAT
 * feature extractor (model.py:430-469).  ABI v21, additive.  With h = node W [B, n, F], s = h a[:F], t = h a[F:] (the caller's
 * products; s and t are read at (b n + i) ldst, so an interleaved [B n, 2] pair is ldst = 2):
 *     keep_ij = graph_lap ? |adj_ij| > thresh : adj_ij > 0                                   (strict)
 *     e_ij    = LeakyReLU_alpha(s_i + t_j) where keep_ij, else the reference's literal -9e15
 *     P       = softmax_j(e):  P_ij = keep_ij ? exp(e_ij - L_i) : w0_i,   L_i = logsumexp_{j kept} e_ij
 *               (a row that keeps nothing: every weight is 1/n; then w0_i = 1/n and L_i = log n; every other row: w0_i = 0)
 *     Pm_ij   = P_ij m_ij,  m_ij = 0 or 1/(1-p): ONE keep decision per (seed, salt, b, i, j), shared by all entry points
 *     U       = Pm h;   out = relu?(concat ? ELU(U) : U)
 *   gt_graphattn_mask      adj [B, n, n] with adj_ij at ((b n + i) n + j) adj_stride (1: dense; E: channel 0 of an edge tensor
 *                          [B, n, n, E], read in place) -> bits, bitsT: [B, n, ceil(n/64)] 64-bit words, bit (j mod 64) of word (b, i, j / 64)
 *                          = keep_ij and bit (i mod 64) of word (b, j, i / 64) = keep_ij, padding bits 0; w0 [B, n].  Once per
 *                          layer stack: adj is read only here, in row order.
 *   gt_graphattn_fwd       L [B, n], then U (may be NULL: not stored) and out, leading dimension ldo.
 *   gt_graphattn_bwd_row   dU = dout * act'(U) [B, n, lddu] (written), ds_i = sum_j dz_ij (at (b n + i) ldst) with
 *                          dz_ij = P_ij (m_ij dU_i.h_j - dU_i.U_i) LeakyReLU'(s_i + t_j) keep_ij, and the partial column sums
 *                          dt_part[b, r, j] = sum over the rows i of the 64-row tile r of dz_ij: [B, ceil(n/64), n] floats.
 *                          dout and U share the leading dimension ldo.
 *   gt_graphattn_bwd_col   dt_j = sum_r dt_part[b, r, j] (in tile order, written at (b n + j) ldst) and
 *                          dH_j = sum_i Pm_ij dU_i + ds_j a[:F]^T + dt_j a[F:]^T, over the transposed bits; a is [2F].
 *   gt_graphattn_weights   Pm [B, n, n] dense, for a caller who wants the attention weights.
 * fp32 arithmetic whatever the GEMM precision mode, v_mfma_f32_16x16x4_f32 for the products, no atomics, fixed summation
 * orders: bit-identical from run to run.  The caller's stream, no allocation.  B, n, F < 1, ldst < 1, a leading dimension
 * < F, a NULL tensor, adj_stride < 1, a dropout p >= 1 or without a seed: GT_EINVAL.  F % 4 != 0, F > GT_GRAPHATTN_MAX_F,
 * n > GT_GRAPHATTN_MAX_N, B > 65535, alpha < 0 (fwd): GT_ENOTSUP.  Decided from the arguments alone, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define GT_GRAPHATTN_MAX_N 8192
#define GT_GRAPHATTN_MAX_F 256
int gt_graphattn_mask(const float* adj, int64_t adj_stride, void* bits, void* bitsT, float* w0, int32_t B, int32_t n,
                      int32_t graph_lap, float thresh, void* stream);
int gt_graphattn_fwd(const void* bits, const float* w0, const float* s, const float* t, int64_t ldst, const float* h,
                     int64_t ldh, float* U, float* out, int64_t ldo, float* L, int32_t B, int32_t n, int32_t F,
                     float alpha, int32_t concat, int32_t relu, const gt_dropout* drop, void* stream);
int gt_graphattn_bwd_row(const void* bits, const float* s, const float* t, int64_t ldst, const float* L,
                         const float* dout, const float* U, int64_t ldo, const float* h, int64_t ldh, float* dU,
                         int64_t lddu, float* ds, float* dt_part, int32_t B, int32_t n, int32_t F, float alpha,
                         int32_t concat, int32_t relu, const gt_dropout* drop, void* stream);
int gt_graphattn_bwd_col(const void* bitsT, const float* w0, const float* s, const float* t, int64_t ldst,
                         const float* L, const float* dU, int64_t lddu, const float* a, const float* ds,
                         const float* dt_part, float* dt, float* dH, int64_t lddh, int32_t B, int32_t n, int32_t F,
                         float alpha, const gt_dropout* drop, void* stream);
int gt_graphattn_weights(const void* bits, const float* w0, const float* s, const float* t, int64_t ldst, const float* L,
                         float* Pm, int32_t B, int32_t n, float alpha, const gt_dropout* drop, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Causal linear attention (gt_causal.hip; reference layers.py:736-762), additive to ABI 21.  Per (sample, head) on head
 * tiles Q, K, V [B*n, h, DP] (token-major, zero pad columns) and an optional keep vector keep [B, n] of bytes (0 = the key /
 * value token is dropped; NULL keeps all):
 *     k^_j = keep_j k_j / n,  v^_j = keep_j v_j,  S_i = sum_{j<=i} k^_j v^_j^T,  z_i = sum_{j<=i} k^_j
 *     den_i = sum_d (z_i[d] + eps) q_i[d],        O_i = S_i^T q_i / den_i
 * i.e. A = tril(Q K^^T), O = A V^ / (rowsum(A) + eps sum_d q).  No attention dropout.  Linear in n: chunks of 64 tokens,
 * three stages per direction (chunk sums, an exclusive scan over the chunks in chunk order, the per-chunk product); neither
 * the n x n matrix nor the [n, DP, DP] running state reaches HBM.
 *   gt_causal_attn_fwd   writes O [B*n, h, DP], den [B, h, n] and `states`: per (sample, head, chunk) the exclusive prefix
 *                        [S_prev (DP x DP) | z_prev (DP)], gt_causal_attn_state_bytes = 4 B h ceil(n / 64) (DP^2 + DP)
 *                        bytes.  The backward READS them (they are kept, not recomputed): the caller keeps the buffer.
 *   gt_causal_attn_bwd   with g_i = dO_i / den_i, c_i = -(dO_i . O_i) / den_i, R_j = sum_{i>=j} q_i g_i^T, r_j = sum_{i>=j}
 *                        c_i q_i:  dQ_i = S_i g_i + c_i (z_i + eps),  dK_j = keep_j / n (R_j v^_j + r_j),  dV_j = keep_j
 *                        R_j^T k^_j.  D <= DP is the number of real columns: columns D .. DP-1 of dQ, dK, dV are written
 *                        as exact zeros, and so are the rows of dK, dV at dropped tokens.  Scratch `ws` of
 *                        gt_causal_attn_bwd_ws_bytes = state bytes + 4 B h n bytes.
 * DP in {16, 32, 48, 64, 96} and {20, 36, 52, 68, 100}; any other width: GT_ENOTSUP (the size queries return 0), never a
 * nearest instance.  fp32 arithmetic on v_mfma_f32_16x16x4_f32 whatever the GEMM precision mode.  Plain pointers, the caller's
 * stream, no allocation, no synchronisation, graph-capturable; no atomics, fixed summation orders: bit-identical from run to
 * run.  Tiles and their gradients 16-byte aligned.  B, h > 65535 or a non-positive size: GT_EINVAL; a short buffer: GT_EWS.
 * ------------------------------------------------------------------------------------------- */
int64_t gt_causal_attn_state_bytes(int32_t B, int32_t n, int32_t h, int32_t DP);
int64_t gt_causal_attn_bwd_ws_bytes(int32_t B, int32_t n, int32_t h, int32_t DP);
int gt_causal_attn_fwd(const float* Q, const float* K, const float* V, const uint8_t* keep, float* O, float* den, int32_t B,
                       int32_t n, int32_t h, int32_t DP, float eps, float* states, int64_t states_bytes, void* stream);
int gt_causal_attn_bwd(const float* dO, const float* O, const float* Q, const float* K, const float* V, const uint8_t* keep,
                       const float* den, const float* states, float* dQ, float* dK, float* dV, int32_t B, int32_t n,
                       int32_t h, int32_t DP, int32_t D, float eps, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GT_HIP_H */
