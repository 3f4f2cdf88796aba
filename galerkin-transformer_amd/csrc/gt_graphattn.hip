// Fused masked graph attention (gfx950): the GAT layer of the reference (GraphAttention, layers.py:201-257; GAT,
// model.py:430-469).  The scores are rank-1 before the LeakyReLU,
//     e_ij = LeakyReLU(s_i + t_j),   s = h a[:F],  t = h a[F:],   h = node W,
// so nothing here forms an n x n float tensor: a pass reads two length-n vectors, ONE BIT per pair and [64, F] tiles of h.
//   mask      : adj [B, n, n] (element stride es: channel 0 of an edge tensor [B, n, n, E] in place) -> the keep bits as 64-bit words, row-major (bit j - 64c of word (b, i, c)) and transposed
//               (bit i - 64c of word (b, j, c)), and w0[b,i] = the weight of a MASKED entry of row i: 0, or 1/n when the row
//               keeps nothing (the softmax over the reference's literal -9e15 is uniform there).  A block owns 64 rows and
//               walks the 64-column tiles: a wave ballots one row at a time (a 256-byte read), the 64 row words meet in LDS
//               and thread t gathers bit t of each into the transposed word -- adj is read once, in row order.
//   stats     : L[b,i] = logsumexp_j over the kept scores of row i (log n for a row that keeps nothing), one wave per row, the
//               exact maximum first (LeakyReLU is monotone: the row maximum is LeakyReLU(s_i + max kept t_j)), then the sum.
//   apply     : the product kernel, forward (U = Pm h) and column pass (dH = Pm^T dU) from ONE template.  A block owns 64
//               "owned" indices (rows i forward, columns j in the column pass) x 64 feature columns and streams the other
//               index in chunks of 64: the [64, 64] tile of h (dU) goes through LDS as the B operand of
//               v_mfma_f32_16x16x4_f32, and each lane builds its A operand -- Pm[owned = lane & 15][streamed = 4 ks + (lane >> 4)]
//               = keep ? exp(e - L_i) : w0_i, times the dropout multiplier -- in registers from one mask word, never in LDS.
//   bwd_row   : per 64 rows, ALL F: dU = dout * act'(U) (stored for the column pass), then per 64-column chunk
//               dPm = dU h^T on the MFMA (A = the dU rows in registers, B = the h chunk in LDS), in TWO sweeps: the first
//               sums D_i = sum_j Pm_ij dPm_ij, the second forms dz_ij = P_ij (m_ij dPm_ij - D_i) LeakyReLU'(s_i + t_j) keep_ij
//               in the accumulator layout; ds_i = sum_j dz_ij leaves by a shuffle reduction, and the column sums of the
//               block's 64 rows go to dt_part[b, row tile, j].
//   bwd_col   : `apply` over the transposed bits; its epilogue sums dt_j = sum_tiles dt_part in tile order and stores
//               dH_j + ds_j a1^T + dt_j a2^T.
//   weights   : Pm [B, n, n] materialised with the same functions, for a caller who wants the weights.
// fp32 throughout, expf / logf (not the hardware approximations), no atomics, fixed summation orders: bit-identical from
// run to run.  The caller's stream, no allocation.  64-bit offsets.
#include "gt_common.h"

namespace gt {

constexpr int GA_THREADS = 256;
constexpr int GA_TILE = 64;            // owned indices per block = streamed indices per chunk = bits per mask word
constexpr int GA_FT = 64;              // feature columns per block of the apply kernel
constexpr int GA_FTP = GA_FT + 16;     // LDS pitch of its tile: the four k rows of a B fragment land 16 banks apart

__device__ __forceinline__ float ga_lrelu(float x, float alpha) { return x > 0.f ? x : alpha * x; }

// THE dropout keep decision of entry (b, i, j): `row` = b n + i (< 2^30), a row key hashed once more with the column
__device__ __forceinline__ float ga_dropmul(const DropDev& d, uint32_t key, uint32_t row, uint32_t j) {
    return drop_hash(fmix32(row * 0x9e3779b1u + key), j) >= d.thresh ? d.scale : 0.f;
}

// P_ij before dropout: a kept entry exp(e_ij - L_i); a masked one w0_i inside the matrix and 0 in the padding
__device__ __forceinline__ float ga_weight(bool bit, bool inside, float si, float tj, float Li, float w0i, float alpha) {
    const float p = expf(ga_lrelu(si + tj, alpha) - Li);
    return bit ? p : (inside ? w0i : 0.f);
}

__global__ __launch_bounds__(GA_THREADS) void ga_mask_kernel(const float* __restrict__ adj, int64_t es, uint64_t* __restrict__ bits,
                                                             uint64_t* __restrict__ bitsT, float* __restrict__ w0, int n, int W,
                                                             int lap, float thresh) {
    __shared__ uint64_t rowm[GA_TILE];
    const int b = blockIdx.y, i0 = blockIdx.x * GA_TILE, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bn = (int64_t)b * n;
    uint64_t any = 0;                               // threads 0..63: the OR of row i0 + tid's words
    for (int c = 0; c < W; ++c) {
        const int col = c * GA_TILE + lane;
        float v[16];                                // sixteen rows in flight, then the ballots
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = i0 + 16 * wave + rr;    // wave-uniform
            v[rr] = (row < n && col < n) ? adj[((bn + row) * n + col) * es] : 0.f;
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = i0 + 16 * wave + rr;
            const uint64_t word = __ballot(lap ? fabsf(v[rr]) > thresh : v[rr] > 0.f);
            if (lane == 0) {
                rowm[16 * wave + rr] = word;
                if (row < n) bits[(bn + row) * W + c] = word;
            }
        }
        __syncthreads();
        if (tid < GA_TILE) {
            any |= rowm[tid];
            uint64_t cw = 0;
#pragma unroll 8
            for (int i = 0; i < GA_TILE; ++i) cw |= ((rowm[i] >> tid) & 1ull) << i;
            if (col < n) bitsT[(bn + col) * W + blockIdx.x] = cw;          // (tid == lane here)
        }
        __syncthreads();
    }
    if (tid < GA_TILE && i0 + tid < n) w0[bn + i0 + tid] = any ? 0.f : 1.f / (float)n;
}

__global__ __launch_bounds__(GA_THREADS) void ga_stats_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ s,
                                                              const float* __restrict__ t, int64_t ldst, float* __restrict__ L,
                                                              int n, int W, float alpha) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (row >= n) return;                           // wave-uniform, and the kernel has no barrier
    const int64_t bn = (int64_t)b * n;
    const uint64_t* __restrict__ bw = bits + (bn + row) * W;
    const float* __restrict__ tb = t + bn * ldst;
    float tmax = 0.f;
    bool any = false;
    for (int c = 0; c < W; ++c)
        if ((bw[c] >> lane) & 1ull) {
            const float tj = tb[(int64_t)(c * GA_TILE + lane) * ldst];
            tmax = any ? fmaxf(tmax, tj) : tj;
            any = true;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(tmax, o, 64);
        const int oa = __shfl_xor((int)any, o, 64);
        tmax = (any && oa) ? fmaxf(tmax, om) : (oa ? om : tmax);
        any = any || oa;
    }
    if (!any) {
        if (lane == 0) L[bn + row] = logf((float)n);
        return;
    }
    const float si = s[(bn + row) * ldst], m = ga_lrelu(si + tmax, alpha);
    float sum = 0.f;
    for (int c = 0; c < W; ++c)
        if ((bw[c] >> lane) & 1ull) sum += expf(ga_lrelu(si + tb[(int64_t)(c * GA_TILE + lane) * ldst], alpha) - m);
    sum = wave_sum(sum);
    if (lane == 0) L[bn + row] = m + logf(sum);
}

// rows r0 .. r0 + 63 of X [n, ldx], columns c0 .. c0 + width - 1 (width % 4 == 0) -> dst[r * pitch + c]; rows at or past n and
// columns at or past F are zero-filled
template <bool VEC>
__device__ __forceinline__ void ga_stage(const float* __restrict__ X, int64_t ldx, int r0, int n, int c0, int width, int F,
                                         float* __restrict__ dst, int pitch) {
    if (VEC) {
        const int wq = width >> 2;
        for (int idx = threadIdx.x; idx < GA_TILE * wq; idx += GA_THREADS) {
            const int r = idx / wq, q = idx - r * wq, col = c0 + 4 * q;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < n && col < F) v = *reinterpret_cast<const f32x4*>(X + (int64_t)(r0 + r) * ldx + col);
            *reinterpret_cast<f32x4*>(dst + r * pitch + 4 * q) = v;
        }
    } else {
        for (int idx = threadIdx.x; idx < GA_TILE * width; idx += GA_THREADS) {
            const int r = idx / width, q = idx - r * width, col = c0 + q;
            dst[r * pitch + q] = (r0 + r < n && col < F) ? X[(int64_t)(r0 + r) * ldx + col] : 0.f;
        }
    }
}

// The same tile for the apply kernel (width GA_FT), in two halves: global -> registers, registers -> LDS, so that the next
// chunk's loads fly while the current one is multiplied.  Thread t holds the elements idx = t + 256 k.
template <bool VEC>
__device__ __forceinline__ void ga_fetch(const float* __restrict__ X, int64_t ldx, int r0, int n, int c0, int F, f32x4 (&reg)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (VEC) {
            const int idx = threadIdx.x + GA_THREADS * k, r = idx >> 4, col = c0 + 4 * (idx & 15);
            reg[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r0 + r < n && col < F) reg[k] = *reinterpret_cast<const f32x4*>(X + (int64_t)(r0 + r) * ldx + col);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = threadIdx.x + GA_THREADS * (4 * k + e), r = idx >> 6, col = c0 + (idx & 63);
                reg[k][e] = (r0 + r < n && col < F) ? X[(int64_t)(r0 + r) * ldx + col] : 0.f;
            }
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void ga_put(const f32x4 (&reg)[4], float* __restrict__ dst) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (VEC) {
            const int idx = threadIdx.x + GA_THREADS * k;
            *reinterpret_cast<f32x4*>(dst + (idx >> 4) * GA_FTP + 4 * (idx & 15)) = reg[k];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = threadIdx.x + GA_THREADS * (4 * k + e);
                dst[(idx >> 6) * GA_FTP + (idx & 63)] = reg[k][e];
            }
        }
    }
}

// TRANS = false, forward:     owned = rows i,    streamed = columns j, X = h;   U = Pm h, out = act(U)
// TRANS = true,  column pass: owned = columns j, streamed = rows i,    X = dU;  dH = Pm^T dU + ds a1^T + dt a2^T
template <bool TRANS, bool VEC>
__global__ __launch_bounds__(GA_THREADS) void ga_apply_kernel(
    const uint64_t* __restrict__ bits, const float* __restrict__ s, const float* __restrict__ t, int64_t ldst,
    const float* __restrict__ L, const float* __restrict__ w0, const float* __restrict__ X, int64_t ldx, float* __restrict__ Y,
    float* __restrict__ Y2, int64_t ldy, const float* __restrict__ avec, const float* __restrict__ ds,
    const float* __restrict__ dtp, float* __restrict__ dt, int n, int W, int F, float alpha, int concat, int relu, DropDev drop) {
    __shared__ __attribute__((aligned(16))) float xs[GA_TILE * GA_FTP];
    __shared__ float sv[GA_TILE], lv[GA_TILE], zv[GA_TILE];     // per chunk: the streamed score vector; TRANS: L and w0 too
    __shared__ float dsv[GA_TILE], dtv[GA_TILE];                // TRANS: ds, dt of the owned columns
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ii = lane & 15, kq = lane >> 4;
    const int b = blockIdx.z, f0 = blockIdx.y * GA_FT, o0 = blockIdx.x * GA_TILE;
    const int64_t bn = (int64_t)b * n;
    const int own = o0 + 16 * wave + ii, ownc = min(own, n - 1);          // a row past the end recomputes the last one, unstored
    const float ov = (TRANS ? t : s)[(bn + ownc) * ldst];
    const float oL = TRANS ? 0.f : L[bn + ownc], oz = TRANS ? 0.f : w0[bn + ownc];
    const uint64_t* __restrict__ bw = bits + (bn + ownc) * W;
    const float* __restrict__ Xb = X + bn * ldx;
    const float* __restrict__ strv = (TRANS ? s : t) + bn * ldst;
    const uint32_t key = drop_key_dev(drop);
    const int ntv = min(4, (F - f0 + 15) >> 4);                           // 16-column tiles with a real column (block-uniform)
    if (TRANS && tid < GA_TILE) {
        const int j = o0 + tid;
        float a = 0.f, d = 0.f;
        if (j < n) {
            a = ds[(bn + j) * ldst];
            for (int rt = 0; rt < W; ++rt) d += dtp[((int64_t)b * W + rt) * n + j];      // tile order
            if (blockIdx.y == 0) dt[(bn + j) * ldst] = d;
        }
        dsv[tid] = a;
        dtv[tid] = d;
    }
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 xreg[4];
    float vreg[3] = {0.f, 0.f, 0.f};                // threads 0..63: the streamed vectors of the chunk in flight
    auto fetch = [&](int c) {
        const int q0 = c * GA_TILE;
        ga_fetch<VEC>(Xb, ldx, q0, n, f0, F, xreg);
        if (tid < GA_TILE) {
            const int q = q0 + tid;
            const bool v = q < n;
            vreg[0] = v ? strv[(int64_t)q * ldst] : 0.f;
            if (TRANS) {
                vreg[1] = v ? L[bn + q] : 0.f;
                vreg[2] = v ? w0[bn + q] : 0.f;
            }
        }
    };
    fetch(0);
    for (int c = 0; c < W; ++c) {
        const int q0 = c * GA_TILE;
        __syncthreads();                            // the previous chunk has been read
        ga_put<VEC>(xreg, xs);
        if (tid < GA_TILE) {
            sv[tid] = vreg[0];
            if (TRANS) {
                lv[tid] = vreg[1];
                zv[tid] = vreg[2];
            }
        }
        __syncthreads();
        if (c + 1 < W) fetch(c + 1);                // in flight under this chunk's products
        const uint64_t word = bw[c];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int kk = 4 * ks + kq, q = q0 + kk;
            const bool bit = (word >> kk) & 1ull, inside = q < n;
            float p;
            if (TRANS) {
                p = ga_weight(bit, inside, sv[kk], ov, lv[kk], zv[kk], alpha);
                if (drop.thresh) p *= ga_dropmul(drop, key, (uint32_t)(bn + q), (uint32_t)own);
            } else {
                p = ga_weight(bit, inside, ov, sv[kk], oL, oz, alpha);
                if (drop.thresh) p *= ga_dropmul(drop, key, (uint32_t)(bn + own), (uint32_t)q);
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                if (nt < ntv) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, xs[kk * GA_FTP + 16 * nt + ii], acc[nt], 0, 0, 0);
        }
    }
    // accumulator element r of tile nt: owned index o0 + 16 wave + 4 kq + r, feature column f0 + 16 nt + ii
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int col = f0 + 16 * nt + ii;
        if (nt >= ntv || col >= F) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ol = 16 * wave + 4 * kq + r, o = o0 + ol;
            if (o >= n) continue;
            const float u = acc[nt][r];
            if (TRANS) {
                Y[(bn + o) * ldy + col] = (u + dsv[ol] * avec[col]) + dtv[ol] * avec[F + col];
            } else {
                if (Y) Y[(bn + o) * ldy + col] = u;
                float v = concat ? (u > 0.f ? u : expm1f(u)) : u;
                if (relu) v = fmaxf(v, 0.f);
                Y2[(bn + o) * ldy + col] = v;
            }
        }
    }
}

// KS: the dU fragments a lane holds, 4 KS >= F.  Two sweeps over the columns with the same MFMA products: the first sums
// D_i = sum_j Pm_ij dPm_ij, the second forms dz with it -- D from the very numbers it is subtracted from, so a row with one
// kept entry (P = 1, dP = D) gives an exact zero, as the reference's softmax backward does.
template <int KS, bool VEC>
__global__ __launch_bounds__(GA_THREADS) void ga_bwd_row_kernel(
    const uint64_t* __restrict__ bits, const float* __restrict__ s, const float* __restrict__ t, int64_t ldst,
    const float* __restrict__ L, const float* __restrict__ dout, const float* __restrict__ U, int64_t ldo,
    const float* __restrict__ h, int64_t ldh, float* __restrict__ dU, int64_t lddu, float* __restrict__ ds,
    float* __restrict__ dtp, int n, int W, int F, int FP, float alpha, int concat, int relu, DropDev drop) {
    extern __shared__ __attribute__((aligned(16))) float ga_smem[];
    float* hs = ga_smem;                            // the h chunk [64][FP]
    float* tv = hs + GA_TILE * FP;                  // t of the chunk [64]
    float* red = tv + GA_TILE;                      // the waves' column sums [4][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ii = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, i0 = blockIdx.x * GA_TILE;
    const int64_t bn = (int64_t)b * n;
    const uint32_t key = drop_key_dev(drop);
    float a[KS];
    {
        const int row = i0 + 16 * wave + ii;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int f = 4 * ks + kq;
            float du = 0.f;
            if (row < n && f < F) {
                const float u = U[(bn + row) * ldo + f], g = dout[(bn + row) * ldo + f];
                du = g;
                if (relu) du = u > 0.f ? g : 0.f;                     // relu(elu(u)) > 0 <=> u > 0
                else if (concat) du = u > 0.f ? g : g * expf(u);
                dU[(bn + row) * lddu + f] = du;
            }
            a[ks] = du;
        }
    }
    float sr[4], Lr[4], Dr[4], racc[4];
    const uint64_t* bwr[4];
    bool vr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = i0 + 16 * wave + 4 * kq + r, rc = min(row, n - 1);
        vr[r] = row < n;
        sr[r] = s[(bn + rc) * ldst];
        Lr[r] = L[bn + rc];
        Dr[r] = 0.f;
        bwr[r] = bits + (bn + rc) * W;
        racc[r] = 0.f;
    }
    const float* __restrict__ hb = h + bn * ldh;
#pragma unroll 1
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int c = 0; c < W; ++c) {
            const int q0 = c * GA_TILE;
            __syncthreads();
            ga_stage<VEC>(hb, ldh, q0, n, 0, F, F, hs, FP);
            if (tid < GA_TILE) tv[tid] = q0 + tid < n ? t[(bn + q0 + tid) * ldst] : 0.f;
            __syncthreads();
            uint64_t word[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) word[r] = vr[r] ? bwr[r][c] : 0ull;
#pragma unroll 1
            for (int ct = 0; ct < 4; ++ct) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const float* hp = hs + (16 * ct + ii) * FP + kq;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    if (4 * ks < F) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], hp[4 * ks], acc, 0, 0, 0);
                // acc[r] = dPm[row i0 + 16 wave + 4 kq + r][column q0 + 16 ct + ii]
                const int jl = 16 * ct + ii, j = q0 + jl;
                const float tj = tv[jl];
                float colsum = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = 0.f;
                    if ((word[r] >> jl) & 1ull) {
                        const float x = sr[r] + tj, P = expf(ga_lrelu(x, alpha) - Lr[r]);
                        float dp = acc[r];
                        if (drop.thresh) dp *= ga_dropmul(drop, key, (uint32_t)(bn + i0 + 16 * wave + 4 * kq + r), (uint32_t)j);
                        v = sweep == 0 ? P * dp : P * (dp - Dr[r]) * (x > 0.f ? 1.f : alpha);
                    }
                    racc[r] += v;
                    colsum += v;
                }
                if (sweep) {
                    colsum += __shfl_xor(colsum, 16, 64);
                    colsum += __shfl_xor(colsum, 32, 64);
                    if (kq == 0) red[wave * GA_TILE + jl] = colsum;
                }
            }
            if (sweep) {
                __syncthreads();
                if (tid < GA_TILE && q0 + tid < n)
                    dtp[((int64_t)b * W + blockIdx.x) * n + q0 + tid] =
                        ((red[tid] + red[GA_TILE + tid]) + red[2 * GA_TILE + tid]) + red[3 * GA_TILE + tid];
            }
        }
        // the row sums of the sweep, over the 16 lanes that share the rows: D after the first, ds after the second
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = racc[r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
            if (sweep == 0) Dr[r] = v;
            else if (ii == 0 && vr[r]) ds[(bn + i0 + 16 * wave + 4 * kq + r) * ldst] = v;
            racc[r] = 0.f;
        }
    }
}

__global__ __launch_bounds__(GA_THREADS) void ga_weights_kernel(const uint64_t* __restrict__ bits, const float* __restrict__ s,
                                                                const float* __restrict__ t, int64_t ldst,
                                                                const float* __restrict__ L, const float* __restrict__ w0,
                                                                float* __restrict__ Pm, int n, int W, float alpha, DropDev drop) {
    const int j = blockIdx.x * GA_THREADS + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    if (j >= n) return;
    const int64_t bn = (int64_t)b * n;
    const bool bit = (bits[(bn + i) * W + (j >> 6)] >> (j & 63)) & 1ull;
    float p = ga_weight(bit, true, s[(bn + i) * ldst], t[(bn + j) * ldst], L[bn + i], w0[bn + i], alpha);
    if (drop.thresh) p *= ga_dropmul(drop, drop_key_dev(drop), (uint32_t)(bn + i), (uint32_t)j);
    Pm[(bn + i) * n + j] = p;
}

// ---- argument checks shared by the entry points; 0, GT_EINVAL or GT_ENOTSUP, nothing launched on a refusal
static int ga_check_n(int32_t B, int32_t n) {
    if (B < 1 || n < 1) return GT_EINVAL;
    if (n > GT_GRAPHATTN_MAX_N || B > 65535) return GT_ENOTSUP;
    return 0;
}
static int ga_check(int32_t B, int32_t n, int32_t F, int64_t ldst, const gt_dropout* drop) {
    if (B < 1 || n < 1 || F < 1 || ldst < 1) return GT_EINVAL;
    if (drop && drop->p > 0.f && (!(drop->p < 1.f) || !drop->seed)) return GT_EINVAL;
    if ((F & 3) || F > GT_GRAPHATTN_MAX_F) return GT_ENOTSUP;
    return ga_check_n(B, n);
}
static int ga_words(int n) { return ceil_div(n, GA_TILE); }

template <bool TRANS, typename... A>
static void ga_apply_launch(bool vec, dim3 grid, hipStream_t st, A... args) {
    if (vec) hipLaunchKernelGGL((ga_apply_kernel<TRANS, true>), grid, dim3(GA_THREADS), 0, st, args...);
    else hipLaunchKernelGGL((ga_apply_kernel<TRANS, false>), grid, dim3(GA_THREADS), 0, st, args...);
}

template <int KS, typename... A>
static int ga_row_launch(bool vec, dim3 grid, size_t smem, hipStream_t st, A... args) {
    if (vec) {
        if (int rc = allow_big_lds<ga_bwd_row_kernel<KS, true>>(smem)) return rc;
        hipLaunchKernelGGL((ga_bwd_row_kernel<KS, true>), grid, dim3(GA_THREADS), smem, st, args...);
    } else {
        if (int rc = allow_big_lds<ga_bwd_row_kernel<KS, false>>(smem)) return rc;
        hipLaunchKernelGGL((ga_bwd_row_kernel<KS, false>), grid, dim3(GA_THREADS), smem, st, args...);
    }
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" int gt_graphattn_mask(const float* adj, int64_t adj_stride, void* bits, void* bitsT, float* w0, int32_t B, int32_t n,
                                 int32_t graph_lap, float thresh, void* stream) {
    if (!adj || !bits || !bitsT || !w0 || adj_stride < 1) return GT_EINVAL;
    if (int rc = ga_check_n(B, n)) return rc;
    const int W = ga_words(n);
    hipLaunchKernelGGL(ga_mask_kernel, dim3(W, B), dim3(GA_THREADS), 0, (hipStream_t)stream, adj, adj_stride, (uint64_t*)bits,
                       (uint64_t*)bitsT, w0, n, W, graph_lap ? 1 : 0, thresh);
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_graphattn_fwd(const void* bits, const float* w0, const float* s, const float* t, int64_t ldst, const float* h,
                                int64_t ldh, float* U, float* out, int64_t ldo, float* L, int32_t B, int32_t n, int32_t F,
                                float alpha, int32_t concat, int32_t relu, const gt_dropout* drop, void* stream) {
    if (!bits || !w0 || !s || !t || !h || !out || !L) return GT_EINVAL;
    if (int rc = ga_check(B, n, F, ldst, drop)) return rc;
    if (ldh < F || ldo < F) return GT_EINVAL;
    if (!(alpha >= 0.f)) return GT_ENOTSUP;         // the statistics pass takes the row maximum through a monotone LeakyReLU
    const int W = ga_words(n);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ga_stats_kernel, dim3(ceil_div(n, 4), B), dim3(GA_THREADS), 0, st, (const uint64_t*)bits, s, t, ldst, L, n,
                       W, alpha);
    GT_LAUNCH_CHECK();
    const bool vec = (ldh & 3) == 0 && !misaligned16(h);
    ga_apply_launch<false>(vec, dim3(W, ceil_div(F, GA_FT), B), st, (const uint64_t*)bits, s, t, ldst, (const float*)L, w0, h, ldh,
                           U, out, ldo, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr,
                           (int)n, W, (int)F, alpha, concat ? 1 : 0, relu ? 1 : 0, make_drop(drop));
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_graphattn_bwd_row(const void* bits, const float* s, const float* t, int64_t ldst, const float* L,
                                    const float* dout, const float* U, int64_t ldo, const float* h, int64_t ldh, float* dU,
                                    int64_t lddu, float* ds, float* dt_part, int32_t B, int32_t n, int32_t F, float alpha,
                                    int32_t concat, int32_t relu, const gt_dropout* drop, void* stream) {
    if (!bits || !s || !t || !L || !dout || !U || !h || !dU || !ds || !dt_part) return GT_EINVAL;
    if (int rc = ga_check(B, n, F, ldst, drop)) return rc;
    if (ldo < F || ldh < F || lddu < F) return GT_EINVAL;
    const int W = ga_words(n);
    const int FP = ((F >> 2) & 1) ? F : F + 4;      // pitch = 4 x odd: the 16 rows of a B fragment fall on 16 distinct bank quads
    const size_t smem = ((size_t)GA_TILE * FP + 5 * GA_TILE) * sizeof(float);
    const bool vec = (ldh & 3) == 0 && !misaligned16(h);
    const dim3 grid(W, B);
    const hipStream_t st = (hipStream_t)stream;
    const DropDev dd = make_drop(drop);
    const int c = concat ? 1 : 0, r = relu ? 1 : 0;
    int rc;
    if (F <= 32)
        rc = ga_row_launch<8>(vec, grid, smem, st, (const uint64_t*)bits, s, t, ldst, L, dout, U, ldo, h, ldh, dU, lddu, ds, dt_part,
                              (int)n, W, (int)F, FP, alpha, c, r, dd);
    else if (F <= 96)
        rc = ga_row_launch<24>(vec, grid, smem, st, (const uint64_t*)bits, s, t, ldst, L, dout, U, ldo, h, ldh, dU, lddu, ds, dt_part,
                               (int)n, W, (int)F, FP, alpha, c, r, dd);
    else
        rc = ga_row_launch<64>(vec, grid, smem, st, (const uint64_t*)bits, s, t, ldst, L, dout, U, ldo, h, ldh, dU, lddu, ds, dt_part,
                               (int)n, W, (int)F, FP, alpha, c, r, dd);
    if (rc) return rc;
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_graphattn_bwd_col(const void* bitsT, const float* w0, const float* s, const float* t, int64_t ldst,
                                    const float* L, const float* dU, int64_t lddu, const float* a, const float* ds,
                                    const float* dt_part, float* dt, float* dH, int64_t lddh, int32_t B, int32_t n, int32_t F,
                                    float alpha, const gt_dropout* drop, void* stream) {
    if (!bitsT || !w0 || !s || !t || !L || !dU || !a || !ds || !dt_part || !dt || !dH) return GT_EINVAL;
    if (int rc = ga_check(B, n, F, ldst, drop)) return rc;
    if (lddu < F || lddh < F) return GT_EINVAL;
    const int W = ga_words(n);
    const bool vec = (lddu & 3) == 0 && !misaligned16(dU);
    ga_apply_launch<true>(vec, dim3(W, ceil_div(F, GA_FT), B), (hipStream_t)stream, (const uint64_t*)bitsT, s, t, ldst, L, w0, dU,
                          lddu, dH, (float*)nullptr, lddh, a, ds, dt_part, dt, (int)n, W, (int)F, alpha, 0, 0, make_drop(drop));
    GT_LAUNCH_CHECK();
    return 0;
}

extern "C" int gt_graphattn_weights(const void* bits, const float* w0, const float* s, const float* t, int64_t ldst, const float* L,
                                    float* Pm, int32_t B, int32_t n, float alpha, const gt_dropout* drop, void* stream) {
    if (!bits || !w0 || !s || !t || !L || !Pm) return GT_EINVAL;
    if (int rc = ga_check(B, n, 4, ldst, drop)) return rc;
    hipLaunchKernelGGL(ga_weights_kernel, dim3(ceil_div(n, GA_THREADS), n, B), dim3(GA_THREADS), 0, (hipStream_t)stream,
                       (const uint64_t*)bits, s, t, ldst, L, w0, Pm, (int)n, ga_words(n), alpha, make_drop(drop));
    GT_LAUNCH_CHECK();
    return 0;
}
