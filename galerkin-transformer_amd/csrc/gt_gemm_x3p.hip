// Packed-B side of the split-operand GEMM (gt_x3_core.h): the weight pack, the f16x2 kernel gemm_x3h_kernel and the host side.
// gemm_x3p_kernel (bf16x3) lives in gt_gemm_x3.hip: away from the ring kernels hipcc schedules three of its instances differently.
#include "gt_x3_core.h"

namespace gt {

// ---------------------------------------------------------------------------------------------------------------------
// Packed-B variant: when B is small next to A (a weight matrix against many token rows), every block would split the
// same B values again -- an in-situ ablation put the B split alone at 2.5 of 37.5 ms/step.
// x3_pack_b_kernel splits B ONCE into its three bf16 planes, stored in MFMA fragment order
//     Bp[plane][n-tile of 32][k-stage of 16][lane 0..63] = 8 bf16  (k = 16 ks + 8 (lane >> 5) + e, n = 32 nt + (lane & 31)),
// zero beyond N and K, n-tiles padded to whole 128-column block tiles.  A wave then reads a B fragment of a stage as ONE
// coalesced 1-KB global load straight into the registers the MFMA takes it from (the planes stay L2-resident: 3 x 2 bytes
// per weight), B needs no LDS, and the ring holds A only (8 KB per stage, depth 4).  The fragments of stage kt + 1 are
// requested at the top of iteration kt into a second register set; the counted waits (vector-memory loads retire in
// order) are written out next to the loop.
// Row of the weight behind tile row n (pad48: the tile rows are 64-column head slots holding 48-wide heads, the 16 rows behind
// a head are zero -- gt_gemm_desc.hip: hn_slots; N counts slot rows then), -1: a zero row.
__device__ __forceinline__ int x3_pack_row(int n, int N, int pad48) {
    if (n >= N) return -1;
    if (!pad48) return n;
    const int j = n & 63;
    return j < 48 ? (n >> 6) * 48 + j : -1;
}

__global__ __launch_bounds__(256) void x3_pack_b_kernel(const float* __restrict__ B, int layout_b, int64_t ldb, int N, int K,
                                                        int NT, int KS, u32x4* __restrict__ out, int pad48) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= NT * KS * 64) return;
    const int lane = idx & 63, t = idx >> 6, ks = t % KS, nt = t / KS;
    const int n = nt * 32 + (lane & 31), k0 = ks * 16 + 8 * (lane >> 5);
    const int nr = x3_pack_row(n, N, pad48);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        v[e] = (nr >= 0 && k < K) ? (layout_b == 0 ? B[(int64_t)nr * ldb + k] : B[(int64_t)k * ldb + nr]) : 0.f;
        v[e] *= x3_alt_sign(n);                    // odd rows of the N-side operand enter negated
    }
    uint32_t q[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_pair<3>(v[2 * i], v[2 * i + 1], q[i]);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
        out[(((int64_t)pl * NT + nt) * KS + ks) * 64 + lane] = u32x4{q[0][pl], q[1][pl], q[2][pl], q[3][pl]};
}

// GT_PREC_F16X2: the two fp16 planes of B in the same fragment order, one block per 32-column tile: pass 1 takes the tile's
// amax (its exponent e: amax 2^e in [2^13, 2^14)), pass 2 splits the scaled values.  The exponents follow the planes as NT ints.
__device__ __forceinline__ void x3_pack_b16_tile(const float* __restrict__ B, int layout_b, int64_t ldb, int N, int K, int NT,
                                                 int KS, u32x4* __restrict__ out, int nt, int pad48 = 0) {
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = nt * 32 + (lane & 31);
    const int nr = x3_pack_row(n, N, pad48);
    auto load8 = [&](int ks, float (&v)[8]) {        // this lane's eight k of stage ks (one row n, k contiguous or strided)
        const int k0 = ks * 16 + 8 * (lane >> 5);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            v[e] = (nr >= 0 && k < K) ? (layout_b == 0 ? B[(int64_t)nr * ldb + k] : B[(int64_t)k * ldb + nr]) : 0.f;
        }
    };
    // sixteen waves, a stage each per trip; a wave's stages stay in registers between the two passes when there are at most
    // four of them (K <= 1024), so the weight is read once
    constexpr int KEEP = 4;
    float keep[KEEP][8];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
        const int ks = w + 16 * i;
        if (ks < KS) {
            load8(ks, keep[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(keep[i][e]));
        }
    }
    for (int ks = w + 16 * KEEP; ks < KS; ks += 16) {
        float v[8];
        load8(ks, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if (lane == 0) red[w] = amax;
    __syncthreads();
    amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, red[i]);
    const int ex = (int)((__float_as_uint(amax) >> 23) & 0xff);
    const int e = ex == 0 ? 0 : X3H_TARGET + 127 - ex;            // amax 2^e in [2^13, 2^14); an all-zero tile keeps 1
    const float sc = pow2_f(e) * x3_alt_sign(n);                // odd rows of the N-side operand enter negated
    auto store = [&](int ks, const float (&v)[8]) {
        uint32_t q[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) x3h_split_pair(v[2 * i], v[2 * i + 1], sc, q[i]);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            out[(((int64_t)pl * NT + nt) * KS + ks) * 64 + lane] = u32x4{q[0][pl], q[1][pl], q[2][pl], q[3][pl]};
    };
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
        const int ks = w + 16 * i;
        if (ks < KS) store(ks, keep[i]);
    }
    for (int ks = w + 16 * KEEP; ks < KS; ks += 16) {
        float v[8];
        load8(ks, v);
        store(ks, v);
    }
    if (tid == 0) reinterpret_cast<int*>(out + (int64_t)2 * NT * KS * 64)[nt] = e;
}
__global__ __launch_bounds__(1024) void x3_pack_b16_kernel(const float* __restrict__ B, int layout_b, int64_t ldb, int N, int K,
                                                           int NT, int KS, u32x4* __restrict__ out, int pad48) {
    x3_pack_b16_tile(B, layout_b, ldb, N, K, NT, KS, out, blockIdx.x, pad48);
}
// All the step's weights in ONE launch (round 5, dispatch diet: a step packed 45 weights in 45 launches of 5 - 8 us): block b
// works tile b - start[e] of entry e.
constexpr int X3_PACK_MANY = 64;
struct PackManyP {
    const float* B[X3_PACK_MANY];
    u32x4* out[X3_PACK_MANY];
    int64_t ldb[X3_PACK_MANY];
    int layout_b[X3_PACK_MANY], N[X3_PACK_MANY], K[X3_PACK_MANY], NT[X3_PACK_MANY], KS[X3_PACK_MANY], start[X3_PACK_MANY + 1];
    unsigned char pad48[X3_PACK_MANY];
    int n;
};
__global__ __launch_bounds__(1024) void x3_pack_b16_many_kernel(const PackManyP p) {
    int e = 0;
    while (e + 1 < p.n && (int)blockIdx.x >= p.start[e + 1]) ++e;
    x3_pack_b16_tile(p.B[e], p.layout_b[e], p.ldb[e], p.N[e], p.K[e], p.NT[e], p.KS[e], p.out[e], (int)blockIdx.x - p.start[e],
                     p.pad48[e]);
}

// The GT_PREC_F16X2 twin of gemm_x3p_kernel (gt_gemm_x3.hip; two fp16 planes, three products, see gt_x3_core.h).  TWO bodies, one per
// arithmetic, on purpose: folding both into one templated body changed hipcc's code for the bf16 instances enough to make the
// head-norm launch return different bits from run to run (16 rows of one head, one launch in four; tools: 40 repeated
// launches) while the instruction stream around its counted waits looked the same.  Each body is covered by its own
// repeat-launch test, test_packed_gemm_repeat_launch_bitwise[bf16x3 | f16x2]; the K loop, its lambdas and the counted wait
// are not shared between them.
template <int LA, int HN, int CV, int BN>
__device__ __forceinline__ void x3h_body(const GemmP& p) {
    constexpr int MI = BN == 64 ? 1 : 2;           // 32-row tiles of A per wave
    static_assert(BN == 128 || (BN == 64 && HN == 0 && LA == 0), "the narrow tile serves plain / convolution launches");
    constexpr int R = X3P_R, PLANES = 2;
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
    int ea[MI];                                    // running exponent of this lane's row in tile i (gt_x3_core.h: x3h_*)
#pragma unroll
    for (int i = 0; i < MI; ++i) ea[i] = X3H_E0;
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
    // f16x8 is the MFMA's own operand type: no conversion (= no copy of a register the load has not filled yet) between load and use
    f16x8 bn0[2][PLANES], bn1[2][PLANES];
    auto loadb = [&](int ks, f16x8 (&bn)[2][PLANES]) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                const char* sp = bbase + pl * bplane + ((int64_t)j * p.bp_KS + ks) * 1024;
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(bn[j][pl]) : "v"(voff), "s"(sp));
            }
    };
    // one 32-row tile of A at a time: its fragment is split and goes through its six MFMAs before the next one is read
    // (the planes of ONE tile are live, not of both)
    auto stage = [&](int kt, f16x8 (&bn)[2][PLANES]) {
        const char* sa = smem + (kt % R) * X3R_OP;
        const int kbase = kt * X3_BK + 8 * lh;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            float v[8];
            const int row = wrow + 32 * i + lr;
            x3r_frag<LA>(sa, row, lh, v);
            if (p.a_drop.thresh) x3_mask8<LA>(p.a_drop, akey, p.a_drop_ld, 0, m0 + row, kbase, v);
            // the row's amax of this stage (both k-halves); lower the row's exponent -- and rescale what the lane has
            // accumulated for it -- before anything could overflow
            // (a chain, so that it becomes four v_max3_f32 with |.| modifiers; the other k-half of the row sits in lane
            // l ^ 32: one v_permlane32_swap instead of a ds_bpermute round trip per tile and stage)
            float amax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2]));
            amax = fmaxf(fmaxf(amax, fabsf(v[3])), fabsf(v[4]));
            amax = fmaxf(fmaxf(amax, fabsf(v[5])), fabsf(v[6]));
            amax = xor32_max(fmaxf(amax, fabsf(v[7])));
            const int ex = (int)(__float_as_uint(amax) >> 23);
            const bool need = ex + ea[i] - 127 >= X3H_LIMIT;
            if (__any(need)) {                        // wave-uniform
                const int enew = need ? X3H_TARGET + 127 - ex : ea[i];
                const int d = enew - ea[i];           // <= 0
                const float f = d < -126 ? 0.f : pow2_f(d);   // 2^-127 of a value is below fp32 resolution of the new ones
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] *= f;
                ea[i] = enew;
            }
            const float sv = pow2_f(ea[i]) * (MI == 1 ? tsgn : ((i & 1) ? -1.f : 1.f));
            uint32_t q[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t) x3h_split_pair(v[2 * t], v[2 * t + 1], sv, q[t]);
            f16x8 am[2];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) am[pl] = __builtin_bit_cast(f16x8, u32x4{q[0][pl], q[1][pl], q[2][pl], q[3][pl]});
#pragma unroll
            for (int s = 1; s >= 0; --s)             // h1 g0 + h0 g1, then h0 g0
#pragma unroll
                for (int pa = 0; pa < 2; ++pa) {
                    const int pb = s - pa;
                    if (pb < 0 || pb > 1) continue;
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = mfma32h(bn[j][pb], am[pa], acc[i][j]);
                }
        }
    };
    // Request order of a wave:  B(0) A(0) .. A(R-2) | B(1) A(R-1) | B(2) A(R) | ...   (A = 2 loads, B = 4).
    // Top of iteration kt >= 1: A(kt) and B(kt) must have landed; the only request behind B(kt) is A(kt+R-2): vmcnt(2).
    // The barrier makes every wave's pieces of A(kt) visible and frees slot (kt-1) % R for the request of A(kt+R-1).
    // Tying the set to the statement keeps its MFMAs behind the wait.  Every iteration issues the same requests -- past
    // the end of K the A loader reads the zero line into a free slot and B re-reads its last stage -- so the counts hold
    // to the last stage and no load sits under a branch: a conditional asm load makes hipcc allocate fresh registers for
    // it and COPY them into the set at the join, before the data has arrived (seen in the ISA of a first version).
#define X3P_WAIT_AB(N, bn)                                                                                             \
    asm volatile("s_waitcnt vmcnt(" #N ")\n\ts_barrier"                                                                \
                 : "+v"(bn[0][0]), "+v"(bn[0][1]), "+v"(bn[1][0]), "+v"(bn[1][1])                                      \
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

    // un-scale (row exponent of the lane, tile exponent of the packed columns) with the alternating sign
    {
        const int* ebp = reinterpret_cast<const int*>(reinterpret_cast<const char*>(p.Bp) + 2 * bplane) + ((n0 + wn_u * 64) >> 5);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int et = -(ea[i] + ebp[j]), etc = et < -126 ? -126 : (et > 126 ? 126 : et);
                const float sg = pow2_f(etc) * (MI == 1 ? tsgn : ((i & 1) ? -1.f : 1.f));
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] *= (e & 1) ? -sg : sg;
                if (et != etc) {       // row amax x tile amax below ~2^-100: the rest of the power of two (no cliff)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = ldexpf(acc[i][j][e], et - etc);
                }
            }
    }
    __syncthreads();                               // every wave is done with the ring: its first slots become staging
    if constexpr (HN > 0)
        x3_epilogue_hn<(HN > 0 ? HN : 32), 2>(p, acc, m0 + wm * 64 + lr, n0 + wn * 64 + 4 * lh, lane,
                                               reinterpret_cast<float*>(smem) + wave * X3_HN_STG);
    else
        x3_epilogue<MI>(p, acc, m0 + wrow, n0 + wn * 64, lane, reinterpret_cast<float*>(smem) + wave * X3_EP_STG, 0, 0, 0, 0,
                        bias4);
}

template <int LA, int HN, int CV, int BN = 128>     // CV: 0 plain, 1 implicit 3x3 convolution on A
__global__ __launch_bounds__(256, 3) void gemm_x3h_kernel(const GemmP p) {
    x3h_body<LA, HN, CV, BN>(p);
}

// ---- packed-B path: host side ---------------------------------------------------------------------------------------
// B small next to A (a weight against >= 16384 token rows), three planes, one launch (no batching, split-K, second
// product or row-sum by-product), operands the direct loads can take.
bool x3_packed_ok(const gt_gemm_desc* d, int planes, int split) {
    if (planes != 3 || split != 1 || d->batch0 * d->batch1 != 1 || d->K2 > 0 || d->a_colsum) return false;
    if (d->cv_c > 0 && d->cv_wgrad) return false;
    // below 16384 rows the extra (pack) launch is not paid back -- except for the implicit convolutions, whose K = 9 C makes
    // the product long enough (round 5: the down-scaler chain runs at every batch, no library convolution below B = 3)
    if (d->M < (d->cv_c > 0 ? 1024 : 16384) || d->M < 8 * (int64_t)d->N) return false;
    const bool a16 = (reinterpret_cast<uintptr_t>(d->A) & 15) == 0;
    if (d->cv_c > 0) return a16 && d->layout_a == 0 && (d->cv_c & 15) == 0 && (d->lda <= d->cv_c || (d->lda & 3) == 0);
    if (!a16 || (d->lda & 3)) return false;
    return d->layout_a == 0 ? (d->K & 3) == 0 : (d->M & 3) == 0;
}

static inline int x3p_nt(int N) { return ((N + X3_BN - 1) / X3_BN) * (X3_BN / 32); }
static inline int x3p_ks(int K) { return (K + X3_BK - 1) / X3_BK; }

int64_t x3_packed_bytes(const gt_gemm_desc* d) { return (int64_t)3 * x3p_nt(d->N) * x3p_ks(d->K) * 1024; }

// the descriptor (already in head slots, gt_gemm_desc.hip: hn_slots) describes 48-wide heads in 64-column slots
static inline int x3_pad48(const gt_gemm_desc* d) {
    return d->ep_mode == GT_EP_HEADNORM && d->hn_dk == 48 && d->N == 3 * d->hn_h * 64;
}

int x3_pack_b(const gt_gemm_desc* d, GemmP& p, void* ws, int64_t ws_bytes, hipStream_t st) {
    if (d->b_packed) {                             // the caller packed this weight already (gt_gemm_pack_b_many)
        if (reinterpret_cast<uintptr_t>(d->b_packed) & 15) return GT_EALIGN;
        p.bp_f16 = d->precision == GT_PREC_F16X2;
        p.Bp = d->b_packed; p.bp_NT = x3p_nt(d->N); p.bp_KS = x3p_ks(d->K);
        return 0;
    }
    if (!ws || ws_bytes < x3_packed_bytes(d) || (reinterpret_cast<uintptr_t>(ws) & 15)) return GT_EWS;
    const int NT = x3p_nt(d->N), KS = x3p_ks(d->K);
    const int threads = NT * KS * 64;
    const int pad48 = x3_pad48(d);
    p.bp_f16 = d->precision == GT_PREC_F16X2;
    if (p.bp_f16)              // two planes + NT tile exponents: fits the three-plane buffer
        hipLaunchKernelGGL(x3_pack_b16_kernel, dim3(NT), dim3(1024), 0, st, d->B, d->layout_b, d->ldb, d->N, d->K, NT, KS,
                           reinterpret_cast<u32x4*>(ws), pad48);
    else
        hipLaunchKernelGGL(x3_pack_b_kernel, dim3((threads + 255) / 256), dim3(256), 0, st, d->B, d->layout_b, d->ldb, d->N,
                           d->K, NT, KS, reinterpret_cast<u32x4*>(ws), pad48);
    GT_LAUNCH_CHECK();
    p.Bp = ws; p.bp_NT = NT; p.bp_KS = KS;
    return 0;
}

int x3_pack_b_many(const gt_gemm_desc* descs, void* const* outs, int n, hipStream_t st) {
    if (n <= 0 || n > X3_PACK_MANY) return GT_EINVAL;
    PackManyP q{};
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const gt_gemm_desc* d = &descs[i];
        if (d->precision != GT_PREC_F16X2 || !d->B || !outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 15)) return GT_ENOTSUP;
        q.B[i] = d->B; q.out[i] = reinterpret_cast<u32x4*>(outs[i]); q.ldb[i] = d->ldb; q.layout_b[i] = d->layout_b;
        q.N[i] = d->N; q.K[i] = d->K; q.NT[i] = x3p_nt(d->N); q.KS[i] = x3p_ks(d->K); q.pad48[i] = (unsigned char)x3_pad48(d);
        q.start[i] = blocks;
        blocks += q.NT[i];
    }
    q.start[n] = blocks;
    q.n = n;
    hipLaunchKernelGGL(x3_pack_b16_many_kernel, dim3(blocks), dim3(1024), 0, st, q);
    GT_LAUNCH_CHECK();
    return 0;
}

int x3h_launch(const GemmP& p, const X3Pick& k, dim3 grid, hipStream_t st) { X3P_LAUNCH_PICK(gemm_x3h_kernel) }

}  // namespace gt
