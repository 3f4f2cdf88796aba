// Column-statistics passes over a dense [rows][C4] array of float4: what the token norm (gt_tokennorm.hip), the batch norm
// (gt_batchnorm.hip) and the token softmax (gt_linattn.hip) share.  A block owns a chunk of consecutive rows and CG <= 256
// adjacent column groups (whole contiguous runs per row); its 256 threads form RL = 256 / CG row lanes, lane rl taking the
// rows r0 + rl, r0 + rl + RL, ...  Per-lane partials are merged in LDS in lane order, per-chunk partials in chunk order: no
// atomics, two runs give the same bits.  The variance is never formed as E[x^2] - mean^2: Welford per lane on values taken
// relative to a pivot row common to all partials of a column (a large common offset costs the running means no digits),
// Chan's pairwise update between partials, and every count derived from an index, never stored.  The row index type I is
// int for the head tiles (n tokens of one sample) and int64_t for the batch norm (all B n rows).  gfx950 only.
#pragma once
#include "gt_common.h"

namespace gt {

constexpr int COL_THREADS = 256;
constexpr int COL_CHUNK_MAX = 128, COL_CHUNK_MIN = 32;
constexpr int COL_MIN_BLOCKS = 1024;      // four blocks per CU of the 256 before the chunks stop shrinking

// ------------------------------------------------------------------------------------------ 1. geometry
struct ColGeom {
    int C4, CG, RL, ncb;      // column groups, of them per block, row lanes, column blocks
};
static inline ColGeom col_geom(int C4) {
    ColGeom g;
    g.C4 = C4;
    g.CG = std::min(C4, COL_THREADS);
    g.RL = COL_THREADS / g.CG;
    g.ncb = (C4 + g.CG - 1) / g.CG;
    return g;
}
// rows per chunk of the norms: shorter chunks while the grid (`per_chunk_row` blocks for every chunk) would not cover the device
static inline int col_chunk(int64_t rows, int64_t per_chunk_row) {
    int chunk = COL_CHUNK_MAX;
    while (chunk > COL_CHUNK_MIN && ((rows + chunk - 1) / chunk) * per_chunk_row < COL_MIN_BLOCKS) chunk >>= 1;
    return chunk;
}

// rows [r0, r1) of piece q when `total` rows are cut into pieces of `len`; r1 - r0 is the count behind partial q
template <typename I>
struct ColRows {
    I r0, r1;
};
template <typename I>
__device__ __forceinline__ ColRows<I> col_rows(int q, I len, I total) {
    const I r0 = q * len, e = r0 + len;
    return {r0, e < total ? e : total};
}

// ------------------------------------------------------------------------------------------ 2. lane decomposition
struct ColLane {
    int cl, rl, col4;      // column within the block, row lane, column group within the array
    bool active;           // false: a thread past RL * CG, or past C4 in a ragged last column block
};
__device__ __forceinline__ ColLane col_lane(int CG, int RL, int C4, int cb) {
    ColLane L;
    L.cl = threadIdx.x % CG;
    L.rl = threadIdx.x / CG;
    L.col4 = cb * CG + L.cl;
    L.active = L.rl < RL && L.col4 < C4;
    return L;
}
// rows of lane q of a block with `rows` rows
template <typename I>
__device__ __forceinline__ float col_lane_rows(I rows, int q, int RL) {
    return q < rows ? (float)((rows - q + RL - 1) / RL) : 0.f;
}

// ------------------------------------------------------------------------------------------ 3. Chan's pairwise update
// (mean, M2, na) <- merged with (mb, Mb, nb).  na == 0 gives (mb, Mb) exactly.
__device__ __forceinline__ void col_chan(f32x4& mean, f32x4& M2, float& na, const f32x4 mb, const f32x4 Mb, const float nb) {
    if (nb == 0.f) return;
    const float nt = na + nb, w = nb / nt;
    const f32x4 d = mb - mean;
    mean += d * w;
    M2 += Mb + d * d * (na * w);
    na = nt;
}

// ------------------------------------------------------------------------------------------ 4. a lane's rows
// X4 / G4 point at the column group in the pivot row (row 0 of the array), rows r = r0, r0 + RL, ... < r1.
// forward: Welford (mean, M2) of x - pivot
template <typename I>
__device__ __forceinline__ void col_welford_rows(const f32x4* X4, int C4, I r0, I r1, int RL, f32x4& mean, f32x4& M2) {
    const f32x4 piv = X4[0];
    float cnt = 0.f;
#pragma unroll 4
    for (I r = r0; r < r1; r += RL) {
        const f32x4 x = X4[(int64_t)r * C4] - piv;
        cnt += 1.f;
        const f32x4 d = x - mean;
        mean += d * (1.f / cnt);
        M2 += d * (x - mean);
    }
}
// backward: s1 = sum g, s2 = sum g xh, xh recomputed from x and (mean, rstd)
template <typename I>
__device__ __forceinline__ void col_gsum_rows(const f32x4* X4, const f32x4* G4, int C4, I r0, I r1, int RL, const f32x4 mean,
                                              const f32x4 rstd, f32x4& s1, f32x4& s2) {
#pragma unroll 4
    for (I r = r0; r < r1; r += RL) {
        const f32x4 x = X4[(int64_t)r * C4], g = G4[(int64_t)r * C4];
        s1 += g;
        s2 += g * ((x - mean) * rstd);
    }
}

// ------------------------------------------------------------------------------------------ 5. lane-order LDS merge
// The lanes' partials are parked as sa[t], sb[t]; merge(a2, b2, q) folds lane q = 1 .. RL-1 of column cl, in lane order.
template <typename F>
__device__ __forceinline__ void col_fold_lanes(const f32x4* sa, const f32x4* sb, int CG, int RL, int cl, F merge) {
    for (int q = 1; q < RL; ++q) merge(sa[q * CG + cl], sb[q * CG + cl], q);
}
// the norms' partials: parked, then lane 0 of each column ends with the block's (mean, M2) of its `rows` rows, or (s1, s2)
template <bool BWD, typename I>
__device__ __forceinline__ void col_merge_lanes(f32x4* sa, f32x4* sb, const ColLane& L, int CG, int RL, I rows, f32x4& a,
                                                f32x4& m2) {
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = m2;
    __syncthreads();
    if (!(L.active && L.rl == 0)) return;
    float na = col_lane_rows(rows, 0, RL);
    col_fold_lanes(sa, sb, CG, RL, L.cl, [&](const f32x4 a2, const f32x4 b2, int q) {
        if (BWD) {
            a += a2;
            m2 += b2;
        } else {
            col_chan(a, m2, na, a2, b2, col_lane_rows(rows, q, RL));
        }
    });
}

// ------------------------------------------------------------------------------------------ 6. chunk-order merge
// Partials q0 .. q1-1 of one column group, laid out [q][2][C4] from `part` (which points at the column group of q = 0), in
// order; partial q stands for the rows col_rows(q, len, total).
template <bool BWD, typename I>
__device__ __forceinline__ void col_merge_chunks(const f32x4* part, int C4, int q0, int q1, I len, I total, f32x4& a,
                                                 f32x4& m2) {
    float na = 0.f;
    for (int q = q0; q < q1; ++q) {
        const f32x4* o = part + (int64_t)q * 2 * C4;
        const f32x4 a2 = o[0], b2 = o[C4];
        if (BWD) {
            a += a2;
            m2 += b2;
        } else {
            const ColRows<I> R = col_rows(q, len, total);
            col_chan(a, m2, na, a2, b2, (float)(R.r1 - R.r0));
        }
    }
}

// ------------------------------------------------------------------------------------------ 7. head-tile shapes
// the head sizes with kernels on the layout [B*n][h][DP], DP = round4(dk + p)
static inline bool head_tile_shape_ok(int dk, int p) {
    return (dk == 16 || dk == 32 || dk == 48 || dk == 64 || dk == 96) && p >= 0 && p <= 2;
}

}  // namespace gt
