// The descriptor layer of gt_gemm.  Every entry point starts at resolve(): the caller's descriptor becomes one or two column
// ranges, each with its Route -- engine, plan and instance, decided ONCE.  The queries read the route; gt_gemm validates, fills
// the launch parameters from it and launches.  Kernels and launchers: gt_gemm.hip, gt_gemm_x3*.hip, gt_tsmm.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gt_gemm_core.h"

namespace gt {

struct Plan { int cfg, bm, bn, bk, tiles_m, tiles_n, split, k_chunk, stream, x3; };

static inline bool m4(int64_t v) { return (v & 3) == 0; }

static bool has_epilogue(const gt_gemm_desc* d) {
    return d->c_masked || d->bias || d->rp || d->add || d->pre || d->act || d->aux_op || d->drop.p > 0.f || d->res ||
           d->out_scale != 1.f || d->ep_mode != GT_EP_NORMAL || d->K2 > 0;
}

// number of bf16 planes the split-operand kernels (gt_x3_core.h) would use for d, 0 = fp32 MFMA kernels
static int x3_planes(const gt_gemm_desc* d) {
    // GT_PREC_F16X2: the packed-B kernels run the two-term fp16 arithmetic, every other split-operand launch bf16x3
    const int planes = (d->precision == GT_PREC_BF16X3 || d->precision == GT_PREC_F16X2) ? 3
                       : d->precision == GT_PREC_BF16X2 ? 2 : d->precision == GT_PREC_BF16 ? 1 : 0;
    if (!planes || !x3_shape_ok(d) || (d->a_colsum && d->layout_a != 1)) return 0;
    return planes;
}

static int make_plan(const gt_gemm_desc* d, Plan* pl) {
    if (d->M <= 0 || d->N <= 0 || d->K < 0 || d->batch0 <= 0 || d->batch1 <= 0) return GT_EINVAL;
    if (d->precision < GT_PREC_F32 || d->precision > GT_PREC_F16X2) return GT_EINVAL;
    if (d->act < GT_ACT_NONE || (d->act > GT_ACT_SILU && d->act != GT_ACT_DROP_SILU && d->act != GT_ACT_SILU2))
        return GT_EINVAL;                          // GT_ACT_GELU: elementwise entry points only
    if (d->act == GT_ACT_SILU2 && d->drop.p > 0.f) return GT_EINVAL;
    const int64_t batch = (int64_t)d->batch0 * d->batch1;
    if (batch > 65535) return GT_EINVAL;
    pl->x3 = x3_planes(d);
    // Tile choice by a small cost model (calibrated on MI355X with tools/gemm_probe.py): the blocks that
    // share a CU share its matrix pipes, so time ~ ceil(tiles / CUs) * tile area / efficiency of the
    // configuration (MFMAs per LDS read / per barrier).  Padding waste shows up through the tile count.
    static const double kEff[kNumF32Cfg] = {1.00, 0.95, 0.80, 0.70, 0.45};
    int c = 0;
    double best = 0.0;
    for (int i = 0; i < kNumF32Cfg; ++i) {
        const int bm = kF32Cfgs[i].wm * 16 * kF32Cfgs[i].mt, bn = kF32Cfgs[i].wn * 16 * kF32Cfgs[i].nt;
        const bool head_ep = d->ep_mode == GT_EP_ROWDOT || d->ep_mode == GT_EP_MLP_BWD;
        if (head_ep && bn < d->N) continue;                         // the fused head needs whole rows per block
        // the 128x128 head instance needs > 256 registers (one block per CU): the 64x128 one runs two
        if (head_ep && i == 0 && d->N <= 128) continue;
        const double tiles = (double)ceil_div(d->M, bm) * ceil_div(d->N, bn) * (double)batch;
        // under-filled grids: with split-K available the K-slices fill the chip (time ~ total padded work),
        // otherwise every block has a CU to itself (time ~ one tile)
        const bool can_split = d->split_k != 1 && d->K >= 512 && !has_epilogue(d);
        const double units = tiles >= 256.0 ? std::ceil(tiles / 256.0) : (can_split ? tiles / 256.0 : 1.0);
        const double cost = units * bm * bn / kEff[i];
        if (best == 0.0 || cost < best) { best = cost; c = i; }
    }
    if (const char* e = getenv("GT_GEMM_CFG")) {      // tuning/debug override (tools/gemm_bench.py)
        const int f = atoi(e);
        if (f >= 0 && f < kNumF32Cfg) c = f;
    }
    if (pl->x3) c = 0;                                // the split-operand kernel has one geometry: 128 x 128 tiles
    pl->cfg = c;
    // BK=32 pays for the long-K reductions with row-contiguous operands (weight gradients); the
    // short-K token GEMMs are prologue/epilogue-bound and run better with the smaller stage
    pl->bk = (d->layout_a == 1 && d->layout_b == 1 && d->K >= 512) ? 32 : 16;
    if (const char* e = getenv("GT_GEMM_BK")) pl->bk = (atoi(e) == 16) ? 16 : 32;
    // streamed kernel: 128-wide N tiles, 16-byte aligned operands, whole granules at every edge
    // (measured: it wins from K = 256 up; at K = 128 a tile is only 4 stages long and the v1 kernel's
    // higher occupancy hides the per-tile epilogue better)
    pl->stream = (c <= 1) && d->K >= 256 && (d->K & 3) == 0 && !misaligned16(d->A, d->B) && m4(d->lda) &&
                 m4(d->ldb) && m4(d->a_bs0) && m4(d->a_bs1) && m4(d->b_bs0) && m4(d->b_bs1) &&
                 (d->layout_a == 0 || (d->M & 3) == 0) && (d->layout_b == 0 || (d->N & 3) == 0);
    if (d->ep_mode != GT_EP_NORMAL) { pl->stream = 0; pl->bk = 16; }
    if (d->K2 > 0) pl->stream = 0;
    if (pl->stream) pl->bk = 32;
    if (pl->x3) { pl->stream = 0; pl->bk = 16; }
    pl->bm = kF32Cfgs[c].wm * 16 * kF32Cfgs[c].mt;
    pl->bn = kF32Cfgs[c].wn * 16 * kF32Cfgs[c].nt;
    pl->tiles_m = ceil_div(d->M, pl->bm);
    pl->tiles_n = ceil_div(d->N, pl->bn);
    const int64_t blocks = (int64_t)pl->tiles_m * pl->tiles_n * batch;
    int split = d->split_k;
    if (split == 0) {
        split = 1;
        // aim at ~2 resident blocks per CU (two waves per SIMD hide each other's barriers and loads)
        int target = 512;
        if (const char* e = getenv("GT_GEMM_TARGET")) target = std::max(1, atoi(e));
        if (!has_epilogue(d) && blocks < 384 && d->K >= 512) {
            split = (int)std::min<int64_t>((target + blocks / 2) / blocks, d->K / (4 * pl->bk));
            if (split < 1) split = 1;
            // token-contracted products on the split engine hand whole groups of K chunks to the eight XCDs (gemm_x3w_kernel's
            // chunk-major grid): a multiple of eight chunks keeps every XCD at or under its 64 resident blocks -- 171 chunks x
            // 3 tiles put 66 on seven of them and the launch paid a second round (178 us against 117)
            if (pl->x3 && d->layout_a == 1 && d->layout_b == 1 && split >= 16) split &= ~7;
        }
    }
    if (d->cv_c > 0 && d->cv_wgrad)                   // nine taps per chunk: ~3 resident blocks per CU, whole XCD groups
        split = (int)std::max<int64_t>(1, std::min<int64_t>((768 + blocks - 1) / blocks, d->K / (4 * pl->bk)));
    if (split > 1 && has_epilogue(d)) return GT_ENOTSUP;
    if (split > 1024) split = 1024;
    int chunk = ceil_div(std::max(d->K, 1), split);
    chunk = ((chunk + pl->bk - 1) / pl->bk) * pl->bk;
    split = std::max(1, ceil_div(std::max(d->K, 1), chunk));
    pl->split = split;
    pl->k_chunk = chunk;
    return 0;
}

// ---- the route: which engine runs a product (d already in head slots, already one column range) -------------------------
enum Engine { ENG_TSMM, ENG_X3, ENG_HEAD, ENG_STREAM, ENG_TILE };
struct Route {
    Engine engine;
    int rc;                 // make_plan's answer; the plan and what follows hold when it is 0 (ENG_TSMM launches without a plan)
    Plan pl;
    bool packed, wg_f16;    // ENG_X3: a packed-B launch (x3_packed_ok) / the GT_PREC_F16X2 weight gradient (x3w_ok)
    F32Pick f32;            // ENG_HEAD / ENG_STREAM / ENG_TILE: the instance
};

static Route route(const gt_gemm_desc* d) {
    Route r{};
    r.rc = make_plan(d, &r.pl);
    if (tsmm_eligible(d)) { r.engine = ENG_TSMM; return r; }
    r.engine = ENG_TILE;
    if (r.rc) return r;
    if (r.pl.x3) {
        r.engine = ENG_X3;
        r.packed = x3_packed_ok(d, r.pl.x3, r.pl.split);
        r.wg_f16 = x3w_ok(d, r.pl.split);
    } else {                                          // (a fused-head epilogue never streams: make_plan)
        r.engine = d->ep_mode != GT_EP_NORMAL ? ENG_HEAD : r.pl.stream ? ENG_STREAM : ENG_TILE;
        r.f32 = F32Pick{r.engine == ENG_HEAD ? F32_HEAD : r.engine == ENG_STREAM ? F32_STREAM : F32_TILE, d->layout_a,
                        d->layout_b, r.pl.cfg, r.pl.bk, d->n_out};
    }
    return r;
}

// GT_EP_HEADNORM with 48-wide heads (ex3: d_model 192, 4 heads): the fused epilogue needs every head inside one wave's 64
// output columns, so the product runs with each head in a 64-column SLOT -- N' = 3 h 64 tile columns, the 16 columns behind a
// head are zero rows of the PACKED weight (the pack kernels map slot rows to weight rows; the weight itself is read in place),
// and the epilogue normalises / stores the 48 real columns.  The caller's descriptor keeps N = 3 h 48; every entry point
// plans with this copy.  (A third more MFMA work in a launch that is bound by its memory traffic; no extra HBM byte.)
static const gt_gemm_desc* hn_slots(const gt_gemm_desc* d, gt_gemm_desc* tmp) {
    if (d->ep_mode != GT_EP_HEADNORM || d->hn_dk != 48 || d->hn_h <= 0 || d->N != 3 * d->hn_h * 48) return d;
    *tmp = *d;
    tmp->N = 3 * d->hn_h * 64;
    return tmp;
}

// Widths just above a multiple of 128 (the merged-head width h*(d_k+p) = 144 of the Darcy model) would
// waste most of a second 128-wide tile column: run the aligned part and the remainder as two launches,
// the remainder on a narrow-tile configuration.
// Splits d (whose route is r) into the 128-aligned column range `a` and the remainder `b` when that pays; false otherwise.
static bool width_split(const gt_gemm_desc* d, const Route& r, gt_gemm_desc* a, gt_gemm_desc* b) {
    const int rem = d->N % 128;
    const Plan& pl = r.pl;
    if (!(d->N > 128 && rem != 0 && rem <= 64 && d->ep_mode == GT_EP_NORMAL && d->cv_c == 0 && r.rc == 0 && pl.bn == 128))
        return false;
    // only when the aligned part alone fills the chip: two half-empty launches would serialise instead.  One launch
    // per tile (split == 1): >= 512 tiles (measured);  K-split products (token-contracted, no epilogue): the K
    // slices of the aligned part fill it
    const int64_t main_tiles = (int64_t)pl.tiles_m * (d->N / 128) * d->batch0 * d->batch1;
    if (pl.split == 1 ? main_tiles < 512 : (main_tiles * pl.split < 256 || d->K2 > 0)) return false;
    const int n_main = d->N - rem;
    *a = *d;
    *b = *d;
    a->N = n_main;
    b->N = rem;
    b->B = d->B + (d->layout_b == 0 ? (int64_t)n_main * d->ldb : (int64_t)n_main);
    b->C = d->C + n_main;
    if (d->K2 > 0) b->B2 = d->B2 + (d->layout_b == 0 ? (int64_t)n_main * d->ldb2 : (int64_t)n_main);
    if (d->bias) b->bias = d->bias + n_main;
    if (d->rp) b->rp_b = d->rp_b + (int64_t)n_main * d->rp_ldb;
    if (d->add) b->add = d->add + n_main;
    if (d->pre) b->pre = d->pre + n_main;
    if (d->aux) b->aux = d->aux + n_main;
    if (d->res) b->res = d->res + n_main;
    if (d->c_masked) b->c_masked = d->c_masked + n_main;
    if (pl.split == 1) a->split_k = b->split_k = 1;      // else: each part plans its own K slices (split_k as given)
    b->a_colsum = nullptr;                               // the row sums of A ride on the first launch only
    return true;
}

// What gt_gemm does with a descriptor: `whole` = the product as one launch (what gt_gemm_plan and gt_gemm_kernel_name describe),
// part[0 .. n) = the launches it takes -- the whole, or the two column ranges of a width split.
struct Launches {
    gt_gemm_desc store[2];              // the head-slot copy, or the two column ranges
    const gt_gemm_desc *whole, *part[2];
    Route whole_r, part_r[2];
    int n;
};

static void resolve(const gt_gemm_desc* d, Launches* g) {
    g->whole = g->part[0] = hn_slots(d, &g->store[0]);
    g->whole_r = g->part_r[0] = route(g->whole);
    g->n = 1;
    // (a head-slot product is never split -- GT_EP_HEADNORM -- so the ranges do not land on the copy they are made from)
    if (!width_split(g->whole, g->whole_r, &g->store[0], &g->store[1])) return;
    for (g->n = 0; g->n < 2; ++g->n) {
        g->part[g->n] = &g->store[g->n];
        g->part_r[g->n] = route(g->part[g->n]);
    }
}

// > 0: every launch of the product is ONE launch of the packed-B kernels and this is the size of its packed weight (the buffer a
// caller that packs ahead -- gt_gemm_pack_b_many -- hands over in d->b_packed): the launches' packs back to back, the aligned
// range first; 0: some other path, b_packed must stay NULL
static int64_t packed_total(const Launches& g) {
    int64_t t = 0;
    for (int i = 0; i < g.n; ++i) {
        if (!g.part_r[i].packed) return 0;
        t += x3_packed_bytes(g.part[i]);
    }
    return t;
}

// ---- scratch of one launch: sizes and offsets, stated once for gt_gemm_ws_bytes and for the launch --------------------------
struct WsCarve {
    int64_t slabs;                  // split-K slabs [split][batch][M][N], at offset 0
    int64_t parts, acs; bool acs_staged;    // a_colsum: per-(K-slice, batch) partial row sums [parts][M] behind the slabs
    int dw2_slabs; int64_t dw2;     // GT_EP_MLP_BWD: dw2 partials [tiles_m * WM][n_out][N], at offset 0
    int64_t total;                  // what gt_gemm_ws_bytes answers: an upper bound (acs_staged), or the plane buffer x3_pack_b fills
};

static WsCarve ws_carve(const gt_gemm_desc* d, const Route& r) {
    WsCarve w;
    const int64_t batch = (int64_t)d->batch0 * d->batch1, f4 = sizeof(float);
    w.slabs = r.pl.split > 1 ? r.pl.split * batch * d->M * d->N * f4 : 0;
    w.parts = d->a_colsum ? r.pl.split * batch : 0;
    w.acs = w.parts * d->M * f4;
    // the row sums go through scratch when there is something to reduce or to scale (without a mask the loader does not apply
    // a_drop_sign: the reduce folds it in), else straight to a_colsum
    w.acs_staged = d->a_colsum && (w.parts > 1 || (!(d->a_drop.p > 0.f) && d->a_drop_sign != 1.f));
    w.dw2_slabs = r.pl.tiles_m * kF32Cfgs[r.pl.cfg].wm;
    w.dw2 = d->ep_mode == GT_EP_MLP_BWD ? w.dw2_slabs * f4 * d->n_out * d->N : 0;
    w.total = r.packed ? (d->b_packed ? 0 : x3_packed_bytes(d)) : d->ep_mode == GT_EP_MLP_BWD ? w.dw2 : w.slabs + w.acs;
    return w;
}

// ---- (a) checks that look at the descriptor alone ---------------------------------------------------------------------------
static int validate(const gt_gemm_desc* d) {
    if (!d->A || !d->B) return GT_EINVAL;
    if (!d->C && d->ep_mode != GT_EP_ROWDOT && !(d->ep_mode == GT_EP_HEADNORM && (d->hn_skip_raw_mask & 7) == 7))
        return GT_EINVAL;
    if (d->ep_mode == GT_EP_HEADNORM) {
        if (d->layout_a || d->layout_b || d->batch0 * d->batch1 != 1 || d->K2 > 0 || d->split_k > 1) return GT_ENOTSUP;
        if (d->hn_h <= 0 || d->hn_p < 0 || d->N != 3 * d->hn_h * hn_slot_width(d->hn_dk) || (d->hn_norm_mask & ~7)) return GT_EINVAL;
        if (!d->hn_out || (d->hn_p > 0 && !d->hn_pos)) return GT_EINVAL;
        if (d->hn_norm_mask && (!d->hn_gamma || !d->hn_beta || !d->hn_stats)) return GT_EINVAL;
        if (d->rp || d->add || d->pre || d->act || d->aux_op || d->drop.p > 0.f || d->res || d->out_scale != 1.f ||
            d->a_drop.p > 0.f || d->a_colsum)
            return GT_ENOTSUP;
    } else if (d->ep_mode != GT_EP_NORMAL) {
        if (d->ep_mode != GT_EP_ROWDOT && d->ep_mode != GT_EP_MLP_BWD) return GT_EINVAL;
        if (d->N > 128 || d->batch0 * d->batch1 != 1 || d->n_out < 1 || d->n_out > 4 || !d->w2) return GT_ENOTSUP;
        if (d->ep_mode == GT_EP_ROWDOT && !d->out2) return GT_EINVAL;
        if (d->ep_mode == GT_EP_MLP_BWD && (!d->g2 || !d->dw2)) return GT_EINVAL;
        if (d->a_colsum || d->a_drop.p > 0.f) return GT_ENOTSUP;
    }
    if ((d->layout_a | d->layout_b) & ~1) return GT_EINVAL;
    if (d->cv_c != 0) {                               // implicit 3x3 convolution on A (gt_hip.h: cv_*)
        if (d->cv_c < 0 || d->cv_h <= 0 || d->cv_w <= 0) return GT_EINVAL;
        if (d->cv_wgrad) {
            if (d->K % ((int64_t)d->cv_h * d->cv_w) != 0 || d->N != d->cv_c || d->batch0 != 9 || d->batch1 != 1)
                return GT_EINVAL;
            if (d->layout_a != 1 || d->layout_b != 1 || d->split_k != 0 || d->cv_w < 16 || has_epilogue(d) ||
                d->a_drop.p > 0.f || d->a_colsum)
                return GT_ENOTSUP;
        } else {
            if (d->K != 9 * d->cv_c || d->M % ((int64_t)d->cv_h * d->cv_w) != 0) return GT_EINVAL;
            if (d->layout_a || d->layout_b || (d->cv_c & 15) || d->batch0 * d->batch1 != 1 || d->split_k != 1 ||
                d->a_drop.p > 0.f || d->a_colsum || d->K2 > 0 || d->ep_mode != GT_EP_NORMAL)
                return GT_ENOTSUP;
        }
    }
    return 0;
}

// ... and what the plan and the scratch at hand refuse, in the order the codes have always been given in (behind the tall-skinny
// dispatch, which knows neither a rank update nor dropout)
static int admit(const gt_gemm_desc* d, const Route& r, const WsCarve& w, const void* ws, int64_t ws_bytes) {
    if (d->rp < 0 || d->rp > 8) return GT_EINVAL;
    if ((d->a_drop.p > 0.f && !d->a_drop.seed) || (d->drop.p > 0.f && !d->drop.seed)) return GT_EINVAL;
    if (d->a_drop.p >= 1.f || d->drop.p >= 1.f || d->a_drop.p < 0.f || d->drop.p < 0.f) return GT_EINVAL;
    if (r.rc) return r.rc;
    const Plan& pl = r.pl;
    const int64_t batch = (int64_t)d->batch0 * d->batch1;
    if ((int64_t)pl.tiles_m * pl.tiles_n * pl.split * batch > (1 << 30)) return GT_EINVAL;
    if (d->cv_c > 0 && (!pl.x3 || (!d->cv_wgrad && pl.split != 1))) return GT_ENOTSUP;
    if (d->K2 > 0 && (!d->A2 || !d->B2 || d->a_drop.p > 0.f || d->a_colsum || pl.split != 1)) return GT_ENOTSUP;
    if (d->ep_mode == GT_EP_HEADNORM) {
        if (!pl.x3 || pl.split != 1) return GT_ENOTSUP;
    } else if (d->ep_mode != GT_EP_NORMAL) {
        if (pl.tiles_n != 1 || pl.split != 1) return GT_ENOTSUP;
        if (d->ep_mode == GT_EP_MLP_BWD && (!ws || ws_bytes < w.dw2)) return GT_EWS;
    }
    if (d->a_colsum) {
        if (d->layout_a != 1) return GT_ENOTSUP;
        if (w.acs_staged && (!ws || ws_bytes < w.slabs + w.acs)) return GT_EWS;
    }
    if (pl.split > 1) {
        if (!ws || ws_bytes < w.slabs) return GT_EWS;
    } else {
        if (d->rp && (!d->rp_a || !d->rp_b)) return GT_EINVAL;
        if (d->aux_op && !d->aux) return GT_EINVAL;
        if (d->c_masked) {
            if (batch != 1 || d->ep_mode != GT_EP_NORMAL || d->K2 > 0) return GT_ENOTSUP;
            if (d->c_mask.p < 0.f || d->c_mask.p >= 1.f || (d->c_mask.p > 0.f && !d->c_mask.seed)) return GT_EINVAL;
        }
    }
    if (d->c_masked && pl.split > 1) return GT_ENOTSUP;
    if (d->b_packed && !r.packed) return GT_EINVAL;   // not a packed-B launch: see gt_hip.h
    return 0;
}

// ---- (b) descriptor -> launch parameters: the one place.  Takes no scratch (gemm_one binds it) and refuses nothing (admit),
// so gt_gemm_kernel_name fills the same block for a product nobody launches.  drop_ld / n_off: see gemm_one.
static bool aligned4(const float* p, int64_t ld, int64_t bs0 = 0, int64_t bs1 = 0) {
    return !misaligned16(p) && m4(ld) && m4(bs0) && m4(bs1);
}

static void fill_params(const gt_gemm_desc* d, const Route& r, int drop_ld, int n_off, GemmP* out) {
    GemmP& p = *out;
    const Plan& pl = r.pl;
    const int64_t batch = (int64_t)d->batch0 * d->batch1, mn = (int64_t)d->M * d->N;
    memset(&p, 0, sizeof(p));
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.batch1 = d->batch1; p.k_chunk = pl.k_chunk;
    p.n_split = pl.split; p.n_batch = (int)batch;
    p.n_work = (int)((int64_t)pl.tiles_m * pl.tiles_n * pl.split * batch);
    p.light_wait = 1;
    p.A = d->A; p.lda = d->lda; p.a_bs0 = d->a_bs0; p.a_bs1 = d->a_bs1;
    p.B = d->B; p.ldb = d->ldb; p.b_bs0 = d->b_bs0; p.b_bs1 = d->b_bs1;
    p.a_vec = aligned4(d->A, d->lda, d->a_bs0, d->a_bs1);
    p.b_vec = aligned4(d->B, d->ldb, d->b_bs0, d->b_bs1);
    p.a_drop = make_drop(&d->a_drop, d->a_drop_sign);
    p.a_drop_ld = d->a_drop_ld; p.a_drop_bstride = d->a_drop_bstride;
    p.acs = d->a_colsum;
    if (d->cv_c > 0) {
        p.cv_H = d->cv_h; p.cv_W = d->cv_w; p.cv_C = d->cv_c; p.cv_wgrad = d->cv_wgrad != 0;
        // lda (forward / data gradient) / ldb (weight gradient) = the pixel pitch of the image: >= cv_c, so a convolution can
        // read a channel slice of a wider channels-last buffer in place (values below cv_c mean "dense")
        if (d->cv_wgrad) {
            p.ldb = d->ldb > d->cv_c ? d->ldb : d->cv_c; p.b_bs0 = p.b_bs1 = 0;
            p.b_vec = aligned4(d->B, p.ldb);
        } else {
            p.lda = d->lda > d->cv_c ? d->lda : d->cv_c;
            p.a_vec = aligned4(d->A, p.lda);
        }
    }
    if (d->K2 > 0) {
        p.K2 = d->K2; p.A2 = d->A2; p.lda2 = d->lda2; p.a2_bs0 = d->a2_bs0; p.a2_bs1 = d->a2_bs1;
        p.B2 = d->B2; p.ldb2 = d->ldb2; p.b2_bs0 = d->b2_bs0; p.b2_bs1 = d->b2_bs1;
        p.a2_vec = aligned4(d->A2, d->lda2, d->a2_bs0, d->a2_bs1);
        p.b2_vec = aligned4(d->B2, d->ldb2, d->b2_bs0, d->b2_bs1);
    }
    if (d->ep_mode == GT_EP_HEADNORM) {
        p.ep_mode = d->ep_mode;
        p.hn_gamma = d->hn_gamma; p.hn_beta = d->hn_beta; p.hn_pos = d->hn_pos; p.hn_out = d->hn_out;
        p.hn_stats = d->hn_stats; p.hn_h = d->hn_h; p.hn_dk = hn_slot_width(d->hn_dk); p.hn_dkr = d->hn_dk; p.hn_p = d->hn_p;
        p.hn_DP = (d->hn_dk + d->hn_p + 3) & ~3; p.hn_mask = d->hn_norm_mask; p.hn_eps = d->hn_eps;
        p.hn_skip_raw = d->hn_skip_raw_mask & 7; p.hn_plain = d->hn_plain != 0;
    } else if (d->ep_mode != GT_EP_NORMAL) {
        p.ep_mode = d->ep_mode; p.n_out = d->n_out; p.w2 = d->w2; p.ldw2 = d->ldw2; p.b2 = d->b2;
        p.out2 = d->out2; p.g2 = d->g2;
    }
    if (pl.split > 1) {                               // raw K-slices into slabs (gemm_one: p.C); the reduce applies alpha
        p.ldc = d->N; p.c_bs0 = (int64_t)d->batch1 * mn; p.c_bs1 = mn; p.c_split = batch * mn;
        p.c_vec = m4(d->N) && m4(mn);
        p.raw = 1; p.alpha = 1.f; p.out_scale = 1.f;
    } else {
        p.C = d->C; p.ldc = d->ldc; p.c_bs0 = d->c_bs0; p.c_bs1 = d->c_bs1; p.c_split = 0;
        p.c_vec = aligned4(d->C, d->ldc, d->c_bs0, d->c_bs1);
        if (d->res) p.c_vec = p.c_vec && aligned4(d->res, d->ldr, d->r_bs0, d->r_bs1);
        if (d->add) p.c_vec = p.c_vec && aligned4(d->add, d->ldadd, d->add_bs0, d->add_bs1);
        if (d->aux_op) p.c_vec = p.c_vec && aligned4(d->aux, d->ldaux, d->aux_bs0, d->aux_bs1);
        if (d->pre) p.c_vec = p.c_vec && aligned4(d->pre, d->ldpre, (int64_t)d->M * d->ldpre);
        p.alpha = d->alpha; p.bias = d->bias;
        p.rp = d->rp; p.rp_a = d->rp_a; p.rp_lda = d->rp_lda; p.rp_a_bs0 = d->rp_a_bs0; p.rp_b = d->rp_b; p.rp_ldb = d->rp_ldb;
        p.add = d->add; p.ldadd = d->ldadd; p.add_bs0 = d->add_bs0; p.add_bs1 = d->add_bs1; p.pre = d->pre; p.ldpre = d->ldpre;
        p.act = d->act; p.aux_op = d->aux_op; p.aux = d->aux; p.ldaux = d->ldaux;
        p.aux_bs0 = d->aux_bs0; p.aux_bs1 = d->aux_bs1; p.aux_scale = d->aux_scale;
        p.drop = make_drop(&d->drop); p.drop_ld = drop_ld; p.n_off = n_off;
        p.res = d->res; p.ldr = d->ldr; p.r_bs0 = d->r_bs0; p.r_bs1 = d->r_bs1; p.out_scale = d->out_scale;
        if (d->c_masked) {
            p.c2 = d->c_masked; p.ldc2 = d->ldc_masked; p.drop2 = make_drop(&d->c_mask);
            p.c_vec = p.c_vec && aligned4(d->c_masked, d->ldc_masked);
        }
    }
    if (r.packed) p.bp_f16 = d->precision == GT_PREC_F16X2;      // (the pack itself: x3_pack_b)
    p.wg_f16 = r.wg_f16;
}

// One kernel launch (+ the reduces of what it left in scratch) for the column range [n_off, n_off + d->N) of a problem whose
// full width is drop_ld.
static int gemm_one(const gt_gemm_desc* d, const Route& r, int drop_ld, int n_off, void* ws, int64_t ws_bytes, void* stream) {
    int rc = validate(d);
    if (rc) return rc;
    if (r.engine == ENG_TSMM) return d->b_packed ? GT_EINVAL : tsmm_run(d, ws, ws_bytes, stream);
    const WsCarve w = ws_carve(d, r);
    if ((rc = admit(d, r, w, ws, ws_bytes))) return rc;
    GemmP p;
    fill_params(d, r, drop_ld, n_off, &p);
    // (c) the scratch the carve describes (admit has checked the sizes)
    if (d->ep_mode == GT_EP_MLP_BWD) p.dw2_partial = reinterpret_cast<float*>(ws);
    if (w.acs_staged) p.acs = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + w.slabs);
    if (r.pl.split > 1) {
        p.C = reinterpret_cast<float*>(ws);
        p.c_vec = p.c_vec && !misaligned16(ws);
    }
    // (d) launch, then the reduces
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned tiles = (unsigned)(r.pl.tiles_m * r.pl.tiles_n), split = (unsigned)r.pl.split, batch = (unsigned)p.n_batch;
    if (r.engine == ENG_X3) {
        if (r.packed && (rc = x3_pack_b(d, p, ws, ws_bytes, st))) return rc;
        rc = x3_launch(p, d->layout_a, d->layout_b, r.pl.x3, tiles, split, batch, st);
    } else {
        rc = f32_launch(p, r.f32, dim3(tiles, split, batch), st);
    }
    if (rc) return rc;
    if (p.dw2_partial) {
        const int64_t n2 = (int64_t)d->n_out * d->N;
        if ((rc = gt_slab_reduce(p.dw2_partial, n2, w.dw2_slabs, n2, 1.f, d->dw2, stream))) return rc;
    }
    if (w.acs_staged) {
        const float sc = (d->a_drop.p > 0.f) ? 1.f : d->a_drop_sign;
        if ((rc = gt_slab_reduce(p.acs, d->M, (int)w.parts, d->M, sc, d->a_colsum, stream))) return rc;
    }
    if (r.pl.split > 1)
        return splitk_reduce_launch(p.C, r.pl.split, d->M, d->N, d->batch0, d->batch1, d->alpha, d->C, d->ldc, d->c_bs0, d->c_bs1, st);
    return 0;
}

}  // namespace gt

using namespace gt;

extern "C" void gt_gemm_desc_init(gt_gemm_desc* d) {
    memset(d, 0, sizeof(*d));
    d->alpha = d->out_scale = d->a_drop_sign = d->aux_scale = 1.f;
    d->batch0 = d->batch1 = d->split_k = 1;
}

extern "C" int gt_gemm_plan(const gt_gemm_desc* d, int32_t* bm, int32_t* bn, int32_t* split) {
    Launches g;
    resolve(d, &g);
    const Route& r = g.whole_r;
    if (r.rc) return r.rc;
    if (bm) *bm = r.pl.bm;
    if (bn) *bn = r.pl.bn;
    if (split) *split = r.pl.split;
    return 0;
}

// Symbol of the kernel instance gt_gemm would launch for `d` (as rocprofv3 prints it), for matching the
// bench's roofline line against a kernel trace.
extern "C" int gt_gemm_kernel_name(const gt_gemm_desc* d, char* buf, int32_t n) {
    if (!d || !buf || n <= 0) return GT_EINVAL;
    Launches g;
    resolve(d, &g);
    d = g.whole;
    const Route& r = g.whole_r;
    if (r.engine != ENG_TSMM && r.rc) return r.rc;
    const char* name;
    if (r.engine == ENG_TSMM) {
        name = tsmm_kernel_name(d);
    } else if (r.engine == ENG_X3) {
        GemmP p;
        fill_params(d, r, d->N, 0, &p);
        if (r.packed) p.Bp = d->B;                    // nothing is packed here: any pointer stands for the plane buffer
        name = x3_kernel_name(p, d->layout_a, d->layout_b, r.pl.x3, d->ep_mode == GT_EP_HEADNORM ? hn_slot_width(d->hn_dk) : 0);
    } else {
        name = f32_kernel_name(r.f32);
    }
    snprintf(buf, n, "%s", name);
    return 0;
}

extern "C" int64_t gt_gemm_ws_bytes(const gt_gemm_desc* d) {
    if (!d) return 0;
    Launches g;
    resolve(d, &g);
    int64_t need = 0;                   // the launches of a width split share the scratch, one after the other (and b_packed)
    for (int i = 0; i < g.n; ++i) {
        const Route& r = g.part_r[i];
        need = std::max(need, r.engine == ENG_TSMM ? tsmm_ws_bytes(g.part[i]) : r.rc ? 0 : ws_carve(g.part[i], r).total);
    }
    return need;
}

// Round 6: a width-split product (N = 192 = 128 + 64, ex3's d_model) is TWO packed-B launches when both column ranges take
// the packed kernels; its packed weight is the two packs back to back (the aligned range first).
extern "C" int64_t gt_gemm_packed_b_bytes(const gt_gemm_desc* d) {
    if (!d) return 0;
    Launches g;
    resolve(d, &g);
    return packed_total(g);
}

extern "C" int gt_gemm_pack_b_many(const gt_gemm_desc* descs, void* const* outs, int32_t n, void* stream) {
    if (!descs || !outs || n < 0 || n > 64) return GT_EINVAL;
    gt_gemm_desc parts[128];
    void* pouts[128];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        Launches g;
        resolve(&descs[i], &g);
        if (packed_total(g) <= 0) return GT_ENOTSUP;
        int64_t off = 0;
        for (int j = 0; j < g.n; ++j) {
            parts[m] = *g.part[j];
            pouts[m++] = reinterpret_cast<char*>(outs[i]) + off;
            off += x3_packed_bytes(g.part[j]);
        }
    }
    for (int i0 = 0; i0 < m; i0 += 64) {
        int rc = x3_pack_b_many(parts + i0, pouts + i0, std::min(64, m - i0), (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int gt_gemm(const gt_gemm_desc* d, void* ws, int64_t ws_bytes, void* stream) {
    if (!d) return GT_EINVAL;
    Launches g;
    resolve(d, &g);
    // a weight packed ahead is the two column ranges' packs back to back (gt_gemm_packed_b_bytes): each range gets ITS
    // pack -- never the full-width pointer with the wrong tile geometry
    if (g.n == 2 && d->b_packed) {
        if (packed_total(g) <= 0) return GT_EINVAL;
        g.store[1].b_packed = reinterpret_cast<const char*>(d->b_packed) + x3_packed_bytes(g.part[0]);
    }
    for (int i = 0; i < g.n; ++i) {                   // same stream: the scratch is free again for the second range
        const int rc = gemm_one(g.part[i], g.part_r[i], g.whole->N, i ? g.part[0]->N : 0, ws, ws_bytes, stream);
        if (rc) return rc;
    }
    return 0;
}
