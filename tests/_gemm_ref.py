"""gt_gemm's contract (include/gt_hip.h) once, in float64, and the case list of the epilogue matrix.

    acc = sum_k A_z(m,k) keepA(m,k) B_z(k,n)  (+ sum_{k<K2} A2 B2)
    v   = alpha acc + bias[n] + sum_j rp_a[m][j] rp_b[n][j] + add_z[m][n]
    pre = v ;  v = act(v) ;  v *= f(aux) ;  v = dropout(v) ;  C = res + out_scale v  (+ c_masked = C keepscale_2)

`gemm_ref` takes the keyword arguments of `_hip.gemm` (strided views as tensor + leading dimension + batch strides) and evaluates
the formula by index arithmetic (torch.as_strided views of the caller's buffers, plain torch arithmetic; no operator of this
project).  With dtype=torch.float32 the same code is the float32 restatement the per-element gate is calibrated with.  Next to
the values it returns the ENVELOPE E: the same formula with every operand replaced by its absolute value, carried through the
epilogue with a Lipschitz bound of the activation, |f(aux)|, the keep scale, |out_scale| and |res| -- the magnitude one float32
rounding of any intermediate is relative to.

`drop_mask` restates the stateless dropout mask (csrc/gt_common.h: fmix32, drop_key, drop_hash, drop_thresh) in NumPy integer
arithmetic, so that the GPU tests compare against a mask no kernel of the library produced.

`CASES` is the one case list: tests/test_gemm_ref_cpu.py calibrates the gate on it (float32 restatement against float64, the
ReLU-kink cap), tests/test_gemm_epilogue_matrix_gpu.py runs it on the device.  `build_case` makes a case's operands -- every
epilogue operand a view into a larger buffer of its own pitch, guard rows and batch gaps -- identically on any device."""
import zlib

import numpy as np
import torch

ACT_NONE, ACT_RELU, ACT_SILU, ACT_DROP_SILU, ACT_SILU2 = 0, 1, 2, 4, 5
AUX_NONE, AUX_GT0, AUX_DSILU, AUX_MUL = 0, 1, 2, 3
U24 = 2.0 ** -24
# Lipschitz bounds: max |silu'| = 1.0998, max |silu''| = 0.5
LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SILU: 1.1, ACT_DROP_SILU: 1.1, ACT_SILU2: 1.1 * 1.1}
KINK = 8.0          # ReLU decisions with |pre64| < KINK * 2^-24 * E are not compared (the share is capped, see the CPU test)


# ---------------------------------------------------------------------------------------------- the stateless mask
_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def drop_key(seed, salt):
    lo, hi = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    s1 = np.uint64((int(salt) + 1) & 0xFFFFFFFF)
    inner = _fmix32((hi + ((np.uint64(0x9E3779B9) * s1) & _M32)) & _M32)
    return _fmix32(lo ^ inner)


def drop_thresh(p):
    t = float(np.float32(p)) * 4294967296.0
    return np.uint64(min(max(int(t), 0), 4294967295))


def drop_scale(p):
    """1 / (1 - p) as the library evaluates it: in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def drop_mask(seed, salt, p, idx):
    """keepscale(idx) of the dropout (seed, salt, p): a float64 array of 0 / 1/(1-p), idx taken mod 2^32.
    keep <=> fmix32(idx * 0x9e3779b1 + key) >= uint32(p * 2^32)."""
    idx = np.asarray(idx).astype(np.uint64) & _M32
    h = _fmix32((((idx * np.uint64(0x9E3779B1)) & _M32) + drop_key(seed, salt)) & _M32)
    return np.where(h >= drop_thresh(p), drop_scale(p), 0.0)


def _pq(d):
    """(p, salt) of a dropout argument: None, a (p, salt) pair, or anything with .p / .salt (a GtDropout)."""
    if d is None:
        return 0.0, 0
    if isinstance(d, (tuple, list)):
        return float(d[0]), int(d[1])
    return float(d.p), int(d.salt)


def _mask_t(seed, d, idx, like):
    p, salt = _pq(d)
    return torch.from_numpy(drop_mask(seed, salt, p, idx)).to(like.device)


# ---------------------------------------------------------------------------------------------- the formula
def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _silu(x):
    return x * _sig(x)


def _dsilu(x):
    s = _sig(x)
    return s * (1.0 + x * (1.0 - s))


def _dsilu_env(x):
    """silu'(x) = s + x s (1 - s) with its terms replaced by their absolute values: what one rounding of the factor is relative
    to (silu' has a zero near x = -1.28, where the two terms cancel)."""
    s = _sig(x)
    return s * (1.0 + x.abs() * (1.0 - s))


def _matmul(a, b):
    """a @ b; in float32 as a chain over k in index order (one rounded multiply and one rounded add per term: the same on
    every host, which a BLAS call is not)."""
    if a.dtype != torch.float32:
        return a @ b
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=a.dtype, device=a.device)
    for k in range(a.shape[-1]):
        acc = acc + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return acc


def _view(t, sizes, strides, dtype):
    return torch.as_strided(t, sizes, strides).to(dtype)


def gemm_ref(A, B, Cout=None, M=0, N=0, K=0, *, layout_a=0, layout_b=0, lda, ldb, ldc=0, batch=(1, 1), a_bs=(0, 0),
             b_bs=(0, 0), c_bs=(0, 0), split_k=1, alpha=1.0, bias=None, act=ACT_NONE, a_drop=None, a_drop_sign=1.0,
             a_drop_ld=0, a_drop_bstride=0, a_colsum=None, rp=0, rp_a=None, rp_lda=0, rp_a_bs0=0, rp_b=None, rp_ldb=0,
             add=None, ldadd=0, add_bs=(0, 0), pre=None, ldpre=0, aux_op=AUX_NONE, aux=None, ldaux=0, aux_bs=(0, 0),
             aux_scale=1.0, drop=None, res=None, ldr=0, r_bs=(0, 0), out_scale=1.0, K2=0, A2=None, lda2=0, a2_bs=(0, 0),
             B2=None, ldb2=0, b2_bs=(0, 0), precision=None, weight_b=False, c_masked=None, ldc_masked=0, c_mask=None,
             seed=0, dtype=torch.float64):
    """The header's formula for the arguments of `_hip.gemm`; dropout arguments as (p, salt) or GtDropout, `seed` the
    device seed's value.  Returns a dict of [b0, b1, M, N] tensors of `dtype`: C, pre, c_masked (None where not asked for),
    their envelopes E_C, E_pre, E_cm (and G_*: the factor the product's own envelope `eacc` enters them with),
    a_colsum [M], `kink` (ReLU decisions within rounding of zero) and `zeroed` (elements whose epilogue factor is an exact
    zero: dropped by the mask, or GT_AUX_GT0 on aux <= 0)."""
    b0, b1 = batch
    nz = b0 * b1

    def operand(T, ld, bs, rows, cols, transposed):          # -> [b0, b1, rows, cols]
        st = (1, ld) if transposed else (ld, 1)
        return _view(T, (b0, b1, rows, cols), (bs[0], bs[1]) + st, dtype)

    def product(A_, lda_, abs_, B_, ldb_, bbs_, Kk, keep=None):
        a = operand(A_, lda_, abs_, M, Kk, layout_a == 1)               # A(m,k) = A[m*lda + k] | A[k*lda + m]
        b = operand(B_, ldb_, bbs_, Kk, N, layout_b == 0)               # B(k,n) = B[n*ldb + k] | B[k*ldb + n]
        if keep is not None:
            a = a * keep
        return a, _matmul(a, b), a.abs() @ b.abs()

    keepA = None
    pa, _ = _pq(a_drop)
    if pa > 0:      # mask index of A's element: z*bstride + outer*ld + inner, outer = the lda-strided index
        z = np.arange(nz, dtype=np.int64).reshape(b0, b1, 1, 1) * int(a_drop_bstride)
        m, k = np.arange(M, dtype=np.int64).reshape(1, 1, M, 1), np.arange(K, dtype=np.int64).reshape(1, 1, 1, K)
        idx = z + (m * int(a_drop_ld) + k if layout_a == 0 else k * int(a_drop_ld) + m)
        keepA = (_mask_t(seed, a_drop, idx, A) * float(a_drop_sign)).to(dtype)
    a_eff, acc, eacc = product(A, lda, a_bs, B, ldb, b_bs, K, keepA)
    if K2:
        _, acc2, eacc2 = product(A2, lda2, a2_bs, B2, ldb2, b2_bs, K2)
        acc, eacc = acc + acc2, eacc + eacc2
    out = {"a_colsum": None}
    if a_colsum is not None:        # the (masked, signed) column sums of the [K, M] tensor behind A, over batch and k
        out["a_colsum"] = (a_eff if pa > 0 else a_eff * float(a_drop_sign)).sum((0, 1, 3))

    v, E = alpha * acc, abs(alpha) * eacc
    G = torch.full_like(eacc, abs(alpha))          # dE/d(eacc): what a change of the product's own envelope is multiplied with
    if bias is not None:
        bv = bias[:N].to(dtype)
        v, E = v + bv, E + bv.abs()
    if rp:
        ra = _view(rp_a, (b0, 1, M, rp), (rp_a_bs0, 0, rp_lda, 1), dtype)
        rb = _view(rp_b, (N, rp), (rp_ldb, 1), dtype)
        v, E = v + ra @ rb.t(), E + ra.abs() @ rb.abs().t()
    if add is not None:
        ad = _view(add, (b0, b1, M, N), (add_bs[0], add_bs[1], ldadd, 1), dtype)
        v, E = v + ad, E + ad.abs()

    pd, _ = _pq(drop)
    ks = None
    if pd > 0:                      # mask index (z*M + m)*N + n
        ks = _mask_t(seed, drop, np.arange(nz * M * N, dtype=np.int64).reshape(b0, b1, M, N), A).to(dtype)
    zeroed = torch.zeros((b0, b1, M, N), dtype=torch.bool, device=A.device)
    kink = torch.zeros_like(zeroed)
    pre_v, E_pre, G_pre = v, E, G
    if act == ACT_RELU:
        kink = v.abs() < KINK * U24 * E
        w = torch.clamp(v, min=0.0)
    elif act == ACT_SILU:
        w = _silu(v)
    elif act == ACT_DROP_SILU:      # the dropout in FRONT of the SiLU; pre = keepscale * silu'(u)
        kk = ks if ks is not None else torch.ones_like(v)
        u = kk * v
        w, pre_v, E_pre, G_pre = _silu(u), kk * _dsilu(u), kk * kk * 0.5 * E + kk * _dsilu_env(u), kk * kk * 0.5 * G
        E, G = kk * E, kk * G
        if ks is not None:
            zeroed = zeroed | (ks == 0)
    elif act == ACT_SILU2:          # silu(silu(v)); pre = silu'(v) * silu'(silu(v))
        a1 = _silu(v)
        # |d pre / d v| <= 0.5 * 1.1 + 1.1^2 * 0.5, plus the factors' own roundings
        w, pre_v, E_pre, G_pre = _silu(a1), _dsilu(v) * _dsilu(a1), 1.155 * E + _dsilu_env(v) * _dsilu_env(a1), 1.155 * G
    else:
        w = v
    E, G = LIP[act] * E, LIP[act] * G
    if aux_op:
        ax = _view(aux, (b0, b1, M, N), (aux_bs[0], aux_bs[1], ldaux, 1), dtype)
        if aux_op == AUX_GT0:
            f = torch.where(ax > 0, torch.full_like(ax, aux_scale), torch.zeros_like(ax))
            zeroed = zeroed | (ax <= 0)
            fe = f
        elif aux_op == AUX_DSILU:
            f, fe = _dsilu(ax), _dsilu_env(ax)
        else:
            f = ax * aux_scale
            fe = f.abs()
        w, E, G = w * f, E * fe, G * fe
    if ks is not None and act != ACT_DROP_SILU:
        w, E, G = w * ks, E * ks, G * ks
        zeroed = zeroed | (ks == 0)
    w, E, G = out_scale * w, abs(out_scale) * E, abs(out_scale) * G
    if res is not None:
        r = _view(res, (b0, b1, M, N), (r_bs[0], r_bs[1], ldr, 1), dtype)
        w, E = r + w, E + r.abs()
    out.update(C=w, E_C=E, pre=pre_v if pre is not None else None, E_pre=E_pre, kink=kink, zeroed=zeroed,
               c_masked=None, E_cm=None, keep2=None, G_C=G, G_pre=G_pre, G_cm=None, eacc=eacc)
    if c_masked is not None:
        p2, _ = _pq(c_mask)
        k2 = (_mask_t(seed, c_mask, np.arange(nz * M * N, dtype=np.int64).reshape(b0, b1, M, N), A).to(dtype)
              if p2 > 0 else torch.ones_like(w))
        out.update(c_masked=w * k2, E_cm=E * k2, keep2=k2, G_cm=G * k2)
    return out


# ---------------------------------------------------------------------------------------------- cases
# Feature sets.  Keys: alpha, bias, rp, add, pre, act, aux_op (aux_scale), drop (p), res, out_scale, cm (p of c_masked's own
# mask), K2, a_drop (p; sign -1, a_drop_ld != lda), split_k, colsum.
STACK = dict(alpha=0.75, bias=1, rp=2, add=1, pre=1, act=ACT_SILU, aux_op=AUX_MUL, aux_scale=0.5, drop=0.25, res=1,
             out_scale=-1.0)
STACK_CM = dict(STACK, cm=0.1)
FAST = {k: v for k, v in STACK_CM.items() if k not in ("rp", "add")}          # what x3_epilogue_fast takes
ALONE = {
    "plain": {}, "alpha": dict(alpha=-1.5), "bias": dict(bias=1), "rp2": dict(rp=2), "add": dict(add=1), "pre": dict(pre=1),
    "relu": dict(act=ACT_RELU), "silu": dict(act=ACT_SILU), "gt0": dict(aux_op=AUX_GT0, aux_scale=1.25),
    "drop": dict(drop=0.3), "res": dict(res=1), "oscale": dict(out_scale=-0.5), "cm": dict(cm=0.05),
    "res_oscale": dict(res=1, out_scale=-1.0),
}
GEO = [(131, 200, 16), (257, 131, 130), (99, 97, 24)]     # whole tile + ragged edge; N % 4 != 0 twice
PACKED_M = 16384 + 37
BIG_M = 65536 + 37


def _case(cid, fam, eng, prec, M, N, K, feat, la=0, lb=0, cfg=None, batch=(1, 1), mis=None, packed_ahead=False, data=None):
    """`data` names the operands' values (default: the case's id): cases that differ in engine only may share them, and
    with them one evaluation of the reference."""
    return dict(id=cid, fam=fam, eng=eng, prec=prec, M=M, N=N, K=K, feat=dict(feat), la=la, lb=lb, cfg=cfg, batch=batch,
                mis=mis, packed_ahead=packed_ahead, data=data or cid)


def _engines(which="all"):
    """(label, eng, prec, cfg, packed_ahead): one entry per kernel family and arithmetic."""
    e = [("tile%d" % c, "tile", "f32", c, False) for c in range(5)]
    e += [("stream%d" % c, "stream", "f32", c, False) for c in range(2)]
    e += [("ring-" + p, "ring", p, None, False) for p in ("bf16x3", "f16x2")]
    e += [("packed-" + p, "packed", p, None, False) for p in ("bf16x3", "f16x2")]
    e += [("packed-ahead-f16x2", "packed", "f16x2", None, True)]
    if which == "one":          # one instance per family
        keep = ("tile0", "stream0", "ring-bf16x3", "packed-bf16x3", "packed-f16x2")
        e = [x for x in e if x[0] in keep]
    return e


def _geo(eng, M, N, K):
    """The geometry on an engine: the streamed kernel starts at K = 256, the packed kernel at 16384 rows with K % 4 == 0."""
    if eng == "stream":
        return M, N, 256
    if eng == "packed":
        return PACKED_M, N, 20
    if eng == "ring" and K == 130:
        return M, N, 24 if N == 131 else 16
    return M, N, K


def _make_cases():
    cs = []
    # the full stack at every geometry, layouts (0,0) and (0,1), every engine
    for lab, eng, prec, cfg, ahead in _engines():
        for (M, N, K) in GEO:
            for lb in (0, 1):
                m, n, k = _geo(eng, M, N, K)
                cs.append(_case(f"stack-{lab}-{m}x{n}x{k}-lb{lb}", "stack", eng, prec, m, n, k, STACK_CM, lb=lb, cfg=cfg,
                                packed_ahead=ahead))
        if eng in ("tile", "stream"):               # the fp32 engine's narrow widths: vec2 and scalar stores, one tile column
            for n in (1, 2, 3, 36):
                m, n_, k = _geo(eng, 131, n, 24)
                cs.append(_case(f"stack-{lab}-{m}x{n}x{k}", "stack", eng, prec, m, n, k, STACK_CM, cfg=cfg))
        if eng == "tile":                            # K = 130: a ragged last k-stage, unaligned rows of A and B
            cs.append(_case(f"stack-{lab}-131x200x130", "stack", eng, prec, 131, 200, 130, STACK_CM, cfg=cfg))
    # K = 130 on the split-operand engine: K % 4 != 0, which the ring kernel's direct 16-byte loads do not take -- the staged
    # kernel (gemm_x3_kernel) runs it
    for lb in (0, 1):
        cs.append(_case(f"stack-staged-bf16x3-131x200x130-lb{lb}", "stack", "ring", "bf16x3", 131, 200, 130, STACK_CM, lb=lb))
    # plain product, all four layout pairs where the engine takes them
    for lab, eng, prec, cfg, ahead in _engines("one"):
        for la in (0, 1):
            for lb in (0, 1):
                if eng == "packed" and la == 1:      # (m-contiguous A wants M % 4 == 0; PACKED_M is odd on purpose)
                    continue
                m, n, k = _geo(eng, 132 if la == 1 and eng != "tile" else 131, 200, 24)
                cs.append(_case(f"plain-{lab}-{m}x{n}x{k}-la{la}lb{lb}", "plain", eng, prec, m, n, k, {}, la=la, lb=lb, cfg=cfg))
    # every field alone
    for lab, eng, prec, cfg, ahead in _engines("one"):
        m, n, k = _geo(eng, 131, 200, 16)
        for name, feat in ALONE.items():
            if name != "plain":
                cs.append(_case(f"alone-{name}-{lab}", "alone", eng, prec, m, n, k, feat, cfg=cfg))
    # activations x aux ops (pre always; dropout except under GT_ACT_SILU2), at a width off the vector path
    for lab, eng, prec, cfg, ahead in (("tile1", "tile", "f32", 1, False), ("ring-bf16x3", "ring", "bf16x3", None, False),
                                       ("packed-f16x2", "packed", "f16x2", None, False)):
        m, n, k = _geo(eng, 99, 97, 24)
        for act in (ACT_NONE, ACT_RELU, ACT_SILU, ACT_DROP_SILU, ACT_SILU2):
            for aux_op in (AUX_GT0, AUX_DSILU, AUX_MUL):
                feat = dict(bias=1, pre=1, act=act, aux_op=aux_op, aux_scale=1.25, res=1, out_scale=-1.0)
                if act != ACT_SILU2:
                    feat["drop"] = 0.25
                cs.append(_case(f"actaux-a{act}-x{aux_op}-{lab}", "actaux", eng, prec, m, n, k, feat, cfg=cfg))
    # rank updates of every width class, the fast-path subset with and without `add`
    for lab, eng, prec, cfg, ahead in _engines("one"):
        m, n, k = _geo(eng, 131, 200, 16)
        if eng != "stream":
            for rp in (1, 3, 8):
                cs.append(_case(f"rp{rp}-{lab}", "stack", eng, prec, m, n, k, dict(STACK, rp=rp), cfg=cfg))
        cs.append(_case(f"fast-{lab}", "stack", eng, prec, m, n, k, FAST, cfg=cfg))
        cs.append(_case(f"fast+add-{lab}", "stack", eng, prec, m, n, k, dict(FAST, add=1), cfg=cfg))
    # second product (fp32 engine and the split-operand engine below the packed kernel's rows)
    for lab, eng, prec, cfg in (("tile0", "tile", "f32", 0), ("tile3", "tile", "f32", 3), ("ring-bf16x3", "ring", "bf16x3", None)):
        for lb in (0, 1):
            cs.append(_case(f"k2-{lab}-lb{lb}", "stack", eng, prec, 131, 200, 16, dict(STACK, K2=24), lb=lb, cfg=cfg))
    # dropout on A, sign -1, mask pitch != lda, both layouts of A
    for lab, eng, prec, cfg in (("tile0", "tile", "f32", 0), ("ring-bf16x3", "ring", "bf16x3", None),
                                ("packed-f16x2", "packed", "f16x2", None)):
        for la in (0, 1):
            if eng == "packed" and la == 1:
                continue
            m, n, k = _geo(eng, 132 if (la == 1 and eng == "ring") else 131, 200, 24)
            feat = dict(a_drop=0.2, bias=1, res=1)
            if la == 1:
                feat["colsum"] = 1
            cs.append(_case(f"adrop-{lab}-la{la}", "stack", eng, prec, m, n, k, feat, la=la, cfg=cfg))
    # two-level batch (2, 3): distinct, padded strides everywhere; `pre` dense
    for lab, eng, prec, cfg in (("tile0", "tile", "f32", 0), ("tile2", "tile", "f32", 2), ("stream0", "stream", "f32", 0),
                                ("ring-bf16x3", "ring", "bf16x3", None), ("ring-f16x2", "ring", "f16x2", None)):
        for lb in (0, 1):
            m, n, k = _geo(eng, 131, 200, 16)
            cs.append(_case(f"batch-{lab}-lb{lb}", "stack", eng, prec, m, n, k, STACK, lb=lb, cfg=cfg, batch=(2, 3)))
    # split-K into a padded C with batch strides
    for lab, eng, prec, cfg in (("tile0", "tile", "f32", 0), ("ring-bf16x3", "ring", "bf16x3", None)):
        cs.append(_case(f"splitk-{lab}", "plain", eng, prec, 131, 200, 130 if eng == "tile" else 384, dict(alpha=0.5, split_k=3),
                        cfg=cfg, batch=(2, 1)))
    # the fp32 tile kernel's BK = 32 instances: row-contiguous operands, K >= 512, M off the streamed kernel's alignment
    for cfg in (0, 3):
        for name, feat in (("plain", {}), ("stack", STACK_CM)):
            cs.append(_case(f"{name}-tile{cfg}-bk32-131x200x520", name, "tile", "f32", 131, 200, 520, feat, la=1, lb=1, cfg=cfg))
    # one operand in turn moved by one float: c_vec falls, the answer stays
    for lab, eng, prec, cfg, ahead in _engines("one"):
        m, n, k = _geo(eng, 131, 200, 16)
        for mis in ("C", "res", "add", "aux", "pre", "c_masked"):
            feat = FAST if (eng == "packed" and mis != "add") else STACK_CM
            cs.append(_case(f"mis-{mis}-{lab}", "stack", eng, prec, m, n, k, feat, cfg=cfg, mis=mis))
    # width split for real: the aligned part fills the chip, so gt_gemm runs two launches
    wide = dict(STACK_CM)
    for lab, eng, prec, ahead in (("f32", "wide-f32", "f32", False), ("packed-bf16x3", "packed", "bf16x3", False),
                                  ("packed-f16x2", "packed", "f16x2", False), ("packed-ahead-f16x2", "packed", "f16x2", True)):
        for n in (144, 288):
            for lb in ((0, 1) if n == 144 else (0,)):
                cs.append(_case(f"wsplit-{lab}-N{n}-lb{lb}", "wsplit", eng, prec, BIG_M, n, 24, wide, lb=lb, packed_ahead=ahead,
                                cfg=0 if prec == "f32" else None,          # (the fp32 engine splits on its 128-wide tiles only)
                                data=f"wsplit-N{n}-lb{lb}"))
    cs.append(_case("wsplit-f32-N144-k2", "wsplit", "wide-f32", "f32", BIG_M, 144, 24, dict(STACK, K2=16), lb=1, cfg=0))
    cs.append(_case("wsplit-ring-batch8-N144", "wsplit", "ring", "bf16x3", 8192 + 5, 144, 24, STACK, batch=(8, 1)))
    cs.append(_case("wsplit-ring-batch8-N144-lb1", "wsplit", "ring", "bf16x3", 8192 + 5, 144, 24, STACK, lb=1, batch=(8, 1)))
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = _make_cases()

# Largest normalised error of the float32 restatement per case family, max |ref32 - ref64| / (2^-24 E), as
# tests/test_gemm_ref_cpu.py prints it (it asserts that no case exceeds its family's entry).  The GPU gate is 4 x this.
R32 = {"plain": 6.0, "alone": 6.1, "stack": 5.9, "actaux": 5.4, "wsplit": 5.4}

_POOL = {}
POOL_N = 1 << 25


def pool(device):
    """One deterministic N(0, 1) pool per device; operands are slices of it at their own offsets."""
    key = str(device)
    if key not in _POOL:
        g = torch.Generator(device="cpu").manual_seed(20240611)
        _POOL[key] = torch.randn(POOL_N, generator=g).to(device)
    return _POOL[key]


SENTINEL = 0x7FC5A5A5       # a quiet NaN with a payload no kernel computes


class Buf:
    """A [b0, b1, rows, cols] view (strides bs0, bs1, ld, 1) at `off` floats into a flat buffer with guard space around it."""

    def __init__(self, name, flat, off, sizes, strides):
        self.name, self.flat, self.off, self.sizes, self.strides = name, flat, off, tuple(sizes), tuple(strides)
        self.t = flat[off:]                                  # what the library gets: the pointer of element (0, 0, 0, 0)

    @property
    def ld(self):
        return self.strides[2]

    @property
    def bs(self):
        return self.strides[0], self.strides[1]

    def view(self):
        return torch.as_strided(self.flat, self.sizes, self.strides, self.off)

    def inside(self):
        m = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        torch.as_strided(m, self.sizes, self.strides, self.off).fill_(True)
        return m

    def bits(self):
        return self.flat.view(torch.int32)


def _salt(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _padded(name, slot, device, batch, rows, cols, mis=False, dense_batch=False, output=False, scale=1.0):
    """Operand `name` as a view into a larger buffer: pitch cols + 4 (slot + 1) rounded to 4 floats, slot + 1 guard rows in
    front, batch strides larger than dense and distinct per operand; `mis` moves the view by one float."""
    b0, b1 = batch
    ld = (cols + 3) // 4 * 4 + 4 * (slot + 1)
    if dense_batch:                                          # `pre`: dense [batch][M][ldpre] (gt_hip.h)
        bs1 = rows * ld
        bs0 = b1 * bs1
    else:
        bs1 = (rows + 1) * ld + 4 * (slot + 1)
        bs0 = b1 * bs1 + 8 * (slot + 2)
    off = (slot + 1) * ld + (1 if mis else 0)
    total = off + b0 * bs0 + 3 * ld + 8
    if output:
        flat = torch.full((total,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    else:
        o = (1 + _salt(name) % 9973) * 1009 % (POOL_N - total)
        flat = pool(device)[o:o + total].clone()
        if scale != 1.0:
            flat *= scale
    return Buf(name, flat, off, (b0, b1, rows, cols), (bs0, bs1, ld, 1))


def build_case(case, device, seed=0):
    """-> (fields, outs): the keyword arguments of `_hip.gemm` / `gemm_ref` for the case (dropouts as (p, salt) pairs: the GPU
    module turns them into descriptors) and the output buffers {name: Buf}.  A and B are padded views as well."""
    M, N, K, la, lb, batch, f = case["M"], case["N"], case["K"], case["la"], case["lb"], case["batch"], case["feat"]
    mis = case["mis"]
    nm = lambda s: case["data"] + "/" + s

    def opnd(name, slot, rows, cols, scale=1.0):
        return _padded(nm(name), slot, device, batch, rows, cols, scale=scale)

    A = opnd("A", 0, M if la == 0 else K, K if la == 0 else M)
    B = opnd("B", 1, N if lb == 0 else K, K if lb == 0 else N, scale=0.5)
    C = _padded(nm("C"), 0, device, batch, M, N, mis=(mis == "C"), output=True)
    fields = dict(A=A.t, B=B.t, Cout=C.t, M=M, N=N, K=K, layout_a=la, layout_b=lb, lda=A.ld, ldb=B.ld, ldc=C.ld, batch=batch,
                  a_bs=A.bs, b_bs=B.bs, c_bs=C.bs, split_k=f.get("split_k", 1), alpha=f.get("alpha", 1.0),
                  act=f.get("act", ACT_NONE), out_scale=f.get("out_scale", 1.0), precision=case["prec"])
    outs = {"C": C}
    if f.get("bias"):
        fields["bias"] = pool(device)[77:77 + N].clone()
    if f.get("rp"):
        rp = f["rp"]
        ra = _padded(nm("rp_a"), 2, device, (batch[0], 1), M, rp)
        rb = _padded(nm("rp_b"), 3, device, (1, 1), N, rp)
        fields.update(rp=rp, rp_a=ra.t, rp_lda=ra.ld, rp_a_bs0=ra.bs[0], rp_b=rb.t, rp_ldb=rb.ld)
    if f.get("add"):
        ad = _padded(nm("add"), 2, device, batch, M, N, mis=(mis == "add"))
        fields.update(add=ad.t, ldadd=ad.ld, add_bs=ad.bs)
    if f.get("aux_op"):
        ax = _padded(nm("aux"), 3, device, batch, M, N, mis=(mis == "aux"))
        fields.update(aux_op=f["aux_op"], aux=ax.t, ldaux=ax.ld, aux_bs=ax.bs, aux_scale=f.get("aux_scale", 1.0))
    if f.get("res"):
        r = _padded(nm("res"), 1, device, batch, M, N, mis=(mis == "res"))
        fields.update(res=r.t, ldr=r.ld, r_bs=r.bs)
    if f.get("pre"):
        p = _padded(nm("pre"), 4, device, batch, M, N, mis=(mis == "pre"), dense_batch=True, output=True)
        fields.update(pre=p.t, ldpre=p.ld)
        outs["pre"] = p
    if f.get("cm"):
        cm = _padded(nm("c_masked"), 5, device, batch, M, N, mis=(mis == "c_masked"), output=True)
        fields.update(c_masked=cm.t, ldc_masked=cm.ld, c_mask=(f["cm"], _salt(nm("cm"))))
        outs["c_masked"] = cm
    if f.get("drop"):
        fields["drop"] = (f["drop"], _salt(nm("drop")))
    if f.get("a_drop"):             # mask pitch != lda: the mask lives in the index space of a wider dense tensor
        fields.update(a_drop=(f["a_drop"], _salt(nm("a_drop"))), a_drop_sign=-1.0, a_drop_ld=A.ld + 3,
                      a_drop_bstride=(A.sizes[2] + 2) * (A.ld + 3))
    if f.get("colsum"):
        fields["a_colsum"] = torch.full((M,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    if f.get("K2"):
        K2 = f["K2"]
        A2 = opnd("A2", 2, M if la == 0 else K2, K2 if la == 0 else M)
        B2 = opnd("B2", 3, N if lb == 0 else K2, K2 if lb == 0 else N, scale=0.5)
        fields.update(K2=K2, A2=A2.t, lda2=A2.ld, a2_bs=A2.bs, B2=B2.t, ldb2=B2.ld, b2_bs=B2.bs)
    return fields, outs


def ref_fields(fields, seed, dtype=torch.float64):
    return gemm_ref(**fields, seed=seed, dtype=dtype)


def f16x2_extra(fields, ref):
    """What the two-term fp16 packed-B arithmetic adds to the product's envelope, in units of 2^-24 (derivation in
    tests/test_gemm_epilogue_matrix_gpu.py): 2^-22 K rowmax|A_m| tilemax|B| per output element, tile = 32 output columns.
    -> {"C": ..., "pre": ..., "c_masked": ...}, each to be ADDED to the matching envelope E_*."""
    M, N, K = fields["M"], fields["N"], fields["K"]
    la, lb = fields["layout_a"], fields["layout_b"]
    a = torch.as_strided(fields["A"], (M, K), (fields["lda"], 1) if la == 0 else (1, fields["lda"])).double().abs()
    b = torch.as_strided(fields["B"], (K, N), (1, fields["ldb"]) if lb == 0 else (fields["ldb"], 1)).double().abs()
    pa, _ = _pq(fields.get("a_drop"))
    rowmax = a.amax(1) * (drop_scale(pa) if pa > 0 else 1.0)             # [M]
    colmax = b.amax(0)                                                   # [N]
    tile = torch.nn.functional.pad(colmax, (0, (-N) % 32)).reshape(-1, 32).amax(1).repeat_interleave(32)[:N]
    e16 = (4.0 * K * rowmax[:, None] * tile[None, :]).reshape(1, 1, M, N)    # 2^-22 = 4 * 2^-24
    return {k: (ref[g] * e16 if ref[g] is not None else None) for k, g in (("C", "G_C"), ("pre", "G_pre"), ("c_masked", "G_cm"))}


# ---------------------------------------------------------------------------------------------- which kernel a case runs on
F32_CFGS = [(4, 4, 2, 2), (2, 4, 2, 2), (2, 2, 2, 2), (2, 2, 4, 1), (2, 1, 4, 1)]       # gt_gemm_core.h: kF32Cfgs


def expected_kernel(case):
    """The kernel instance the plain, unbatched product of the case's shape and alignment is routed to (gt_gemm_desc.hip:
    make_plan / route, gt_gemm_x3.hip: x3_pick), as a substring of its symbol.  Operands are 16-byte aligned with pitches
    that are multiples of four floats (build_case)."""
    M, N, K, la, lb, prec = case["M"], case["N"], case["K"], case["la"], case["lb"], case["prec"]
    if prec != "f32" and ((M >= 96 and N >= 96 and K >= 16) or
                          (16 <= N < 96 and M >= 16384 and M >= 8 * N and K >= 16 and K % 4 == 0 and la == 0)):
        if M >= 16384 and M >= 8 * N and (K % 4 == 0 if la == 0 else M % 4 == 0) and case["feat"].get("split_k", 1) == 1:
            return "gemm_x3%s_kernel<%d, 0, 0, %d>" % ("h" if prec == "f16x2" else "p", la, 64 if (N <= 64 and la == 0) else 128)
        ring = not ((la == 0 or lb == 0) and K % 4) and not (la == 1 and M % 4) and not (lb == 1 and N % 4)
        return ("gemm_x3r_kernel<%d, %d, 3, 3, 0, 0>" if ring else "gemm_x3_kernel<%d, %d, 3>") % (la, lb)
    cfg = case["cfg"]
    mt, nt, wm, wn = F32_CFGS[cfg]
    if cfg <= 1 and K >= 256 and K % 4 == 0 and (la == 0 or M % 4 == 0) and (lb == 0 or N % 4 == 0):
        return "gemm_stream_kernel<%d, %d, %d>" % (la, lb, mt)
    bk = 32 if (la == 1 and lb == 1 and K >= 512) else 16
    return "gemm_kernel<%d, %d, %d, %d, %d, %d, %d, 0>" % (la, lb, mt, nt, wm, wn, bk)
