"""The attention nodes: dropout mode, mask queue and call setup (_attn_dropout_setup); AttnConfig; what both nodes share around
the cores (_check_config, _core_call); the self node's projection stage; the galerkin / linear, fourier, softmax and causal
cores behind one table, _CORES; SimpleAttentionFn; multihead_attention (the classic Transformer layer's attention) as a
softmax node without coordinates; CrossAttentionFn (query, key, value not one tensor) on the same table;
causal_linear_attention, the causal core alone on [B, h, n, D] tensors.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import NamedTuple

import torch
from torch.autograd import Function

from .. import _hip as H
from ._handoff import _hint_output_mask, _offer_twin, _take_twin, _wanted_mask
from .dense import _check_res_is_x
from .elementwise import _c, _next_salt


# ----------------------------------------------------------------------------------- dropout bookkeeping
# The reference applies F.dropout(p_attn) with the *default* p=0.5, training=True to the attention
# matrix in train and eval alike (layers.py:700-701, 730-731).  Modes:
#   "reference": stateless-RNG Bernoulli(0.5) mask, x2 rescale (default, reference-faithful)
#   "off"      : identity (exact-math parity runs)
#   "replay"   : multiply by explicit masks queued with push_attention_masks() (mask-replay parity)
_attn_mode = "reference"
_attn_masks = []


def set_attention_dropout(mode: str):
    global _attn_mode
    if mode not in ("reference", "off", "replay"):
        raise ValueError(mode)
    _attn_mode = mode
    _attn_masks.clear()


def get_attention_dropout() -> str:
    return _attn_mode


def push_attention_masks(masks):
    """Queue explicit multiplicative masks (values 0 or 2), consumed one per attention call."""
    _attn_masks.extend(masks)


def _attn_dropout_setup(who, kind, keep, device):
    """The attention-dropout mode of one simple_attention / cross_attention call (``who``) -> (mask, p_attn): what travels in
    the node's mask slot and the rate of the stateless dropout.  "replay" pops one queued mask; a Galerkin mask
    [B, h, Dr, Dr] is zero-padded to round4(Dr).  kind='causal' draws no attention dropout and consults no mode: its keep
    vector takes the mask slot.  (multihead_attention has its own rate and mask arguments and does not come here.)"""
    if kind == "causal":
        return keep, 0.0
    if keep is not None:
        raise ValueError(f"{who}: keep is the key / value mask of kind='causal'")
    if _attn_mode != "replay":
        return None, (0.5 if _attn_mode == "reference" else 0.0)
    if not _attn_masks:
        raise RuntimeError("attention dropout mode 'replay' but no mask queued")
    m = _attn_masks.pop(0).to(device=device, dtype=torch.float32)
    if kind not in ("galerkin", "linear"):
        return _c(m), 0.0
    Dr = m.shape[-1]
    DP = H.round4(Dr)
    mask = torch.zeros(*m.shape[:2], DP, DP, dtype=torch.float32, device=device)
    mask[..., :Dr, :Dr] = m
    return mask, 0.0


_plain_tiles = [os.environ.get("GT_PLAIN_TILES", "1") != "0"]          # K', V' head tiles without the LayerNorm affine
_dkv_ln_fused = [os.environ.get("GT_DKV_LN", "1") != "0"]               # gt_galerkin_dkv_ln vs gt_galerkin_dkv + gt_headnorm_bwd
_qkvnorm_fused = [True]         # QKV projection + head norm in one launch when the library supports the shape


# ----------------------------------------------------------------------------------- what both nodes share
# The non-tensor arguments of an attention node, read by field name.  ``share``: "self" in SimpleAttentionFn, else which of
# (query, key, value) are one tensor ("none", "kv", "qk": CrossAttentionFn).
AttnConfig = NamedTuple("AttnConfig", [("kind", str), ("h", int), ("norm_mask", int), ("eps", float), ("sign", float),
                                       ("p_attn", float), ("p_out", float), ("need_w", bool), ("token_norm", bool),
                                       ("share", str)])


def _config(*values):
    """AttnConfig from its ten values in field order, each converted to its field's type."""
    return AttnConfig(*(t(v) for t, v in zip(AttnConfig.__annotations__.values(), values)))


def _check_token_count(n, name):
    if n < 2:       # nn.InstanceNorm1d: "Expected more than 1 spatial element when training"
        raise ValueError(f"norm_type='instance' needs more than 1 token per sample to normalise over (got {name}={n})")


def _check_config(who, cfg, dk, p, n_tok, gamma, beta, nopos_ok):
    """Every refusal of a node (``who``) that needs no tensor data, raised before anything is allocated or launched: the kind,
    what token_norm goes with, and the head sizes that have a kernel.  ``n_tok`` = (name, count) of the tokens that
    norm_type='instance' normalises over; ``nopos_ok``: the node takes softmax head tiles without coordinate columns."""
    kind, DP = cfg.kind, H.round4(dk + p)
    if kind not in _CORES:
        raise ValueError(f"{who}: kind={kind!r}")
    if cfg.token_norm and (kind not in ("galerkin", "linear") or cfg.norm_mask != 0b110 or gamma is None or beta is None):
        raise ValueError(f"{who}: token_norm is the K, V norm of the galerkin / linear kinds")
    if kind == "linear" and not H.linattn_supported(dk, p):
        raise H.GtNotSupported(f"{who}: linear attention: head size d_k={dk}, pos_dim={p} has no softmax kernel")
    # (without coordinates the tiles are exactly d_k wide and run on the tail-free instances: multihead_attention)
    nopos = nopos_ok and p == 0 and DP in H.SOFTMAX_DP_NOPOS
    if kind == "softmax" and DP not in H.SOFTMAX_DP + H.SOFTMAX_DP_WIDE and not nopos:
        raise H.GtNotSupported(f"{who}: softmax attention: head tile width round4(d_k + pos_dim) = {DP} has no kernel "
                               f"(supported: {H.SOFTMAX_DP} and {H.SOFTMAX_DP_WIDE}, i.e. d_k in (16, 32, 48, 64, 96) "
                               "with 1..4 coordinate columns"
                               + (f"; {H.SOFTMAX_DP_NOPOS} without coordinates)" if nopos_ok else ")"))
    if kind == "causal":
        H.causal_check(DP)
    if cfg.token_norm:
        _check_token_count(n_tok[1], n_tok[0])
        if not H.linattn_supported(dk, p):
            raise H.GtNotSupported(f"{who}: norm_type='instance': head size d_k={dk}, pos_dim={p} has no token-norm kernel")


def _head_dims(shape, h, pos):
    """(B, n, d, h, dk, p, Dr, DP) of a query [B, n, d]: Dr = dk + p columns per head tile, padded to DP = round4(Dr)."""
    B, n, d = shape
    dk = d // h
    p = 0 if pos is None else pos.shape[-1]
    return B, n, d, h, dk, p, dk + p, H.round4(dk + p)


def _save_named(ctx, **tensors):
    """ctx.save_for_backward by name: the only way a tensor travels from an attention forward to its backward.  A value is a
    tensor, None, or a tuple of those (saved one by one, handed back as a tuple)."""
    ctx.saved_names = tuple((k, len(v) if isinstance(v, tuple) else None) for k, v in tensors.items())
    ctx.save_for_backward(*(t for v in tensors.values() for t in (v if isinstance(v, tuple) else (v,))))


def _saved(ctx):
    it = iter(ctx.saved_tensors)
    return SimpleNamespace(**{k: next(it) if cnt is None else tuple(next(it) for _ in range(cnt))
                              for k, cnt in ctx.saved_names})


def _core_call(cfg, dims, salt, dev, mask, keep, has_bias_fc, *, n_kv=None, plain=False, fused_ln=False, wf=None, bfc=None,
               affine=(None, None)):
    """The per-call namespace ``c`` that both halves of a core read, built the same way by a forward and by its backward (which
    leaves out wf, bfc, affine: the backward takes its tensors from the saved ones).  d_attn / d_out: the descriptors of the
    stateless attention dropout (none under an explicit mask) and of the output dropout, at salt and salt + 1."""
    return SimpleNamespace(kind=cfg.kind, dims=dims, n_kv=n_kv, sign=cfg.sign, need_w=cfg.need_w, token_norm=cfg.token_norm,
                           mask=mask, keep=keep, wf=wf, bfc=bfc, affine=affine, plain=plain, fused_ln=fused_ln,
                           has_bias_fc=has_bias_fc,
                           d_attn=H.dropout_desc(cfg.p_attn, salt, dev) if (cfg.p_attn > 0 and mask is None) else None,
                           d_out=H.dropout_desc(cfg.p_out, salt + 1, dev) if cfg.p_out > 0 else None)


def _masked_out_grad(g, d_out, twin=None):
    """The output gradient under the output dropout's mask: masked once here, not in every consumer's operand loader, and not
    at all where ``twin(g)`` finds the copy that the consumer of ``out`` wrote (the hand-off of ops/_handoff.py)."""
    if d_out is None:
        return g
    gmk = None if twin is None else twin(g)
    return gmk if gmk is not None else H.dropout_apply(g, d_out)


def _token_norm_bwd(s, dO3, dims, m):
    """The token-axis norm of K, V backwards: dK', dV' (dO3[1], dO3[2], over m tokens per sample) -> the gradients of the raw
    tiles s.out3[1], s.out3[2], in place.  Returns (dgamma, dbeta) [2, h, dk] in (norm_K, norm_V) order."""
    B, n, d, h, dk, p, Dr, DP = dims
    dgamma = torch.empty(2, h, dk, dtype=torch.float32, device=dO3[1].device)
    dbeta = torch.empty_like(dgamma)
    H.token_norm_bwd(s.out3[1], dO3[1], s.gamma[0], s.st_k, B, m, h, dk, p, out=dO3[1], dgamma=dgamma[0], dbeta=dbeta[0])
    H.token_norm_bwd(s.out3[2], dO3[2], s.gamma[1], s.st_v, B, m, h, dk, p, out=dO3[2], dgamma=dgamma[1], dbeta=dbeta[1])
    return dgamma, dbeta


# ----------------------------------------------------------------------------------- the self node's projection stage
def _project_heads(xc, posc, wq, bqkv, gamma, beta, dims, norm_mask, eps, token_norm, fused_ln):
    """QKV projection + head norm (+ the token-axis norm of K, V): what every kind shares.  Returns (qkv, stats, out3, tn,
    plain): the raw projection (None where nothing reads it), the LayerNorm statistics, the head tiles [3, T, h, DP], the
    token-norm triple (kvn, st_k, st_v) or Nones, and whether the tiles are "plain"."""
    B, n, d, h, dk, p, Dr, DP = dims
    T, dev = B * n, xc.device
    if token_norm:
        # the projection leaves RAW K, V (+ coordinates) in the tiles: no per-token norm, no affine on its epilogue
        hn_mask, hn_gamma, hn_beta = 0, None, None
    else:
        hn_mask, hn_gamma, hn_beta = norm_mask, gamma, beta
    qkv = out3 = stats = None
    # "plain" head tiles: when every consumer of K', V' is one of the fused Galerkin kernels, the tiles keep the
    # normalised values WITHOUT the LayerNorm affine (the consumers apply gamma / beta), the backward takes xh from the
    # tiles, and the raw projection has no reader left: it is neither written nor allocated (gt_hip.h: hn_plain)
    plain = fused_ln and _plain_tiles[0] and H.galerkin_ktv_supported(dk, p)
    if _qkvnorm_fused[0] and dk in (16, 32, 48, 64) and bqkv is not None and H.get_precision() in H.SPLIT_EXACT:
        # head norm on the projection's epilogue (GT_EP_HEADNORM): one pass less over [T, 3d], one launch less
        out3 = torch.empty(3, T, h, DP, dtype=torch.float32, device=dev)
        stats = torch.empty(2, T, h, 2, dtype=torch.float32, device=dev)
        if not plain and not token_norm:       # (token_norm: no stream is LayerNormed, nothing reads the raw projection)
            qkv = torch.empty(T, 3 * d, dtype=torch.float32, device=dev)
        try:
            # the raw projection is kept for the LayerNorm backward only: the normalised streams' blocks of qkv
            H.gemm(xc, wq, qkv, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=bqkv, weight_b=True,
                   hn=dict(gamma=hn_gamma, beta=hn_beta, pos=posc, out=out3, stats=stats, h=h, dk=dk, p=p,
                           norm_mask=hn_mask, eps=eps, skip_raw=7 if plain else (~hn_mask) & 7, plain=plain))
        except H.GtNotSupported:                          # shapes / alignment the fused kernel does not take
            out3 = None
    if out3 is None:
        plain = False
        qkv = torch.empty(T, 3 * d, dtype=torch.float32, device=dev)
        H.gemm(xc, wq, qkv, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=bqkv, weight_b=True)
        out3, stats = H.headnorm_fwd(qkv, posc, hn_gamma, hn_beta, T, h, dk, p, hn_mask, eps)
        if token_norm:
            qkv = None
    tn = (None, None, None)
    if token_norm:
        # out3[1:] keep the raw tiles for the backward (xh is recomputed from them: a zero weight must work); the
        # normalised pair goes to its own buffer, which the softmax / contraction chain of the core reads and rewrites
        kvn = torch.empty(2, T, h, DP, dtype=torch.float32, device=dev)
        _, st_k = H.token_norm_fwd(out3[1], gamma[0], beta[0], eps, B, n, h, dk, p, out=kvn[0])
        _, st_v = H.token_norm_fwd(out3[2], gamma[1], beta[1], eps, B, n, h, dk, p, out=kvn[1])
        tn = (kvn, st_k, st_v)
    return qkv, stats, out3, tn, plain


def _project_heads_bwd(s, dO3, ln, g_in, in_mask, dims, norm_mask, token_norm, hbq, has_res):
    """The tail of every backward: the gradient tiles dO3 [3, T, h, DP] (or ``ln`` = (d_qkv, dgamma, dbeta) where the core
    already ran the LayerNorm backward) -> dx (+ its masked twin), d(wqkv), d(bqkv), dgamma, dbeta."""
    B, n, d, h, dk, p, Dr, DP = dims
    T, dev = B * n, g_in.device
    if token_norm:
        dgamma, dbeta = _token_norm_bwd(s, dO3, dims, n)
        # scatter only: the value columns of the three gradient tiles into d_qkv (no stream is LayerNormed, so the raw
        # projection is not read; where the forward did not keep one, the gradient tiles stand in for the pointer)
        dqkv, _, _ = H.headnorm_bwd(dO3, s.qkv if s.qkv is not None else dO3, None, s.stats, T, h, dk, p, 0)
    elif ln is None:
        dqkv, dgamma, dbeta = H.headnorm_bwd(dO3, s.qkv, s.gamma, s.stats, T, h, dk, p, norm_mask)
    else:
        dqkv, dgamma, dbeta = ln
    dwqkv = torch.empty(3 * d, d, dtype=torch.float32, device=dev)
    dbqkv = torch.empty(3 * d, dtype=torch.float32, device=dev) if hbq else None
    dx = torch.empty(T, d, dtype=torch.float32, device=dev)
    with H.side_branch(dev, T):     # weight gradient next to the data gradient
        H.gemm(dqkv, s.xc, dwqkv, 3 * d, d, T, layout_a=1, layout_b=1, lda=3 * d, ldb=d, ldc=d, split_k=0,
               a_colsum=dbqkv)
    dxm = torch.empty_like(dx) if in_mask is not None else None
    # (res is x: its gradient, the unmasked g_in, is folded into dx here and the `res` slot of the backward returns None)
    H.gemm(dqkv, s.wq, dx, T, d, 3 * d, layout_b=1, lda=3 * d, ldb=d, ldc=d, res=g_in if has_res else None,
           ldr=d, weight_b=True, c_masked=dxm, ldc_masked=d,
           c_mask=H.dropout_desc(in_mask[0], in_mask[1], dev) if in_mask else None)
    if dxm is not None:
        _offer_twin(dx, dxm, *in_mask)
    H.join_side(dev)
    if not norm_mask:
        dgamma = dbeta = None
    return dx, dwqkv, dbqkv, dgamma, dbeta


# ----------------------------------------------------------------------------------- the cores
# fwd(c, Qp, Kp, Vp, out, rc) -> (attn_weight, tensors to save, route): from the head tiles to ``out``, written in place;
# ``route`` is the tuple of decisions the core took, decided once there.  bwd(c, s, g, route) -> (dO3, ln, dwfc, dbfc): from
# the masked output gradient g [T, d] and the saved tensors s to the gradient tiles; it follows ``route`` and consults no
# module-level switch.  ``ln`` is None except on the Galerkin core's fused_ln route.  ``c``: _core_call.
def _merged_fc_fwd(c, att, out, rc):
    """fc over the merged heads, shared by the fourier, softmax and causal cores: out = res + sign * dropout(fc(att)) from the
    head outputs att [T, h*DP].  Returns wpad [d, h*DP], the fc weight with zero columns under the tiles' padding (saved
    for _merged_fc_bwd)."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD = B * n, h * DP
    wpad = torch.zeros(d, h, DP, dtype=torch.float32, device=out.device)
    wpad[:, :, :Dr] = c.wf.reshape(d, h, Dr)
    wpad = wpad.reshape(d, hD)
    H.gemm(att, wpad, out, T, d, hD, lda=hD, ldb=hD, ldc=d, bias=c.bfc, drop=c.d_out, res=rc, ldr=d, out_scale=c.sign)
    return wpad


def _merged_fc_bwd(c, s, g):
    """Backward of _merged_fc_fwd from the masked gradient g [T, d], s.att and s.wpad: (datt [T, h*DP], dwfc, dbfc)."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD, dev = B * n, h * DP, g.device
    dwpad = torch.empty(d, hD, dtype=torch.float32, device=dev)
    dbfc = torch.empty(d, dtype=torch.float32, device=dev) if c.has_bias_fc else None
    H.gemm(g, s.att, dwpad, d, hD, T, layout_a=1, layout_b=1, lda=d, ldb=hD, ldc=hD, split_k=0, alpha=c.sign,
           a_colsum=dbfc, a_drop_sign=c.sign)     # (alpha signs the product, a_drop_sign the column sums)
    dwfc = dwpad.reshape(d, h, DP)[:, :, :Dr].reshape(d, h * Dr)
    datt = torch.empty(T, hD, dtype=torch.float32, device=dev)
    H.gemm(g, s.wpad, datt, T, hD, d, layout_b=1, lda=d, ldb=hD, ldc=hD, alpha=c.sign)
    return datt, dwfc, dbfc


def _galerkin_fwd(c, Qp, Kp, Vp, out, rc):
    """galerkin / linear core: M = mask .* (K'^T V')/n, out = res + sign * dropout(fc(Q' M)).  c.affine = (gamma, beta) for
    "plain" tiles, else (None, None).  c.n_kv (cross-attention, else None): K', V' hold n_kv tokens per sample, Q' and out n;
    the sum of K'^T V' runs over the n_kv memory tokens and the divisor stays n, the QUERY count (layers.py:719, 728).
    attn_weight is M; no route to record."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    hD, dev = h * DP, out.device
    m = n if c.n_kv is None else c.n_kv     # tokens of K', V'
    # gt_galerkin_ktv reads the coordinate columns once, from K', for both operands: right for [pos, K], [pos, V]
    streaming = True
    if c.kind == "linear":
        # Q~ = softmax over the head's columns, K~ = softmax over the tokens, both in place: the backward needs the
        # softmax outputs only, and the LayerNorm backward of K reads the raw projection, not the tiles
        H.feature_softmax_fwd(Qp, B * n * h, dk, p, out=Qp)
        H.token_softmax_fwd(Kp, B, m, h, dk, p, out=Kp)
        # ... not for K~, whose coordinate columns went through the token softmax: with coordinates the full tiles are
        # contracted through gt_gemm below
        streaming = p == 0
    slabs = H.galerkin_ktv(Kp, Vp, B, m, h, dk, p, gamma=c.affine[0], beta=c.affine[1]) if streaming else None
    if slabs is None:                                       # head sizes the streaming MFMA kernel does not cover
        slabs = torch.empty(1, B, h, DP, DP, dtype=torch.float32, device=dev)
        H.gemm(Kp, Vp, slabs, DP, DP, m, layout_a=1, layout_b=1, lda=hD, ldb=hD, ldc=DP, batch=(B, h),
               a_bs=(m * hD, DP), b_bs=(m * hD, DP), c_bs=(h * DP * DP, DP * DP), split_k=0)
    Mt, P, Pv = H.galerkin_finalize_fwd(slabs, slabs.shape[0], B * h * DP * DP, B, h, DP, Dr, d, n, c.mask,
                                        c.d_attn, c.wf, value_rows_of=p)
    H.gemm(Qp, P, out, n, d, hD, layout_b=1, lda=hD, ldb=d, ldc=d, batch=(B, 1), a_bs=(n * hD, 0),
           b_bs=(hD * d, 0), c_bs=(n * d, 0), bias=c.bfc, drop=c.d_out, res=rc, ldr=d, r_bs=(n * d, 0),
           out_scale=c.sign)
    return Mt[:, :, :Dr, :Dr], dict(wf=c.wf, Mt=Mt, P=P, Pv=Pv), ()


def _galerkin_bwd(c, s, g, route):
    """Backward of _galerkin_fwd.  dO3 holds the gradient tiles, or with c.fused_ln ln = (d_qkv, dgamma, dbeta) comes from
    gt_galerkin_dkv_ln and dO3 is None.  With c.n_kv (never together with c.fused_ln) dO3 is a triple of tiles: dQ'
    [B*n, h, DP], dK' and dV' [B*n_kv, h, DP]."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD, dev = B * n, h * DP, g.device
    m = n if c.n_kv is None else c.n_kv     # tokens of K', V'
    dbfc = torch.empty(d, dtype=torch.float32, device=dev) if c.has_bias_fc else None
    # (token_norm: the contractions ran on the normalised pair; out3[1:] are the raw tiles)
    Qp, (Kp, Vp) = s.out3[0], (s.kvn if c.token_norm else s.out3[1:])
    # dP^T[b] = (sign*g*mask1)^T[b] Q'[b]        [B, d, h*DP]
    dPt = torch.empty(B, d, hD, dtype=torch.float32, device=dev)
    with H.side_branch(dev, T): # the token-contracted product next to the token-row product below
        H.gemm(g, Qp, dPt, d, hD, n, layout_a=1, layout_b=1, lda=d, ldb=hD, ldc=hD, batch=(B, 1),
               a_bs=(n * d, 0), b_bs=(n * hD, 0), c_bs=(d * hD, 0), split_k=0, alpha=c.sign,
               a_colsum=dbfc, a_drop_sign=c.sign)     # + d(fc bias) = column sums of the masked g; a_drop_sign is ITS sign
    # dQ'[b] = (sign*g*mask1)[b] P[b]^T
    dO3 = dqkv = None
    if c.fused_ln:
        # only the value columns of dQ' reach d_qkv (the coordinates take no gradient): contract with those rows
        # of P and write the Q block of d_qkv directly -- one 128-wide tile column instead of h*DP = 144, no
        # dQ' round trip
        dqkv = torch.empty(T, 3 * d, dtype=torch.float32, device=dev)
        H.gemm(g, s.Pv, dqkv, n, d, d, lda=d, ldb=d, ldc=3 * d, batch=(B, 1), a_bs=(n * d, 0),
               b_bs=(d * d, 0), c_bs=(n * 3 * d, 0), alpha=c.sign)
    else:
        if c.n_kv is None:
            dO3 = torch.empty(3, T, h, DP, dtype=torch.float32, device=dev)
        else:
            dO3 = tuple(torch.empty(B * r, h, DP, dtype=torch.float32, device=dev) for r in (n, m, m))
        H.gemm(g, s.P, dO3[0], n, hD, d, lda=d, ldb=d, ldc=hD, batch=(B, 1), a_bs=(n * d, 0),
               b_bs=(hD * d, 0), c_bs=(n * hD, 0), alpha=c.sign)
    H.join_side(dev)
    dM, dWs = H.galerkin_finalize_bwd(dPt, s.Mt, c.mask, c.d_attn, s.wf, B, h, DP, Dr, d, n)
    dwfc = torch.empty(d, h * Dr, dtype=torch.float32, device=dev)
    H.slab_reduce(dWs, B, d * h * Dr, d * h * Dr, dwfc)
    # dK' = V' dM^T ; dV' = K' dM          per (b, head)
    ln = None
    if c.fused_ln:       # ... with the head LayerNorm backward behind them: dK', dV' stay in registers
        ln = H.galerkin_dkv_ln(Kp, Vp, dM, None, s.qkv, s.gamma, s.stats, B, n, h, dk, p, d_qkv=dqkv,
                               beta=s.beta if c.plain else None)
    elif DP in H.FOURIER_DP:                           # one streaming pass (gt_galerkin_dkv)
        H.galerkin_dkv(Kp, Vp, dM, dO3[1], dO3[2], B, m, h, DP)
    else:
        H.gemm(Vp, dM, dO3[1], m, DP, DP, lda=hD, ldb=DP, ldc=hD, batch=(B, h), a_bs=(m * hD, DP),
               b_bs=(h * DP * DP, DP * DP), c_bs=(m * hD, DP))
        H.gemm(Kp, dM, dO3[2], m, DP, DP, layout_b=1, lda=hD, ldb=DP, ldc=hD, batch=(B, h),
               a_bs=(m * hD, DP), b_bs=(h * DP * DP, DP * DP), c_bs=(m * hD, DP))
    if c.kind == "linear":
        # (the softmax backwards sit between dK' and the LayerNorm backward, so the fused kernel never applies here)
        # Qp, Kp hold Q~, K~: dQ' = Q~ .* (dQ~ - sum_c Q~ dQ~), dK' = K~ .* (dK~ - sum_t K~ dK~), in place
        H.feature_softmax_bwd(Qp, dO3[0], T * h, dk, p, out=dO3[0])
        H.token_softmax_bwd(Kp, dO3[1], B, m, h, dk, p, out=dO3[1])
    return dO3, ln, dwfc, dbfc


def _fourier_fwd(c, Qp, Kp, Vp, out, rc):
    """fourier core: S = mask .* (Q' K'^T)/sqrt(d_k')/n, out = res + sign * dropout(fc(S V')), on one of three routes: fused
    fp32, fused two-term fp16 (with the presplit images kept for the backward), or materialised S (the attn_weight).
    route = (flash, f16, block16)."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD, dev = B * n, h * DP, out.device
    mask, d_attn = c.mask, c.d_attn
    hd_bs, nn_bs = (n * hD, DP), (h * n * n, n * n)      # batch strides over (sample, head): head tiles, n x n matrices
    scale = 1.0 / math.sqrt(Dr) / n
    # fp16 arithmetic active: every width of the fp16 kernel runs on it; otherwise (f32 / bf16 modes) the fp32-MFMA kernel,
    # which has the same widths behind two entry points (H.fourier_attn picks)
    flash = (not c.need_w) and (DP in H.FOURIER_DP + H.FOURIER_DP_WIDE or (DP in H.FOURIER16_DP and H.fourier16_active()))
    f16 = flash and H.fourier16_active()
    # fp16 arithmetic: the p = 0.5 score mask is drawn per 4 x 4 block (one hash per block: gt_hip.h), by the fused
    # kernels and by the materialising path alike
    block16 = bool(H.fourier16_active() and d_attn is not None and H.fourier16_block_mask(d_attn))
    S = iq = ik = iv = None
    if f16:
        # fused (Q'K'^T * scale .* mask) V': the n x n matrix never reaches HBM.  Two-term fp16 kernels: the head tiles
        # are split once into fragment-ordered images, kept for the backward
        iq, ik, iv = H.fourier16_presplit((Qp, Kp, Vp), B, n, h, DP)
        att = H.fourier16_attn(iq, None, ik, iv, B, n, h, DP, scale, mask, d_attn, False, block16=block16).reshape(T, hD)
    elif flash:
        att = H.fourier_attn(Qp, None, Kp, Vp, B, n, h, DP, scale, mask, d_attn, False).reshape(T, hD)
    else:
        S = torch.empty(B, h, n, n, dtype=torch.float32, device=dev)
        H.gemm(Qp, Kp, S, n, n, DP, lda=hD, ldb=hD, ldc=n, batch=(B, h), a_bs=hd_bs, b_bs=hd_bs, c_bs=nn_bs, alpha=scale,
               drop=None if block16 else d_attn, aux_op=H.AUX_MUL if mask is not None else H.AUX_NONE, aux=mask, ldaux=n,
               aux_bs=nn_bs)
        if block16:
            H.dropout_block16(S, B * h, n, d_attn)
        att = torch.empty(T, hD, dtype=torch.float32, device=dev)
        H.gemm(S, Vp, att, n, DP, n, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs, b_bs=hd_bs, c_bs=hd_bs)
    wpad = _merged_fc_fwd(c, att, out, rc)
    attn_w = S if S is not None else torch.empty(0, device=dev)
    return attn_w, dict(wpad=wpad, S=S, att=att, iq=iq, ik=ik, iv=iv), (flash, f16, block16)


def _fourier_bwd(c, s, g, route):
    """Backward of _fourier_fwd on the route it took."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD, dev = B * n, h * DP, g.device
    mask, d_attn = c.mask, c.d_attn
    flash, f16, block16 = route
    hd_bs, nn_bs = (n * hD, DP), (h * n * n, n * n)      # batch strides over (sample, head): head tiles, n x n matrices
    dO3 = torch.empty(3, T, h, DP, dtype=torch.float32, device=dev)
    Qp, Kp, Vp = s.out3[0], s.out3[1], s.out3[2]
    scale = 1.0 / math.sqrt(Dr) / n
    datt, dwfc, dbfc = _merged_fc_bwd(c, s, g)
    datt3 = datt.reshape(T, h, DP)
    if f16:       # fused passes: dQ' = (dO V'^T .* m) K' ;  dV' = (S .* m)^T dO, dK' = (dO V'^T .* m)^T Q'
        (ido,) = H.fourier16_presplit((datt3,), B, n, h, DP)
        H.fourier16_attn(ido, None, s.iv, s.ik, B, n, h, DP, scale, mask, d_attn, False, O1=dO3[0], block16=block16)
        H.fourier16_attn(s.ik, s.iv, s.iq, ido, B, n, h, DP, scale, mask, d_attn, True, O1=dO3[2], O2=dO3[1],
                         block16=block16)
    elif flash:
        H.fourier_attn(datt3, None, Vp, Kp, B, n, h, DP, scale, mask, d_attn, False, O1=dO3[0])
        H.fourier_attn(Kp, Vp, Qp, datt3, B, n, h, DP, scale, mask, d_attn, True, O1=dO3[2], O2=dO3[1])
    else:
        dS = torch.empty(B, h, n, n, dtype=torch.float32, device=dev)
        H.gemm(datt, Vp, dS, n, n, DP, lda=hD, ldb=hD, ldc=n, batch=(B, h), a_bs=hd_bs, b_bs=hd_bs, c_bs=nn_bs, alpha=scale,
               drop=None if block16 else d_attn, aux_op=H.AUX_MUL if mask is not None else H.AUX_NONE, aux=mask, ldaux=n,
               aux_bs=nn_bs)
        if block16:
            H.dropout_block16(dS, B * h, n, d_attn)
        # dV' = S^T datt ; dQ' = dS K' ; dK' = dS^T Q'
        H.gemm(s.S, datt, dO3[2], n, DP, n, layout_a=1, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs,
               b_bs=hd_bs, c_bs=hd_bs)
        H.gemm(dS, Kp, dO3[0], n, DP, n, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs, b_bs=hd_bs, c_bs=hd_bs)
        H.gemm(dS, Qp, dO3[1], n, DP, n, layout_a=1, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs,
               b_bs=hd_bs, c_bs=hd_bs)
    return dO3, None, dwfc, dbfc


def _softmax_fwd(c, Qp, Kp, Vp, out, rc):
    """softmax core: P = softmax(Q' K'^T / sqrt(d_k')), out = res + sign * dropout(fc((P .* mask) V')), fused (gt_softmax_attn_*:
    no n x n matrix in HBM; gt_softmax_attn_wide_* at DP 68 / 100) or, when the weights are wanted, materialised (gt_gemm +
    gt_row_softmax_*).  The attention runs in fp32 on both routes in every precision mode; the fc product follows
    set_precision.  attn_weight = P .* mask; route = (flash,)."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD, dev = B * n, h * DP, out.device
    hd_bs, nn_bs = (n * hD, DP), (h * n * n, n * n)      # batch strides over (sample, head): head tiles, n x n matrices
    scale = 1.0 / math.sqrt(Dr)
    flash = not c.need_w
    P = Pm = L = None
    if flash:
        att, L = H.softmax_attn_fwd(Qp, Kp, Vp, B, n, h, DP, scale, c.mask, c.d_attn)
        att = att.reshape(T, hD)
    else:
        P = torch.empty(B, h, n, n, dtype=torch.float32, device=dev)
        H.gemm(Qp, Kp, P, n, n, DP, lda=hD, ldb=hD, ldc=n, batch=(B, h), a_bs=hd_bs, b_bs=hd_bs, c_bs=nn_bs, alpha=scale,
               precision="f32")
        P, Pm = H.row_softmax_fwd(P, B * h * n, n, c.mask, c.d_attn, P=P)      # in place; Pm is P without mask and dropout
        att = torch.empty(T, hD, dtype=torch.float32, device=dev)
        H.gemm(Pm, Vp, att, n, DP, n, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs, b_bs=hd_bs, c_bs=hd_bs,
               precision="f32")
    wpad = _merged_fc_fwd(c, att, out, rc)
    attn_w = Pm if Pm is not None else torch.empty(0, device=dev)
    return attn_w, dict(wpad=wpad, att=att, L=L, P=P, Pm=Pm), (flash,)


def _softmax_bwd(c, s, g, route):
    """Backward of _softmax_fwd on the route it took."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T, hD, dev = B * n, h * DP, g.device
    (flash,) = route
    hd_bs, nn_bs = (n * hD, DP), (h * n * n, n * n)      # batch strides over (sample, head): head tiles, n x n matrices
    dO3 = torch.empty(3, T, h, DP, dtype=torch.float32, device=dev)
    Qp, Kp, Vp = s.out3[0], s.out3[1], s.out3[2]
    scale = 1.0 / math.sqrt(Dr)
    datt, dwfc, dbfc = _merged_fc_bwd(c, s, g)
    if flash:     # dQ' (and D), then dK', dV': P = exp(S - L) recomputed tile by tile
        H.softmax_attn_bwd(datt.reshape(T, h, DP), s.att.reshape(T, h, DP), Qp, Kp, Vp, s.L, B, n, h, DP, scale, c.mask,
                           c.d_attn, dQ=dO3[0], dK=dO3[1], dV=dO3[2])
    else:
        dS = torch.empty(B, h, n, n, dtype=torch.float32, device=dev)
        H.gemm(datt, Vp, dS, n, n, DP, lda=hD, ldb=hD, ldc=n, batch=(B, h), a_bs=hd_bs, b_bs=hd_bs,
               c_bs=nn_bs, precision="f32")                                # dPm = dO V'^T
        H.row_softmax_bwd(s.P, dS, B * h * n, n, c.mask, c.d_attn, dS=dS)   # dS = P .* (m .* dPm - sum P m dPm), in place
        # dV' = Pm^T datt ; dQ' = dS K' / sqrt(d_k') ; dK' = dS^T Q' / sqrt(d_k')
        H.gemm(s.Pm, datt, dO3[2], n, DP, n, layout_a=1, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs,
               b_bs=hd_bs, c_bs=hd_bs, precision="f32")
        H.gemm(dS, Kp, dO3[0], n, DP, n, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs,
               b_bs=hd_bs, c_bs=hd_bs, alpha=scale, precision="f32")
        H.gemm(dS, Qp, dO3[1], n, DP, n, layout_a=1, layout_b=1, lda=n, ldb=hD, ldc=hD, batch=(B, h), a_bs=nn_bs,
               b_bs=hd_bs, c_bs=hd_bs, alpha=scale, precision="f32")
    return dO3, None, dwfc, dbfc


_CAUSAL_EPS = 1e-7      # causal_linear_attn's default eps (layers.py:736); SimpleAttention does not pass another


def _causal_fwd(c, Qp, Kp, Vp, out, rc):
    """causal core: att_i = S_i^T q_i / den_i with S_i = sum_{j<=i} k^_j v^_j^T, k^ = keep K' / n, v^ = keep V'
    (gt_causal_attn_fwd: chunked scan, linear in n), out = res + sign * dropout(fc(att)).  c.keep [B, n] uint8 or None.  No
    attention dropout, no attention weight, no route to record; den and the per-chunk prefix states are kept for the
    backward."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    att, den, states = H.causal_attn_fwd(Qp, Kp, Vp, c.keep, B, n, h, DP, _CAUSAL_EPS)
    att = att.reshape(B * n, h * DP)
    wpad = _merged_fc_fwd(c, att, out, rc)
    return torch.empty(0, device=out.device), dict(wpad=wpad, att=att, den=den, states=states), ()


def _causal_bwd(c, s, g, route):
    """Backward of _causal_fwd."""
    B, n, d, h, dk, p, Dr, DP = c.dims
    T = B * n
    dO3 = torch.empty(3, T, h, DP, dtype=torch.float32, device=g.device)
    datt, dwfc, dbfc = _merged_fc_bwd(c, s, g)
    H.causal_attn_bwd(datt.reshape(T, h, DP), s.att.reshape(T, h, DP), s.out3[0], s.out3[1], s.out3[2], c.keep, s.den,
                      s.states, B, n, h, DP, Dr, _CAUSAL_EPS, dQ=dO3[0], dK=dO3[1], dV=dO3[2])
    return dO3, None, dwfc, dbfc


# kind -> (fwd, bwd).  A new kind is one entry here and one core pair above.
_CORES = {"galerkin": (_galerkin_fwd, _galerkin_bwd), "linear": (_galerkin_fwd, _galerkin_bwd),
          "fourier": (_fourier_fwd, _fourier_bwd), "softmax": (_softmax_fwd, _softmax_bwd),
          "causal": (_causal_fwd, _causal_bwd)}


# ----------------------------------------------------------------------------------- self-attention
class SimpleAttentionFn(Function):
    """out = res + sign * dropout1( fc( merge_heads( attention(Q', K', V') ) ) ).

    galerkin: per-head LN on K,V; M = mask .* (K'^T V')/n; heads: Q' M      (layers.py:708-734)
    linear  : the same on Q~ = softmax(Q', dim=-1), K~ = softmax(K', dim=-2)  (layers.py:719-722; 'global' too)
    fourier : per-head LN on Q,K; S = mask .* (Q' K'^T)/sqrt(d_k')/n; heads: S V' (layers.py:672-705)
    softmax : per-head LN on Q,K; P = softmax(Q' K'^T/sqrt(d_k')); heads: (mask .* P) V'  (layers.py:691-703)
    causal  : per-head LN on Q,K; heads: tril(Q' K^'^T) V^' / (its row sums + eps sum_d q) (layers.py:736-762); the ``mask``
              argument is then the keep vector [B, n] (uint8) or None, and no attention dropout is drawn
    with X' = [pos, X] per head (layers.py:869-874) and fc over the merged heads (layers.py:894-897).
    token_norm (norm_type='instance', galerkin / linear): K, V are normalised over the TOKENS per (sample, head, channel)
    instead (layers.py:842-854): the projection writes raw tiles, gt_token_norm_fwd normalises their value columns.
    Also returns the attention matrix (``attn_weight``), detached.

    One autograd node in two stages.  forward: _project_heads (QKV projection, head norm, token norm; shared), then the core
    of the kind from _CORES, which ends in the fc product that writes ``out`` (fourier, softmax and causal share that stage:
    _merged_fc_fwd / _merged_fc_bwd; galerkin folds fc into P).  backward: the core's other half, then _project_heads_bwd.
    Forward to backward: the tensors go by name through _save_named / _saved; ctx.cfg (an AttnConfig, share = "self"),
    ctx.dims, ctx.salt, ctx.has (bqkv, bfc, res given), ctx.xshape and ctx.in_mask carry the call; ctx.route is what the core
    recorded of its own decisions, and ctx.plain, ctx.fused_ln are the two that the projection stage takes.  They stay on ctx
    (the core namespace ``c`` of _core_call is rebuilt from ctx in the backward and only copies them).  The backward follows
    them and consults no module-level switch."""

    @staticmethod
    def forward(ctx, x, pos, wqkv, bqkv, gamma, beta, wfc, bfc, res, cfg, mask):
        dims = B, n, d, h, dk, p, Dr, DP = _head_dims(x.shape, cfg.h, pos)
        mask, keep = (None, mask) if cfg.kind == "causal" else (mask, None)     # keep [B, n] (uint8) came in the mask slot
        H.need_f32_cuda(x, pos, wqkv, bqkv, gamma, beta, wfc, bfc, res, mask)
        _check_config("simple_attention", cfg, dk, p, ("n", n), gamma, beta, nopos_ok=True)
        T, dev = B * n, x.device
        # the Galerkin backward with the head LayerNorm backward fused in (gt_galerkin_dkv_ln); not for linear, whose softmax
        # backwards sit between dK' and the LayerNorm backward
        fused_ln = (cfg.kind == "galerkin" and not cfg.token_norm and _dkv_ln_fused[0]
                    and H.galerkin_dkv_ln_supported(dk, p, cfg.norm_mask))
        xc = _c(x).reshape(T, d)
        posc = None if pos is None else _c(pos).reshape(T, p)
        wq = _c(wqkv)
        salt = _next_salt(4)
        qkv, stats, out3, (kvn, st_k, st_v), plain = _project_heads(xc, posc, wq, bqkv, gamma, beta, dims, cfg.norm_mask,
                                                                    cfg.eps, cfg.token_norm, fused_ln)
        Qp, Kp, Vp = (out3[0], kvn[0], kvn[1]) if cfg.token_norm else (out3[0], out3[1], out3[2])
        out = torch.empty(T, d, dtype=torch.float32, device=dev)
        rc = None if res is None else _c(res).reshape(T, d)
        c = _core_call(cfg, dims, salt, dev, mask, keep, bfc is not None, plain=plain, fused_ln=fused_ln, wf=_c(wfc), bfc=bfc,
                       affine=(gamma, beta) if plain else (None, None))
        attn_w, core, ctx.route = _CORES[cfg.kind][0](c, Qp, Kp, Vp, out, rc)
        _save_named(ctx, xc=xc, wq=wq, gamma=gamma, beta=beta, qkv=qkv, stats=stats, out3=out3, kvn=kvn, st_k=st_k,
                    st_v=st_v, mask=mask, keep=keep, **core)
        ctx.plain, ctx.fused_ln = plain, fused_ln
        ctx.cfg, ctx.dims, ctx.salt, ctx.xshape = cfg, dims, salt, x.shape
        ctx.has = (bqkv is not None, bfc is not None, res is not None)
        ctx.in_mask = _wanted_mask(xc)
        _hint_output_mask(out, cfg.p_out, salt + 1)
        attn_w = attn_w.detach()
        ctx.mark_non_differentiable(attn_w)
        return out.reshape(x.shape), attn_w

    @staticmethod
    def backward(ctx, gy, _gw):
        cfg, salt = ctx.cfg, ctx.salt
        B, n, d = ctx.dims[:3]
        hbq, hbf, has_res = ctx.has
        s = _saved(ctx)
        c = _core_call(cfg, ctx.dims, salt, gy.device, s.mask, s.keep, hbf, plain=ctx.plain, fused_ln=ctx.fused_ln)
        g_in = _c(gy).reshape(B * n, d)                     # unmasked: what flows to the residual branch
        g = _masked_out_grad(g_in, c.d_out, twin=lambda t: _take_twin(t, cfg.p_out, salt + 1))
        dO3, ln, dwfc, dbfc = _CORES[cfg.kind][1](c, s, g, ctx.route)
        dx, dwqkv, dbqkv, dgamma, dbeta = _project_heads_bwd(s, dO3, ln, g_in, ctx.in_mask, ctx.dims, cfg.norm_mask,
                                                             cfg.token_norm, hbq, has_res)
        return (dx.reshape(ctx.xshape), None, dwqkv, dbqkv, dgamma, dbeta, dwfc, dbfc, None, None, None)


def simple_attention(x, pos, wqkv, bqkv, gamma, beta, wfc, bfc, *, kind: str, n_head: int, norm_mask: int,
                     eps: float, res=None, sign: float = 1.0, p_out: float = 0.0, need_weights: bool = True,
                     token_norm: bool = False, keep=None):
    """Self-attention block; ``res`` must be ``x`` (or None).  Returns (out, attn_weight).  For the Fourier and softmax
    types ``need_weights=False`` selects the fused kernel that never materialises the n x n matrix
    (attn_weight is then None); the Galerkin matrix is small and always returned.  ``token_norm`` (galerkin / linear with
    norm_mask = K, V): gamma / beta are the affine of the token-axis norm (norm_type='instance') instead of the LayerNorm's.
    kind='causal': ``keep`` [B, n] (uint8, 0 = the key / value token is dropped) or None; the attention dropout mode is not
    consulted (the reference's dropout acts on the running state, which never exists here) and attn_weight is None."""
    _check_res_is_x(res, x, "simple_attention")
    mask, p_attn = _attn_dropout_setup("simple_attention", kind, keep, x.device)
    cfg = _config(kind, n_head, norm_mask, eps, sign, p_attn, p_out, need_weights, token_norm, "self")
    out, w = SimpleAttentionFn.apply(x, pos, wqkv, bqkv, gamma, beta, wfc, bfc, res, cfg, mask)
    return out, (w if w.numel() else None)


def multihead_attention(x, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, *, n_head: int,
                        p_attn: float = 0.0, res=None, sign: float = 1.0, p_out: float = 0.0, need_weights: bool = False,
                        replay_mask=None):
    """The attention of the classic Transformer layer (nn.MultiheadAttention with its packed in_proj, batch first):
        [q, k, v] = x in_proj_weight^T + in_proj_bias, split into n_head heads of d_k = d / n_head
        P = softmax(q k^T / sqrt(d_k)) over the keys,  Pm = P .* m
        out = res + sign * dropout_{p_out}( out_proj( merge_heads(Pm v) ) )
    m: a stateless dropout of rate ``p_attn`` on the softmax OUTPUT, rescaled by 1 / (1 - p_attn) (the caller passes 0 in eval),
    or the explicit multiplicative ``replay_mask`` [B, h, n, n] (parity tests), or 1.  ``p_attn`` is the caller's own rate: the
    set_attention_dropout switch, which models the reference's SimpleAttention, is not consulted.

    One SimpleAttentionFn node of kind 'softmax': the shared projection with no coordinates and no head norm (head tiles
    exactly d_k wide), then the softmax core with out_proj in fc's place.  ``need_weights=False``: the fused tail-free
    kernels (gt_softmax_attn_nopos_*), no n x n matrix in HBM, returns (out, None).  ``need_weights=True``: the materialised
    route, returns (out, w) with w [B, n, n] the mean of Pm over the heads (average_attn_weights=True), detached.
    d_k outside H.SOFTMAX_DP_NOPOS raises GtNotSupported before anything is launched."""
    h = int(n_head)
    assert x.dim() == 3 and x.size(-1) % h == 0, "multihead_attention: x is [B, n, d] with d divisible by n_head"
    dk = x.size(-1) // h
    if dk not in H.SOFTMAX_DP_NOPOS:
        raise H.GtNotSupported(f"multihead_attention: head width d_k = {dk} has no kernel (supported: {H.SOFTMAX_DP_NOPOS})")
    _check_res_is_x(res, x, "multihead_attention")
    mask = None
    if replay_mask is not None:
        mask = _c(replay_mask.to(device=x.device, dtype=torch.float32))
        assert mask.shape == (x.size(0), h, x.size(1), x.size(1)), "multihead_attention: replay_mask is [B, h, n, n]"
    cfg = _config("softmax", h, 0, 0.0, sign, 0.0 if mask is not None else p_attn, p_out, need_weights, False, "self")
    out, w = SimpleAttentionFn.apply(x, None, in_proj_weight, in_proj_bias, None, None, out_proj_weight, out_proj_bias, res,
                                     cfg, mask)
    return out, (w.mean(dim=1) if w.numel() else None)


# ----------------------------------------------------------------------------------- cross-attention
# which of (query, key, value) are one tensor -> the projection groups (first stream, number of streams): a group is one
# input, one product against its rows of the packed weight, one data-gradient and one weight-gradient product
_CROSS_GROUPS = {"none": ((0, 1), (1, 1), (2, 1)), "kv": ((0, 1), (1, 2)), "qk": ((0, 2), (2, 1))}


def _stream_norm(s, norm_mask, token_norm):
    """Index into gamma / beta [2, h, dk] of stream s (0 = Q, 1 = K, 2 = V) when the head LayerNorm runs on it, else None."""
    if token_norm or not (norm_mask >> s) & 1:
        return None
    return bin(norm_mask & ((1 << s) - 1)).count("1")


def check_cross_shapes(query, key, value, pos):
    """The shape contracts of cross-attention, AssertionErrors raised before anything is launched."""
    assert query.dim() == 3 and key.dim() == 3 and value.dim() == 3 and query.size(-1) == key.size(-1) == value.size(-1), \
        "cross_attention: query, key, value are [B, n, d]"
    assert query.size(0) == key.size(0) == value.size(0), \
        f"cross_attention: batch sizes differ ({query.size(0)}, {key.size(0)}, {value.size(0)})"
    assert key.size(1) == value.size(1), f"cross_attention: key has {key.size(1)} tokens, value {value.size(1)}"
    assert pos is None or (query.size(1) == key.size(1) == pos.size(1)), \
        f"cross_attention: pos is concatenated to Q, K and V alike, so n_q = {query.size(1)}, n_kv = {key.size(1)} and " \
        f"pos.size(1) = {pos.size(1)} must be equal"


class CrossAttentionFn(Function):
    """SimpleAttentionFn for query [B, n_q, d], key and value [B, n_kv, d] that are not one tensor (layers.py:829-899):
    Q = linears[0](query), K = linears[1](key), V = linears[2](value), then the same head norms, cores and fc.

    cfg.share names the inputs that are one tensor: "kv" (key is value; the ``value`` argument is None), "qk" (query is key;
    ``key`` is None) or "none".  Projection: one plain gt_gemm per distinct input against its contiguous rows of the packed
    weight (N = 2d for a shared pair), then gt_headtile_fwd per stream on its column block, then the token norm of K, V
    (norm_type='instance').  Cores: the _CORES entries behind _check_config and _core_call, as in the self node: the Galerkin
    pair with n_kv (never the plain / fused_ln routes, which assume one joint [T, 3 h dk] gradient buffer), the others as they
    are (n_q == n_kv); the tiles are saved as ``out3`` and the normalised pair as ``kvn``, the names the cores read.  Backward:
    gt_headtile_bwd per stream into its column block, then per input one data-gradient and one weight-gradient product (the
    latter on the side branch, the bias gradient on its a_colsum); a shared input's two contributions are summed by its one
    data-gradient product over K = 2d.  ``res`` must be ``query``.  No part in the dropout-mask hand-off of ops/_handoff.py."""

    @staticmethod
    def forward(ctx, query, key, value, pos, wqkv, bqkv, gamma, beta, wfc, bfc, res, cfg, mask):
        kind, norm_mask, token_norm = cfg.kind, cfg.norm_mask, cfg.token_norm
        groups = _CROSS_GROUPS[cfg.share]
        xs = {"none": (query, key, value), "kv": (query, key, key), "qk": (query, query, value)}[cfg.share]
        dims = B, n, d, h, dk, p, Dr, DP = _head_dims(query.shape, cfg.h, pos)
        m, dev = xs[1].shape[1], query.device
        assert kind in ("galerkin", "linear") or n == m, (kind, n, m)      # (cross_attention refuses it with its reason)
        mask, keep = (None, mask) if kind == "causal" else (mask, None)     # keep [B, n_kv] (uint8) came in the mask slot
        H.need_f32_cuda(query, key, value, pos, wqkv, bqkv, gamma, beta, wfc, bfc, res, mask)
        _check_config("cross_attention", cfg, dk, p, ("n_kv", m), gamma, beta, nopos_ok=False)
        rows = (B * n, B * m, B * m)
        posc = None if pos is None else _c(pos).reshape(B * n, p)
        wq = _c(wqkv)
        salt = _next_salt(4)
        xcs, projs, tiles, stats = [None] * 3, [None] * 3, [None] * 3, [None] * 3     # (xcs, projs: by the group's first stream)
        for s0, ns in groups:
            T = rows[s0]
            xc = xcs[s0] = _c(xs[s0]).reshape(T, d)
            proj = torch.empty(T, ns * d, dtype=torch.float32, device=dev)
            H.gemm(xc, wq[s0 * d:(s0 + ns) * d], proj, T, ns * d, d, lda=d, ldb=d, ldc=ns * d,
                   bias=None if bqkv is None else bqkv[s0 * d:(s0 + ns) * d])
            for s in range(s0, s0 + ns):
                ni = _stream_norm(s, norm_mask, token_norm)
                tiles[s], stats[s] = H.headtile_fwd(proj[:, (s - s0) * d:], ns * d, posc, None if ni is None else gamma[ni],
                                                    None if ni is None else beta[ni], T, h, dk, p, cfg.eps)
                if ni is not None:      # the LayerNorm backward reads the raw projection
                    projs[s0] = proj
        kvn, st_k, st_v = None, None, None
        if token_norm:
            # tiles[1:] keep the raw K, V for the backward; the normalised pair is what the core reads and rewrites
            kvn_k, st_k = H.token_norm_fwd(tiles[1], gamma[0], beta[0], cfg.eps, B, m, h, dk, p)
            kvn_v, st_v = H.token_norm_fwd(tiles[2], gamma[1], beta[1], cfg.eps, B, m, h, dk, p)
            kvn = (kvn_k, kvn_v)
        Qp, Kp, Vp = (tiles[0], *kvn) if token_norm else tiles
        out = torch.empty(B * n, d, dtype=torch.float32, device=dev)
        rc = None if res is None else _c(res).reshape(B * n, d)
        c = _core_call(cfg, dims, salt, dev, mask, keep, bfc is not None, n_kv=m, wf=_c(wfc), bfc=bfc)
        attn_w, core, ctx.route = _CORES[kind][0](c, Qp, Kp, Vp, out, rc)
        _save_named(ctx, wq=wq, gamma=gamma, xcs=tuple(xcs), projs=tuple(projs), stats=tuple(stats), out3=tuple(tiles),
                    kvn=kvn, st_k=st_k, st_v=st_v, mask=mask, keep=keep, **core)
        ctx.cfg, ctx.dims, ctx.n_kv, ctx.salt = cfg, dims, m, salt
        ctx.has = (bqkv is not None, bfc is not None, res is not None)
        attn_w = attn_w.detach()
        ctx.mark_non_differentiable(attn_w)
        return out.reshape(query.shape), attn_w

    @staticmethod
    def backward(ctx, gy, _gw):
        cfg, m = ctx.cfg, ctx.n_kv
        norm_mask, token_norm = cfg.norm_mask, cfg.token_norm
        B, n, d, h, dk, p, Dr, DP = ctx.dims
        hbq, hbf, has_res = ctx.has
        dev = gy.device
        s = _saved(ctx)
        c = _core_call(cfg, ctx.dims, ctx.salt, dev, s.mask, s.keep, hbf, n_kv=m)
        g_in = _c(gy).reshape(B * n, d)                     # unmasked: what flows to the residual branch
        g = _masked_out_grad(g_in, c.d_out)                 # (no twin: this node takes no part in the hand-off)
        dO3, _, dwfc, dbfc = _CORES[cfg.kind][1](c, s, g, ctx.route)
        dgamma = dbeta = None
        if token_norm:
            dgamma, dbeta = _token_norm_bwd(s, dO3, ctx.dims, m)
        elif norm_mask:
            dgamma = torch.empty(2, h, dk, dtype=torch.float32, device=dev)
            dbeta = torch.empty(2, h, dk, dtype=torch.float32, device=dev)
        rows = (B * n, B * m, B * m)
        dwqkv = torch.empty(3 * d, d, dtype=torch.float32, device=dev)
        dbqkv = torch.empty(3 * d, dtype=torch.float32, device=dev) if hbq else None
        dxs = [None] * 3
        for s0, ns in _CROSS_GROUPS[cfg.share]:
            T, r0, r1 = rows[s0], s0 * d, (s0 + ns) * d
            dproj = torch.empty(T, ns * d, dtype=torch.float32, device=dev)
            for st in range(s0, s0 + ns):
                ni = _stream_norm(st, norm_mask, token_norm)
                col = (st - s0) * d
                if ni is None:      # scatter only: the value columns of the gradient tile
                    H.headtile_bwd(dO3[st], None, 0, None, None, T, h, dk, p, dproj[:, col:], ns * d)
                else:
                    H.headtile_bwd(dO3[st], s.projs[s0][:, col:], ns * d, s.gamma[ni], s.stats[st], T, h, dk, p,
                                   dproj[:, col:], ns * d, dgamma[ni], dbeta[ni])
            with H.side_branch(dev, T):     # weight gradient next to the data gradient
                H.gemm(dproj, s.xcs[s0], dwqkv[r0:r1], ns * d, d, T, layout_a=1, layout_b=1, lda=ns * d, ldb=d, ldc=d,
                       split_k=0, a_colsum=None if dbqkv is None else dbqkv[r0:r1])
            dx = dxs[s0] = torch.empty(T, d, dtype=torch.float32, device=dev)
            # (res is query: its gradient, the unmasked g_in, is folded into d(query) and the `res` slot returns None)
            H.gemm(dproj, s.wq[r0:r1], dx, T, d, ns * d, layout_b=1, lda=ns * d, ldb=d, ldc=d,
                   res=g_in if (has_res and s0 == 0) else None, ldr=d)
            H.join_side(dev)
        dq, dkey, dval = (None if t is None else t.reshape(B, -1, d) for t in dxs)
        return (dq, dkey, dval, None, dwqkv, dbqkv, dgamma, dbeta, dwfc, dbfc, None, None, None)


def cross_attention(query, key, value, pos, wqkv, bqkv, gamma, beta, wfc, bfc, *, kind: str, n_head: int, norm_mask: int,
                    eps: float, res=None, sign: float = 1.0, p_out: float = 0.0, need_weights: bool = True,
                    token_norm: bool = False, keep=None):
    """Attention block over query [B, n_q, d] and key, value [B, n_kv, d] that are not one tensor; ``res`` must be
    ``query`` (or None).  Returns (out [B, n_q, d], attn_weight).  galerkin / linear: any n_q, n_kv (with ``pos`` they are
    equal), M = (K'^T V') / n_q -- the sum over the n_kv memory tokens, the divisor the QUERY count (layers.py:719, 728).
    fourier / softmax: n_q == n_kv, else NotImplementedError.  ``key is value`` and ``query is key`` are projected as one
    product and their input receives one summed gradient.  The attention dropout modes act as in simple_attention.
    kind='causal': n_q == n_kv (AssertionError otherwise: the reference's reshape needs it too), ``keep`` [B, n_kv] (uint8) or
    None masks the memory tokens, no attention dropout, attn_weight None."""
    check_cross_shapes(query, key, value, pos)
    _check_res_is_x(res, query, "cross_attention")
    if kind == "causal":
        assert query.size(1) == key.size(1), \
            f"cross_attention: kind='causal' needs n_q == n_kv (got {query.size(1)}, {key.size(1)})"
    if kind in ("fourier", "softmax") and query.size(1) != key.size(1):
        raise NotImplementedError(f"cross_attention: kind={kind!r} with n_q={query.size(1)} != n_kv={key.size(1)}: the fused "
                                  "kernels take one token count")
    if token_norm:      # a shape contract like the ones above: refused without a device (the node states it again)
        _check_token_count(key.size(1), "n_kv")
    share = "kv" if key is value else ("qk" if query is key else "none")
    mask, p_attn = _attn_dropout_setup("cross_attention", kind, keep, query.device)
    cfg = _config(kind, n_head, norm_mask, eps, sign, p_attn, p_out, need_weights, token_norm, share)
    out, w = CrossAttentionFn.apply(query, key if share != "qk" else None, value if share != "kv" else None, pos, wqkv, bqkv,
                                    gamma, beta, wfc, bfc, res, cfg, mask)
    return out, (w if w.numel() else None)


# ----------------------------------------------------------------------------------- the causal core alone
class CausalLinearAttnFn(Function):
    """causal_linear_attn (layers.py:736-762) on [B, h, n, D] tensors: the tensors are laid out as token-major head tiles
    [B*n, h, round4(D)] with zero pad columns (a torch copy), then gt_causal_attn_fwd / _bwd."""

    @staticmethod
    def forward(ctx, q, k, v, keep, eps):
        B, h, n, D = q.shape
        DP = H.round4(D)
        H.causal_check(DP)
        H.need_f32_cuda(q, k, v)

        def tile(t):
            out = torch.zeros(B, n, h, DP, dtype=torch.float32, device=t.device)
            out[..., :D] = t.permute(0, 2, 1, 3)
            return out.reshape(B * n, h, DP)
        Q, K, V = tile(q), tile(k), tile(v)
        O, den, states = H.causal_attn_fwd(Q, K, V, keep, B, n, h, DP, eps)
        _save_named(ctx, Q=Q, K=K, V=V, O=O, keep=keep, den=den, states=states)
        ctx.dims, ctx.eps = (B, h, n, D, DP), eps
        return O.reshape(B, n, h, DP)[..., :D].permute(0, 2, 1, 3).contiguous()

    @staticmethod
    def backward(ctx, gy):
        B, h, n, D, DP = ctx.dims
        s = _saved(ctx)
        dO = torch.zeros(B, n, h, DP, dtype=torch.float32, device=gy.device)
        dO[..., :D] = gy.permute(0, 2, 1, 3)
        dQ, dK, dV = H.causal_attn_bwd(dO.reshape(B * n, h, DP), s.O, s.Q, s.K, s.V, s.keep, s.den, s.states, B, n, h, DP, D,
                                       ctx.eps)
        dq, dk, dv = (t.reshape(B, n, h, DP)[..., :D].permute(0, 2, 1, 3).contiguous() for t in (dQ, dK, dV))
        return dq, dk, dv, None, None


def check_kv_mask(kv_mask, B: int, n: int):
    """The key / value mask of the causal kind: None or a torch.bool tensor [B, n], True = keep.  Returns the keep vector
    (uint8 view) or None; TypeError / AssertionError before anything is launched."""
    if kv_mask is None:
        return None
    if not (isinstance(kv_mask, torch.Tensor) and kv_mask.dtype == torch.bool):
        raise TypeError("causal attention: the mask is a torch.bool tensor [B, n_kv] (True = keep), got "
                        f"{getattr(kv_mask, 'dtype', type(kv_mask).__name__)}")
    assert tuple(kv_mask.shape) == (B, n), f"causal attention: the mask is [B, n_kv] = {(B, n)}, got {tuple(kv_mask.shape)}"
    return kv_mask.contiguous().view(torch.uint8)


def causal_linear_attention(q, k, v, kv_mask=None, eps: float = 1e-7):
    """The reference's causal_linear_attn on q, k, v [B, h, n, D] (k is not modified): with k^_j = keep_j k_j / n and
    v^_j = keep_j v_j,  out_i = (sum_{j<=i} k^_j v^_j^T)^T q_i / ((sum_{j<=i} k^_j + eps) . q_i).  ``kv_mask``: torch.bool
    [B, n], True = keep, or None.  Linear in n (gt_causal_attn_*), differentiable in q, k, v.  No dropout is drawn on the
    running state, which is never formed; returns (out, None).  The operator is only as well-conditioned as its
    denominators: with sign-indefinite q, k they cancel and fp32 (here as in torch) loses accuracy accordingly.
    round4(D) outside H.CAUSAL_DP raises GtNotSupported before anything is launched."""
    assert q.dim() == 4 and q.shape == k.shape == v.shape, "causal_linear_attention: q, k, v are [B, h, n, D] alike"
    B, h, n, D = q.shape
    H.causal_check(H.round4(D))
    keep = check_kv_mask(kv_mask, B, n)
    return CausalLinearAttnFn.apply(q, k, v, keep, float(eps)), None
