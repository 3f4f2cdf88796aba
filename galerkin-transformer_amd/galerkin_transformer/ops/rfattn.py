"""Random-feature attention (Performer 'favor' / random Fourier features 'rfa') as one autograd node on gt_rfattn.hip.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from .. import _hip as H
from .dense import _check_res_is_x
from .elementwise import _c, _next_salt


class RandomFeatureAttentionFn(Function):
    """y = res + dropout1( [att, pos] Wout^T + bout ),  att = phi(Q) (phi(K)^T V) / (phi(Q) . sum_tokens phi(K) + eps)
    with one head of width d, q, k, v = the three column blocks of x Wqkv^T + bqkv and phi the feature map of ``kind`` over
    ``omega`` [d, d/2] (examples/ex1_burgers_random_fourier_features.py:272-318 of the reference).

    Five steps.  forward: the packed QKV projection (gt_gemm, [T, 3d]); gt_rfattn_kv -> KVa; gt_rfattn_q -> att, den; the
    output projection with the coordinate columns as its rank-p epilogue (the LAST pos_dim columns of Wout, as in
    ops.linear's ``extra``), the residual and drop1.  backward: the output projection's three gradients; gt_rfattn_bwd_q and
    gt_rfattn_bwd_kv, which recompute phi and write dQ, dK, dV into the column blocks of one d_qkv [T, 3d]; the projection's
    weight and data gradients.  Saved: x, the weights, omega, qkv, att, den, KVa -- phi(Q), phi(K) and u ([B, n, d] each) exist
    in registers only.  Gradients: x, wqkv, bqkv, wout, bout; none for omega and pos."""

    @staticmethod
    def forward(ctx, x, pos, wqkv, bqkv, omega, wout, bout, res, cfg):
        kind, eps, p_out = cfg
        H.need_f32_cuda(x, pos, wqkv, bqkv, omega, wout, bout, res)
        B, n, d = x.shape
        p = pos.shape[-1]
        T, dev = B * n, x.device
        xc, posc = _c(x).reshape(T, d), _c(pos).reshape(T, p)
        wq, wo, om = _c(wqkv), _c(wout), _c(omega)
        salt = _next_salt()
        qkv = torch.empty(T, 3 * d, dtype=torch.float32, device=dev)
        H.gemm(xc, wq, qkv, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=bqkv, weight_b=True)
        Q, K, V = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        KVa = H.rfattn_kv(K, V, 3 * d, om, B, n, d, kind)
        att, den = H.rfattn_q(Q, 3 * d, om, KVa, B, n, d, kind, eps)
        y = torch.empty(T, d, dtype=torch.float32, device=dev)
        rc = None if res is None else _c(res).reshape(T, d)
        drop = H.dropout_desc(p_out, salt, dev) if p_out > 0 else None
        H.gemm(att, wo, y, T, d, d, lda=d, ldb=d + p, ldc=d, bias=bout, rp=p, rp_a=posc, rp_lda=p, rp_b=wo[:, d:],
               rp_ldb=d + p, drop=drop, res=rc, ldr=d)
        ctx.save_for_backward(xc, posc, wq, wo, om, qkv, att, den, KVa)
        ctx.cfg = (kind, p_out, salt, (B, n, d, p), bqkv is not None, bout is not None, res is not None, x.shape)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, gy):
        xc, posc, wq, wo, om, qkv, att, den, KVa = ctx.saved_tensors
        kind, p_out, salt, (B, n, d, p), hbq, hbo, has_res, xshape = ctx.cfg
        T, dev = B * n, gy.device
        f32 = dict(dtype=torch.float32, device=dev)
        g_in = _c(gy).reshape(T, d)                         # unmasked: what flows to the residual branch
        g = H.dropout_apply(g_in, H.dropout_desc(p_out, salt, dev)) if p_out > 0 else g_in
        dwo = torch.empty(d, d + p, **f32)
        dbo = torch.empty(d, **f32) if hbo else None
        with H.side_branch(dev, T):     # the weight gradients next to the data gradient
            H.gemm(g, att, dwo, d, d, T, layout_a=1, layout_b=1, lda=d, ldb=d, ldc=d + p, split_k=0, a_colsum=dbo)
            H.gemm(g, posc, dwo[:, d:], d, p, T, layout_a=1, layout_b=1, lda=d, ldb=p, ldc=d + p, split_k=0)
        datt = torch.empty(T, d, **f32)
        H.gemm(g, wo, datt, T, d, d, layout_b=1, lda=d, ldb=d + p, ldc=d)
        H.join_side(dev)
        dqkv = torch.empty(T, 3 * d, **f32)
        Q, K, V = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        H.rfattn_bwd(Q, K, V, 3 * d, om, KVa, datt, att, den, dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:], 3 * d, B, n, d,
                     kind)
        dwq = torch.empty(3 * d, d, **f32)
        dbq = torch.empty(3 * d, **f32) if hbq else None
        with H.side_branch(dev, T):
            H.gemm(dqkv, xc, dwq, 3 * d, d, T, layout_a=1, layout_b=1, lda=3 * d, ldb=d, ldc=d, split_k=0, a_colsum=dbq)
        dx = torch.empty(T, d, **f32)
        # (res is x: its gradient, the unmasked g_in, is folded into dx and the `res` slot returns None)
        H.gemm(dqkv, wq, dx, T, d, 3 * d, layout_b=1, lda=3 * d, ldb=d, ldc=d, res=g_in if has_res else None, ldr=d,
               weight_b=True)
        H.join_side(dev)
        return dx.reshape(xshape), None, dwq, dbq, None, dwo, dbo, None, None


def random_feature_attention(x, pos, wqkv, bqkv, omega, wout, bout, *, kind: str, eps: float = 1e-6, res=None,
                             p_out: float = 0.0):
    """Random-feature self-attention block over x [B, n, d] with ONE head: ``wqkv`` [3d, d] / ``bqkv`` [3d] the packed query,
    key, value projections, ``omega`` [d, d/2] the random projection (no gradient), ``wout`` [d, d + pos_dim] the output
    projection over [attention, pos] (coordinates LAST), ``kind`` 'rfa' or 'favor'.  ``res`` must be ``x`` (or None);
    ``p_out`` is the dropout on the projected output, in front of the residual.  d in (32, 64, 96), else
    NotImplementedError before anything is launched; ``pos`` is required (the reference concatenates it unconditionally)."""
    if pos is None:
        raise ValueError("random_feature_attention: `pos` is required (the coordinates are concatenated in front of the "
                         "output projection unconditionally)")
    if x.dim() != 3 or pos.dim() != 3 or pos.shape[:2] != x.shape[:2]:
        raise ValueError(f"random_feature_attention: x is [B, n, d] and pos [B, n, pos_dim] (got {tuple(x.shape)}, "
                         f"{tuple(pos.shape)})")
    d, p = x.shape[-1], pos.shape[-1]
    H.rfattn_check(d, kind)
    if tuple(wqkv.shape) != (3 * d, d) or tuple(omega.shape) != (d, d // 2) or tuple(wout.shape) != (d, d + p):
        raise ValueError(f"random_feature_attention: wqkv is [3d, d], omega [d, d/2], wout [d, d + pos_dim] (got "
                         f"{tuple(wqkv.shape)}, {tuple(omega.shape)}, {tuple(wout.shape)})")
    if pos.requires_grad or omega.requires_grad:
        raise NotImplementedError("random_feature_attention: `pos` and `omega` get no gradient")
    _check_res_is_x(res, x, "random_feature_attention")
    return RandomFeatureAttentionFn.apply(x, pos, wqkv, bqkv, omega, wout, bout, res, (kind, float(eps), float(p_out)))
