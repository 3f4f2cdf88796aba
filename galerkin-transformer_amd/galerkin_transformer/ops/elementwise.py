"""Elementwise operators: stateless-RNG dropout, the fused dropout / activation tails, row LayerNorm.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from .. import _hip as H


_next_salt = H.next_salt        # call-site salt counter (rewound by _hip.set_seed / utils.get_seed)


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------- elementwise dropout
class DropoutFn(Function):
    """Stateless-RNG dropout (gt_dropout_apply): one device-resident seed drives every mask of a
    training step, so a captured HIP graph replays with fresh masks and backward regenerates the
    forward mask from (seed, salt) instead of storing it."""

    @staticmethod
    def forward(ctx, x, p: float):
        xc = _c(x)
        ctx.cfg = (p, _next_salt(1))
        return H.dropout_apply(xc, H.dropout_desc(p, ctx.cfg[1], x.device))

    @staticmethod
    def backward(ctx, g):
        p, salt = ctx.cfg
        return H.dropout_apply(_c(g), H.dropout_desc(p, salt, g.device)), None


def dropout(x, p: float, training: bool = True):
    """Drop-in for nn.Dropout.forward on device tensors."""
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, float(p))


class DropActFn(Function):
    """y = act2(drop2(act1(drop1(x)))) in one elementwise pass; backward recomputes from x (gt_dropact_*)."""

    @staticmethod
    def forward(ctx, x, p1: float, act1: int, p2: float, act2: int):
        xc = _c(x)
        ctx.cfg = (p1, _next_salt(1) if p1 > 0 else 0, act1, p2, _next_salt(1) if p2 > 0 else 0, act2)
        ctx.save_for_backward(xc)
        dev = x.device
        return H.dropact_fwd(xc, H.dropout_desc(p1, ctx.cfg[1], dev), act1, H.dropout_desc(p2, ctx.cfg[4], dev), act2)

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        p1, s1, act1, p2, s2, act2 = ctx.cfg
        dev = g.device
        gx = H.dropact_bwd(xc, _c(g), H.dropout_desc(p1, s1, dev), act1, H.dropout_desc(p2, s2, dev), act2)
        return gx, None, None, None, None


def drop_act(x, p1: float, act1: str, training: bool = True, p2: float = 0.0, act2: str = "none"):
    """act2(dropout(act1(dropout(x, p1)), p2)) -- the dropout -> activation tails of the conv blocks, fused."""
    if not training:
        p1 = p2 = 0.0
    return DropActFn.apply(x, float(p1), H.ACT_CODE[act1], float(p2), H.ACT_CODE[act2])


# ----------------------------------------------------------------------------------- row LayerNorm
class LayerNormFn(Function):
    """nn.LayerNorm(d_model) of the encoder layer (model.py:84-85, 128-135)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float):
        xc = _c(x)
        y, stats = H.layernorm_fwd(xc, _c(weight), _c(bias), eps)
        ctx.save_for_backward(xc, weight, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, weight, stats = ctx.saved_tensors
        dx, dg, db = H.layernorm_bwd(_c(gy), xc, _c(weight), stats)
        return dx, dg, db, None


def layer_norm(x, weight, bias, eps):
    return LayerNormFn.apply(x, weight, bias, float(eps))
