"""The training objectives: per-sample relative L2 error and H1-seminorm regulariser of ``ft.WeightedL2Loss2d`` (reference:
libs/ft.py:983-1105) and of the 1-D ``ft.WeightedL2Loss`` (libs/ft.py:898-980), each as one streaming forward pass, a merge
of its partial sums and one gather backward.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _hip as H
from .elementwise import _c


class H1Loss2dFn(Function):
    """(loss [N], reg [N] or None, L2 [N], H1 [N]) from the prediction P [N, n, n], the target T, the target gradient G
    [N, n, n, 2] (or None) and the coefficient K of N n n elements (or None).  P is read in place when its pixels are evenly
    pitched (channel 0 of the model's [N, n, n, c] output); only P gets a gradient, and the norms carry none."""

    @staticmethod
    def forward(ctx, P, T, G, K, dilation: int, h: float, beta: float, gamma: float, eps: float, want_reg: bool):
        P = P if H.h1loss2d_pitch(P) is not None else P.contiguous()
        T, G, K = _c(T), (None if G is None else _c(G)), (None if K is None else _c(K))
        loss, reg, L2, H1 = H.h1loss2d_fwd(P, T, G, K, dilation, h, beta, gamma, eps, want_reg)
        ctx.cfg = (dilation, h, beta, gamma)
        ctx.has = (G is not None, K is not None)
        ctx.save_for_backward(P, T, L2, H1, *(t for t in (G, K) if t is not None))
        ctx.mark_non_differentiable(L2, H1)
        ctx.set_materialize_grads(False)
        return loss, reg, L2, H1

    @staticmethod
    @once_differentiable
    def backward(ctx, gl, gr, _gl2, _gh1):
        P, T, L2, H1, *rest = ctx.saved_tensors
        G = rest.pop(0) if ctx.has[0] else None
        K = rest.pop(0) if ctx.has[1] else None
        if gl is None and gr is None:
            return (None,) * 10
        dilation, h, beta, gamma = ctx.cfg
        gl, gr = (None if gl is None else _c(gl)), (None if gr is None else _c(gr))
        return (H.h1loss2d_bwd(P, T, G, K, L2, H1, gl, gr, dilation, h, beta, gamma),) + (None,) * 9


def weighted_l2_terms_2d(preds, targets, targets_prime=None, K=None, *, dilation=2, h, beta=1.0, gamma=0.1, eps=1e-10,
                         regularizer=False):
    """Per-sample terms of WeightedL2Loss2d on device tensors: (loss [N], reg [N] or None, L2 [N], H1 [N]).  ``reg`` is
    formed when ``regularizer`` and ``targets_prime`` is given; without ``targets_prime`` H1 is 1."""
    want_reg = bool(regularizer) and targets_prime is not None
    return H1Loss2dFn.apply(preds, targets, targets_prime, K, int(dilation), float(h), float(beta), float(gamma), float(eps),
                            want_reg)


class H1Loss1dFn(Function):
    """(loss [N], reg [N] or None, L2 [N], H1 [N]) from the prediction P [N, L], the target T and the target derivative G
    [N, L] (or None).  P is read in place when its elements are evenly pitched (channel 0 of the model's [N, L, c] output);
    only P gets a gradient, and the norms carry none."""

    @staticmethod
    def forward(ctx, P, T, G, dilation: int, h: float, beta: float, gamma_h: float, want_reg: bool):
        P = P if H.h1loss1d_pitch(P) is not None else P.contiguous()
        T, G = _c(T), (None if G is None else _c(G))
        loss, reg, L2, H1 = H.h1loss1d_fwd(P, T, G, dilation, h, beta, gamma_h, want_reg)
        ctx.cfg = (dilation, h, beta, gamma_h)
        ctx.has_g = G is not None
        ctx.save_for_backward(P, T, L2, H1, *(() if G is None else (G,)))
        ctx.mark_non_differentiable(L2, H1)
        ctx.set_materialize_grads(False)
        return loss, reg, L2, H1

    @staticmethod
    @once_differentiable
    def backward(ctx, gl, gr, _gl2, _gh1):
        P, T, L2, H1, *rest = ctx.saved_tensors
        G = rest[0] if ctx.has_g else None
        if gl is None and gr is None:
            return (None,) * 8
        dilation, h, beta, gamma_h = ctx.cfg
        gl, gr = (None if gl is None else _c(gl)), (None if gr is None else _c(gr))
        return (H.h1loss1d_bwd(P, T, G, L2, H1, gl, gr, dilation, h, beta, gamma_h),) + (None,) * 7


def weighted_l2_terms_1d(preds, targets, targets_prime=None, *, dilation=2, h, beta=1.0, gamma_h=0.0, regularizer=False):
    """Per-sample terms of WeightedL2Loss on device tensors: (loss [N], reg [N] or None, L2 [N], H1 [N]).  ``gamma_h`` is the
    regulariser's weight times h, as the class stores it; ``reg`` is formed when ``regularizer``, ``gamma_h > 0`` and
    ``targets_prime`` is given; without ``targets_prime`` H1 is 1."""
    want_reg = bool(regularizer) and gamma_h > 0 and targets_prime is not None
    return H1Loss1dFn.apply(preds, targets, targets_prime, int(dilation), float(h), float(beta), float(gamma_h), want_reg)
