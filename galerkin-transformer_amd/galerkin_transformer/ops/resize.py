"""Bilinear resizes of the scalers: plain, from the three-segment buffer of the convolution chain, and with the
regressor's first Linear commuted in front.
"""
from __future__ import annotations

import math

import torch
from torch.autograd import Function

from .. import _hip as H
from .elementwise import _c


# ----------------------------------------------------------------------------------- bilinear resize
def out_size(hi: int, wi: int, size):
    """(Ho, Wo) of a resize of an hi x wi image.  ``size``: a pair of ints (tuple or list), taken as it is, or a float
    scale factor with the reference's recompute_scale_factor=True rule: output = floor(input * scale), and the
    align_corners scale is then recomputed from the two sizes."""
    if isinstance(size, float):
        return int(math.floor(hi * size)), int(math.floor(wi * size))
    if isinstance(size, (tuple, list)) and isinstance(size[0], float):
        raise NotImplementedError("per-axis scale factors")
    return int(size[0]), int(size[1])


class ResizeFn(Function):
    """act(F.interpolate(x, size, mode='bilinear', align_corners=True)) with the layout change of the
    scaler boundaries fused in (layers.py:483-512, 658-670; model.py:675-687, 740-749)."""

    @staticmethod
    def forward(ctx, x, size, in_nhwc: bool, out_nhwc: bool, act: int):
        xc = _c(x)
        y = H.bilinear2d_fwd(xc, size, in_nhwc, out_nhwc, act)
        in_size = (xc.shape[1], xc.shape[2]) if in_nhwc else (xc.shape[2], xc.shape[3])
        ctx.cfg = (in_size, in_nhwc, out_nhwc, act)
        if act == H.ACT_RELU:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        in_size, in_nhwc, out_nhwc, act = ctx.cfg
        y = ctx.saved_tensors[0] if act == H.ACT_RELU else None
        return H.bilinear2d_bwd(_c(g), y, in_size, in_nhwc, out_nhwc, act), None, None, None, None


def bilinear_resize(x, size, in_nhwc: bool = False, out_nhwc: bool = False, act: str = None):
    """``size``: (Ho, Wo), or a float scale factor with the reference's recompute_scale_factor=True rule
    (output = floor(input * scale), then the align_corners scale is recomputed from the sizes)."""
    hi, wi = (x.shape[1], x.shape[2]) if in_nhwc else (x.shape[2], x.shape[3])
    return ResizeFn.apply(x, out_size(hi, wi, size), bool(in_nhwc), bool(out_nhwc), H.ACT_CODE[act])


class ResizeSegFn(Function):
    """act(F.interpolate(cat[x1, x2, x3], size, bilinear, align_corners=True)) on the padded three-segment buffer of
    scaler_conv_chain: (B, Hi, Wi, 3 segp) -> dense channels-last (B, Ho, Wo, C) (layers.py:508-512)."""

    @staticmethod
    def forward(ctx, x, Cc: int, size, seg: int, segp: int, act: int, relu_input: bool, in_factor=None):
        xc = _c(x)
        dact = None
        if act == H.ACT_SILU:                    # + silu'(resized value), the factor of the backward
            y, dact = H.bilinear2d_seg_fwd(xc, Cc, size, seg, segp, act, want_dact=True)
        else:
            y = H.bilinear2d_seg_fwd(xc, Cc, size, seg, segp, act)
        ctx.cfg = ((xc.shape[1], xc.shape[2]), seg, segp, act, relu_input)
        ctx.save_for_backward(y if act == H.ACT_RELU else dact, xc if relu_input else None, in_factor)
        return y

    @staticmethod
    def backward(ctx, g):
        in_size, seg, segp, act, relu_input = ctx.cfg
        y, xin, fac = ctx.saved_tensors
        dx = H.bilinear2d_seg_bwd(_c(g), y, in_size, seg, segp, act, x_gate=fac if fac is not None else xin,
                                  gate_mul=fac is not None)
        return dx, None, None, None, None, None, None, None


def bilinear_resize_seg(x, n_channels: int, size, seg: int, segp: int, act: str = None, relu_input: bool = False,
                        in_factor=None):
    """relu_input: x is the output of a ReLU (scaler_conv_chain's buffer) -- the gradient returned for x is already zeroed
    where x <= 0, which is what its producer's backward would do first (ScalerConvChainFn(grad_masked=True) skips it).
    in_factor: the same for any other activation -- a buffer shaped like x (scaler_conv_chain's second output: dropout
    scale x activation derivative) that the returned gradient is multiplied with."""
    size = out_size(x.shape[1], x.shape[2], size)
    if relu_input and in_factor is not None:
        raise ValueError("bilinear_resize_seg: relu_input and in_factor are alternatives")
    return ResizeSegFn.apply(x, int(n_channels), size, int(seg), int(segp), H.ACT_CODE[act],
                             bool(relu_input), in_factor)


class UpsampleFcFn(Function):
    """fc(cat[upsample(x), grid]) without ever materialising upsample(x).

    Reference: Interp2dUpsample's final F.interpolate (layers.py:658-670) followed by SpectralRegressor /
    PointwiseRegressor ``fc(torch.cat([x, grid], -1))`` (model.py:615-617, 507-512).  A pointwise Linear
    commutes with bilinear interpolation (the four weights sum to one), so

        fc(cat[up(x), grid]) = up(x W_x^T) + grid W_g^T + b

    x: (B, K, Hi, Wi) channels-first, or (B, Hi, Wi, K) with ``x_nhwc`` (what the scaler's conv block produces on
    its NCHW / implicit-GEMM path); weight (N, K+p); grid (B, Ho, Wo, p).  Returns (B, Ho, Wo, N).  Only valid when
    nothing (dropout) sits between the resize and the Linear -- the caller checks."""

    @staticmethod
    def forward(ctx, x, size, weight, bias, grid, x_nhwc, in_factor=None):
        H.need_f32_cuda(x, weight, bias, grid, in_factor)
        if in_factor is not None and not x_nhwc:
            raise NotImplementedError("ops.upsample_fc: in_factor needs channels-last features")
        if x_nhwc:
            B, Hi, Wi, K = x.shape
        else:
            B, K, Hi, Wi = x.shape
        N, p = weight.shape[0], grid.shape[-1]
        assert weight.shape[1] == K + p
        Ho, Wo = size
        xc, w, gc = _c(x), _c(weight), _c(grid)
        dev, HW = x.device, Hi * Wi
        z = torch.empty(B, Hi, Wi, N, dtype=torch.float32, device=dev)
        if x_nhwc:
            H.gemm(xc, w, z, B * HW, N, K, lda=K, ldb=K + p, ldc=N)
        else:
            H.gemm(xc, w, z, HW, N, K, layout_a=1, lda=HW, ldb=K + p, ldc=N, batch=(B, 1), a_bs=(K * HW, 0),
                   c_bs=(HW * N, 0))
        out = H.bilinear2d_fwd(z, (Ho, Wo), True, True, H.ACT_NONE, bias=bias, rp_a=gc.reshape(B, Ho, Wo, p),
                               rp_b=w[:, K:], rp_ldb=K + p)
        ctx.save_for_backward(xc, w, gc, None if in_factor is None else _c(in_factor))
        ctx.cfg = (B, K, Hi, Wi, Ho, Wo, N, p, bias is not None, x_nhwc)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, w, gc, fac = ctx.saved_tensors
        B, K, Hi, Wi, Ho, Wo, N, p, has_b, x_nhwc = ctx.cfg
        dev, HW, To = g.device, Hi * Wi, B * Ho * Wo
        gg = _c(g)
        f32 = dict(dtype=torch.float32, device=dev)
        dz = H.bilinear2d_bwd(gg, None, (Hi, Wi), True, True, H.ACT_NONE)              # (B, Hi, Wi, N)
        dw = torch.empty(N, K + p, **f32)
        db = torch.empty(N, **f32) if has_b else None
        # d W_g = g^T grid  (+ d bias = column sums of g as a by-product)
        H.gemm(gg, gc, dw[:, K:], N, p, To, layout_a=1, layout_b=1, lda=N, ldb=p, ldc=K + p, split_k=0,
               a_colsum=db)
        dx = None
        if x_nhwc:
            # d W_x^T [K, N] = x^T dz over all B*HW pixels: the tall-skinny reduction (gt_tsmm.hip)
            dwxt = torch.empty(K, N, **f32)
            H.gemm(xc, dz, dwxt, K, N, B * HW, layout_a=1, layout_b=1, lda=K, ldb=N, ldc=N, split_k=0)
            dw[:, :K].copy_(dwxt.t())
            if ctx.needs_input_grad[0]:
                dx = torch.empty(B, Hi, Wi, K, **f32)
                if fac is None:
                    H.gemm(dz, w, dx, B * HW, K, N, layout_b=1, lda=N, ldb=K + p, ldc=K)
                else:       # in_factor: the producer's activation derivative rides on this product's epilogue
                    H.gemm(dz, w, dx, B * HW, K, N, layout_b=1, lda=N, ldb=K + p, ldc=K, aux_op=H.AUX_MUL,
                           aux=fac.reshape(B * HW, K), ldaux=K)
            return dx, None, dw, db, None, None, None
        # d W_x = sum_b dz_b^T x_b^T : one [N, K] slab per batch entry, reduced in a fixed order
        slabs = torch.empty(B, N, K, **f32)
        H.gemm(dz, xc, slabs, N, K, HW, layout_a=1, layout_b=0, lda=N, ldb=HW, ldc=K, batch=(B, 1),
               a_bs=(HW * N, 0), b_bs=(K * HW, 0), c_bs=(N * K, 0), split_k=0)
        dwx = torch.empty(N, K, **f32)
        H.slab_reduce(slabs, B, N * K, N * K, dwx)
        dw[:, :K].copy_(dwx)
        if ctx.needs_input_grad[0]:
            # dx_b [K, HW] = W_x^T dz_b^T
            dx = torch.empty(B, K, Hi, Wi, **f32)
            H.gemm(w, dz, dx, K, HW, N, layout_a=1, layout_b=0, lda=K + p, ldb=N, ldc=HW, batch=(B, 1),
                   b_bs=(HW * N, 0), c_bs=(K * HW, 0))
        return dx, None, dw, db, None, None, None


def upsample_fc(x, size, weight, bias, grid, x_nhwc: bool = False, in_factor=None):
    """in_factor (same shape as x, channels-last only): x is the output of conv3x3_nhwc(act2=True), whose backward expects
    the gradient already multiplied by this factor -- the data-gradient product here does it on its epilogue."""
    if grid.requires_grad:
        raise NotImplementedError("ops.upsample_fc: `grid` gets no gradient")
    return UpsampleFcFn.apply(x, (int(size[0]), int(size[1])), weight, bias, grid, bool(x_nhwc), in_factor)
