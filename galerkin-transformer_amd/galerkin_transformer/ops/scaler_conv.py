"""Operators of the 'conv' scaler modes: the 2x2 average pool with its activation (Conv2dEncoder) and the 3x3 / stride-2
transposed convolution with bias, dropout and activation (DeConv2dBlock).
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from .. import _hip as H
from .conv import _gathered
from .elementwise import _c, _next_salt


# ----------------------------------------------------------------------------------- average pool + activation
class AvgPool2ActFn(Function):
    """act(F.avg_pool2d(x, 2)) with the layout change of the scaler boundary fused in (layers.py:329-341).  The backward
    recomputes the pooled value from x (gt_avgpool2_act_bwd); nothing but x is kept."""

    @staticmethod
    def forward(ctx, x, act: int, in_nhwc: bool, out_nhwc: bool):
        xc = _c(x)
        ctx.cfg = (act, in_nhwc, out_nhwc)
        ctx.save_for_backward(xc)
        return H.avgpool2_act_fwd(xc, in_nhwc, out_nhwc, act)

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        act, in_nhwc, out_nhwc = ctx.cfg
        return H.avgpool2_act_bwd(xc, _c(g), in_nhwc, out_nhwc, act), None, None, None


def avgpool2_act(x, act: str = None, in_nhwc: bool = False, out_nhwc: bool = False):
    """x (B, C, H, W), or (B, H, W, C) with ``in_nhwc`` -> act(avg_pool2d(x, 2)) as (B, C, H//2, W//2), or channels-last with
    ``out_nhwc``.  The pool floors: an odd trailing row / column is dropped and gets a zero gradient.  act: None / 'none',
    'relu' or 'silu'."""
    H.need_f32_cuda(x)
    if act not in (None, "none", "relu", "silu"):
        raise NotImplementedError(f"avgpool2_act: activation {act!r}")
    if x.ndim != 4:
        raise ValueError(f"avgpool2_act: a 4-D image is needed, got {tuple(x.shape)}")
    hi, wi = (x.shape[1], x.shape[2]) if in_nhwc else (x.shape[2], x.shape[3])
    if hi < 2 or wi < 2 or x.shape[0] < 1 or x.numel() == 0:
        raise ValueError(f"avgpool2_act: the pooled map of a {hi} x {wi} image is empty")
    return AvgPool2ActFn.apply(x, H.ACT_CODE[act], bool(in_nhwc), bool(out_nhwc))


# ----------------------------------------------------------------------------------- transposed 3x3 / stride-2 convolution
def deconv_out_size(h: int, w: int, padding: int, output_padding: int):
    """(Ho, Wo) of nn.ConvTranspose2d(kernel_size=3, stride=2, padding, output_padding) on an h x w image:
    2 (h - 1) - 2 padding + 3 + output_padding.  ValueError where torch refuses the call too."""
    h, w, padding, output_padding = int(h), int(w), int(padding), int(output_padding)
    if h < 1 or w < 1 or padding < 0 or output_padding not in (0, 1):      # (output_padding must be smaller than the stride)
        raise ValueError(f"deconv_out_size: bad arguments h={h} w={w} padding={padding} output_padding={output_padding}")
    ho, wo = (2 * (n - 1) - 2 * padding + 3 + output_padding for n in (h, w))
    if ho < 1 or wo < 1:
        raise ValueError(f"deconv_out_size: a {h} x {w} image with padding={padding}, output_padding={output_padding} has "
                         f"the output size {ho} x {wo}")
    return ho, wo


def _deconv_filter(weight):
    """[Cin, Cout, 3, 3] -> [9 Cout, Cin], row (ky*3 + kx)*Cout + co: the B operand of the forward product (layout_b = 0) and,
    read the other way (layout_b = 1), of the data gradient.  One index_select (_gathered)."""
    cin, cout = weight.shape[:2]
    return _gathered(weight, ("deconv",), lambda t: t.permute(2, 3, 1, 0).reshape(9 * cout, cin))


class ConvTranspose3x3S2Fn(Function):
    """act(dropout(conv_transpose2d(x, weight, bias, stride=2, padding, output_padding))) on channels-last images
    (DeConv2dBlock, layers.py:552-559).  Forward: cols [B H W, 9 Cout] = x W as one gt_gemm product, then the gather kernel
    (gt_deconv3x3s2_gather_fwd) with bias, dropout mask and activation where y is stored.  Backward: the gated gradient
    gathered into dcols (gt_deconv3x3s2_gather_bwd: act' and the re-drawn mask are applied there), dx = dcols W^T next to
    dW = x^T dcols on the side branch, db from gt_deconv3x3s2_dbias.  Kept for the backward: x, the weight and, for SiLU,
    the sum in front of the dropout (ReLU reads y itself, no activation nothing)."""

    @staticmethod
    def forward(ctx, x, weight, bias, padding: int, output_padding: int, out_hw, p_drop: float, act: int):
        B, Hh, Ww, Cin = x.shape
        Cout = weight.shape[1]
        T = B * Hh * Ww
        xc = _c(x)
        wt = _deconv_filter(weight)
        ctx.prec = H.get_precision()             # the backward products run in the arithmetic of the forward
        cols = torch.empty(T, 9 * Cout, dtype=torch.float32, device=x.device)
        H.gemm(xc, wt, cols, T, 9 * Cout, Cin, lda=Cin, ldb=Cin, ldc=9 * Cout, precision=ctx.prec)
        salt = _next_salt(1) if p_drop > 0 else 0
        drop = H.dropout_desc(p_drop, salt, x.device) if p_drop > 0 else None
        need = any(ctx.needs_input_grad[:3])     # (grad mode itself is off inside Function.forward)
        y, pre = H.deconv3x3s2_gather_fwd(cols, None if bias is None else _c(bias), B, Hh, Ww, Cout, padding, output_padding,
                                          out_hw, drop, act, want_pre=need and act == H.ACT_SILU)
        gate = pre if act == H.ACT_SILU else (y if act == H.ACT_RELU else None)
        ctx.save_for_backward(xc, weight, gate if need else None)
        ctx.cfg = (padding, output_padding, p_drop, salt, act, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, weight, gate = ctx.saved_tensors
        padding, output_padding, p_drop, salt, act, has_bias = ctx.cfg
        B, Hh, Ww, Cin = xc.shape
        Cout = weight.shape[1]
        T = B * Hh * Ww
        dev = g.device
        gc = _c(g)
        drop = H.dropout_desc(p_drop, salt, dev) if p_drop > 0 else None
        geo = (B, Hh, Ww, Cout, padding, output_padding)
        dx = dw = db = None
        if has_bias and ctx.needs_input_grad[2]:
            db = H.deconv3x3s2_dbias(gc, gate, *geo, drop, act)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dcols = H.deconv3x3s2_gather_bwd(gc, gate, *geo, drop, act)
            if ctx.needs_input_grad[0]:
                wt = _deconv_filter(weight)
                dx = torch.empty(B, Hh, Ww, Cin, dtype=torch.float32, device=dev)
                # K = 9 Cout is long and a small image has few row tiles: below the packed-B kernels' row count the library
                # may cut K (128 channels: 81 -> 18 / 24 / 36 us at 576 / 1764 / 6724 pixels; 62 -> 82 us at 22 500)
                with H.side_branch(dev, T):      # the data gradient next to the weight gradient below
                    H.gemm(dcols, wt, dx, T, Cin, 9 * Cout, layout_b=1, lda=9 * Cout, ldb=Cin, ldc=Cin,
                           split_k=0 if T < 16384 else 1, precision=ctx.prec)
            if ctx.needs_input_grad[1]:
                # dWt[(tap, co)][ci] = sum_pix dcols[pix][(tap, co)] x[pix][ci]
                dwt = torch.empty(9 * Cout, Cin, dtype=torch.float32, device=dev)
                H.gemm(dcols, xc, dwt, 9 * Cout, Cin, T, layout_a=1, layout_b=1, lda=9 * Cout, ldb=Cin, ldc=Cin, split_k=0,
                       precision=ctx.prec)
                dw = dwt.view(3, 3, Cout, Cin).permute(3, 2, 0, 1).contiguous()
            H.join_side(dev)
        return dx, dw, db, None, None, None, None, None


def conv_transpose3x3s2(x_nhwc, weight, bias=None, padding: int = 0, output_padding: int = 0, p_drop: float = 0.0,
                        act: str = None, training: bool = True):
    """x (B, H, W, Cin) channels-last, weight (Cin, Cout, 3, 3) and bias (Cout,) of an nn.ConvTranspose2d(kernel_size=3,
    stride=2) -> act(dropout(conv_transpose2d(x))) as (B, Ho, Wo, Cout), (Ho, Wo) = deconv_out_size(H, W, ...).  Channel
    counts that are no multiples of 4 raise NotImplementedError, sizes without an output ValueError -- both before anything is
    launched; there is no library fallback."""
    H.need_f32_cuda(x_nhwc, weight, bias)
    if act not in (None, "none", "relu", "silu"):
        raise NotImplementedError(f"conv_transpose3x3s2: activation {act!r}")
    if x_nhwc.ndim != 4 or weight.ndim != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] != x_nhwc.shape[3]:
        raise ValueError(f"conv_transpose3x3s2: x {tuple(x_nhwc.shape)} (B, H, W, Cin) does not go with the weight "
                         f"{tuple(weight.shape)} (Cin, Cout, 3, 3)")
    if bias is not None and tuple(bias.shape) != (weight.shape[1],):
        raise ValueError(f"conv_transpose3x3s2: bias {tuple(bias.shape)} for {weight.shape[1]} output channels")
    p = float(p_drop) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"conv_transpose3x3s2: p_drop={p_drop}")
    B, Hh, Ww, Cin = x_nhwc.shape
    if B < 1:
        raise ValueError("conv_transpose3x3s2: empty batch")
    out_hw = deconv_out_size(Hh, Ww, padding, output_padding)
    H.deconv3x3s2_check(B, Hh, Ww, Cin, weight.shape[1], int(padding), int(output_padding))
    return ConvTranspose3x3S2Fn.apply(x_nhwc, weight, bias, int(padding), int(output_padding), out_hw, p, H.ACT_CODE[act])
