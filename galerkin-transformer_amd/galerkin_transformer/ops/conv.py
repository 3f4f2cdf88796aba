"""3x3 convolutions of the scalers: conv0 fused with its resize, the wide channels-last convolution and the chain of
three narrow ones as implicit GEMMs, their filter layouts, weight-gradient routes and switches.
"""
from __future__ import annotations

import os

import torch
from torch.autograd import Function

from .. import _hip as H
from ._handoff import _scaler_mask_sink
from .elementwise import _c, _next_salt
from .resize import out_size


_crb_bits = [os.environ.get("GT_CRB_BITS", "1") != "0"]


class Conv3x3ResizeFn(Function):
    """act(resize(act(dropout(conv3x3(x))))) in one pass, act = ReLU or SiLU -- the head of Interp2dEncoder
    (layers.py:483-495) when the input carries few channels and needs no gradient.  See gt_conv3x3_resize_fwd."""

    @staticmethod
    def forward(ctx, x, weight, size, p_drop: float, out_nhwc: bool = False, act: int = H.ACT_RELU):
        xc, wc = _c(x), _c(weight)
        salt = _next_salt(1)                     # the salt the stand-alone dropout would have drawn
        drop = H.dropout_desc(p_drop, salt, x.device) if p_drop > 0 else None
        # channels-last ReLU: the forward records its four ReLU / dropout decisions per (output pixel, channel) (4 bits each,
        # 1/8 of y), and the backward takes them from there instead of re-evaluating the convolution (GT_CRB_BITS=0: off).
        # SiLU: the backward re-evaluates the convolution and both activations from x; nothing but x and w is kept.
        want = bool(out_nhwc and _crb_bits[0] and ctx.needs_input_grad[1] and act == H.ACT_RELU)   # (nothing to record for an inference pass)
        r = H.conv3x3_resize_fwd(xc, wc, size, drop, out_nhwc, want_bits=want, act=act)
        y, bits = r if want else (r, None)
        ctx.save_for_backward(xc, wc, y if act == H.ACT_RELU else None, bits)
        ctx.cfg = (p_drop, salt, out_nhwc, act)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, wc, y, bits = ctx.saved_tensors
        p_drop, salt, out_nhwc, act = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise RuntimeError("conv3x3_resize: the fused path has no input gradient")
        drop = H.dropout_desc(p_drop, salt, g.device) if p_drop > 0 else None
        return None, H.conv3x3_resize_bwd(_c(g), y, xc, wc, drop, out_nhwc, bits=bits, act=act), None, None, None, None


def conv3x3_resize(x, weight, size, p_drop: float = 0.0, training: bool = True, out_nhwc: bool = False, act: str = "relu"):
    """out_nhwc: return (B, Ho, Wo, Cout) channels-last (same values, same dropout mask).  act: 'relu' or 'silu' (both
    activations of the block: Interp2dEncoder builds them from one activation_type)."""
    size = out_size(x.shape[2], x.shape[3], size)
    if act not in ("relu", "silu"):
        raise NotImplementedError(f"conv3x3_resize: activation {act!r}")
    return Conv3x3ResizeFn.apply(x, weight, size, float(p_drop) if training else 0.0,
                                 bool(out_nhwc), H.ACT_CODE[act])


# ----------------------------------------------------------------------------------- 3x3 convolution, channels-last
def _plain_conv3x3(conv) -> bool:
    """True for a plain 3x3 / stride 1 / zero padding 1 / bias-free / ungrouped, undilated ``nn.Conv2d``: the one
    convolution the scaler kernels implement.  Channel counts, precision modes and switches are the callers'."""
    return (isinstance(conv, torch.nn.Conv2d) and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros")


def conv3x3_nhwc_ok(conv: torch.nn.Conv2d) -> bool:
    """True when ``conv`` is a scaler-block convolution the implicit-GEMM path covers: 3x3, stride 1, zero padding 1,
    no bias / groups / dilation, both channel counts multiples of 16 and >= 96 (whole tiles of the split-operand ring
    kernel in the forward AND the data-gradient product), and a split-operand arithmetic mode."""
    return (_plain_conv3x3(conv) and conv.in_channels % 16 == 0 and conv.out_channels % 16 == 0
            and conv.in_channels >= 96 and conv.out_channels >= 96 and H.get_precision() != "f32"
            and _conv_implicit[0])


_conv_implicit = [os.environ.get("GT_CONV_IMPLICIT", "1") != "0"]        # A/B switches (tools / tests)
# weight gradient of the implicit convolution: "hip" (default) = the nine-tap pixel contraction on the ring kernel,
# "miopen" = the library's channels-last wrw kernel on the same buffers.  Same box, back to back at B = 128 with the
# two-stream backward (tools/gpu_ab.sh): 33.31 / 33.46 vs 33.31 / 33.33 ms/step -- a tie; the library kernel is not
# the default because its solver choice is not ours: at B = 4 MIOpen has been seen to answer this layout with
# naive_conv_ab_nonpacked_wrw_nhwc (34 ms per call, profiles/README.md).
_conv_wgrad = [os.environ.get("GT_CONV_WGRAD", "hip") != "miopen"]
_conv_wgrad_planes = [os.environ.get("GT_CONV_WGRAD_PLANES", "1") != "0"]   # gt_conv3x3_wgrad_nhwc where it applies (A/B switch)
_scaler_wgrad_hip = [os.environ.get("GT_SCALER_WGRAD", "hip") != "miopen"]     # A/B switch (tools / tests)


_gather_cache = {}


def _gathered(w, key, fn):
    """fn(w) for a pure re-layout `fn` (flips, permutes, zero padding, reshapes) as ONE index_select (+ one multiply by a 0 / 1
    mask when fn pads): the index table is worked out once per (fn, shape) by running fn on the element numbers.  The filter
    re-layouts of the scaler convolutions run every step (the weights change every step): flip + permute + zeros + copy +
    contiguous per filter were 26 ATen launches per step (tools/aten_in_step.py), now 8."""
    k = (key, tuple(w.shape), str(w.device))
    ent = _gather_cache.get(k)
    if ent is None:
        src = torch.arange(1, w.numel() + 1, dtype=torch.float64).reshape(w.shape)
        r = fn(src)
        flat = r.reshape(-1)
        idx = (flat.to(torch.int64) - 1).clamp_min(0).to(w.device)
        mask = (flat > 0).to(torch.float32).to(w.device) if bool((flat == 0).any()) else None
        ent = (idx, mask, tuple(r.shape))
        _gather_cache[k] = ent
    idx, mask, shape = ent
    out = w.detach().reshape(-1).index_select(0, idx)
    if mask is not None:
        out = out * mask
    return out.view(shape)


def _conv_k_order(w):
    """[N, 9 taps, C] filter -> [N, 9 C] in the contraction order of the implicit-GEMM kernel (gt_hip.h: cv_*): channel
    blocks of CB outermost, the nine taps of a block adjacent."""
    N, _, Cc = w.shape
    cb = 32 if Cc % 32 == 0 else 16
    return w.reshape(N, 9, Cc // cb, cb).permute(0, 2, 1, 3).reshape(N, 9 * Cc).contiguous()


def _pad_filter(w, co_p, ci_p):
    """[co, ci, 3, 3] -> zero-padded [co_p, 9, ci_p] (tap-major) for _conv_k_order."""
    co, ci = w.shape[:2]
    out = torch.zeros(co_p, 9, ci_p, dtype=w.dtype, device=w.device)
    out[:co, :, :ci] = w.permute(0, 2, 3, 1).reshape(co, 9, ci)
    return out


def _filter_fwd(w, co_p, ci_p):
    """Forward filter of the implicit GEMM: [co, ci, 3, 3] -> [co_p, 9 ci_p] in k order, [co][tap][ci] zero-padded to
    (co_p, ci_p).  Without padding this is one index_select and no mask (_gathered)."""
    return _gathered(w, ("conv_fwd", co_p, ci_p), lambda t: _conv_k_order(_pad_filter(t, co_p, ci_p)))


def _filter_dgrad(w, ci_p, co_p):
    """Data-gradient filter: the taps reversed (tap' = 8 - tap has the opposite shift) and the channel roles swapped,
    [co, ci, 3, 3] -> [ci_p, 9 co_p] in k order."""
    return _gathered(w, ("conv_dgrad", ci_p, co_p),
                     lambda t: _conv_k_order(_pad_filter(t.flip(2, 3).transpose(0, 1), ci_p, co_p)))


def _library_conv_bwd(g, x, weight, wgrad: bool):
    """The library convolution where the HIP kernels answer GT_ENOTSUP (or a switch asks for it), on the channels-last
    buffers g (B, H, W, Cout) and x (B, H, W, Cin).  wgrad: the weight gradient [Cout, Cin, 3, 3] as the library's
    channels-last wrw kernel leaves it (``weight`` gives shape and memory format only); else the data gradient
    (B, H, W, Cin), dense."""
    gd, xd = g.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2)
    if wgrad:
        weight = weight.contiguous(memory_format=torch.channels_last)
    r = torch.ops.aten.convolution_backward(gd, xd, weight, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                            [not wgrad, wgrad, False])
    return r[1] if wgrad else r[0].permute(0, 2, 3, 1).contiguous()


def _conv3x3_wgrad(g, ldg, x, ldx, w, B, Hh, Ww, cin, cout, scale, prec, wide: bool):
    """dW[co][ci][tap] = scale * sum_pix g[pix][co] x[pix + shift(tap)][ci], returned as w's shape.  g / x: 2-D views
    [B*H*W, cout / cin] read in place through their row pitches ldg / ldx (cout, cin: the padded counts of the chain).
    Three routes, in this order:
    planes -- gt_conv3x3_wgrad_nhwc (gt_convw.hip): operands split once per block into LDS planes, all nine taps
              co-resident; images up to 80 wide, one side <= 48 channels wide;
    ring   -- ``wide`` (Conv3x3NhwcFn, dense operands) only: nine [cout, cin] products over the pixels, K chunks x taps on
              one launch + a fixed-order reduce (gt_hip.h: cv_wgrad), images at least 16 pixels wide;
    library-- the channels-last fp32 wrw kernel: on the same buffers (wide), or on dense copies of the two segments
              (chain; GT_SCALER_WGRAD=miopen is the round-3 path)."""
    co, ci = w.shape[:2]
    ring = wide and Ww >= 16 and _conv_wgrad[0]
    planes = (ring and prec in H.SPLIT_EXACT and _conv_wgrad_planes[0]) if wide else _scaler_wgrad_hip[0]
    if planes:
        try:
            dw = H.conv3x3_wgrad_nhwc(g, ldg, x, ldx, B, Hh, Ww, cin, cout, alpha=scale, precision=prec)
            return dw if wide else dw[:co, :ci].contiguous()
        except H.GtNotSupported:
            pass
    if ring:
        dw9 = torch.empty(9, cout, cin, dtype=torch.float32, device=g.device)
        try:
            H.gemm(g, x, dw9, cout, cin, B * Hh * Ww, layout_a=1, layout_b=1, lda=ldg, ldb=ldx, ldc=cin,
                   batch=(9, 1), c_bs=(cout * cin, 0), split_k=0, conv=(Hh, Ww, cin), conv_wgrad=True, precision=prec)
            return dw9.view(3, 3, cout, cin).permute(2, 3, 0, 1).contiguous()
        except H.GtNotSupported:
            pass
    gd = g.contiguous().view(B, Hh, Ww, cout)           # dense channels-last (the wide operands already are)
    xd = x.contiguous().view(B, Hh, Ww, cin)
    if wide:
        return _library_conv_bwd(gd, xd, w, True).contiguous()
    wp = torch.empty(cout, cin, 3, 3, dtype=torch.float32, device=w.device).contiguous(memory_format=torch.channels_last)
    return (_library_conv_bwd(gd, xd, wp, True)[:co, :ci] * scale).contiguous()


class Conv3x3NhwcFn(Function):
    """y = conv2d(x, weight, padding=1) on channels-last activations, as implicit GEMMs on the split-operand ring kernel.

    Replaces ``nn.Conv2d(C, C', 3, padding=1, bias=False)`` of the scaler blocks (layers.py:98-100 inside
    Interp2dUpsample, layers.py:624-670) where the channel counts fill the 128 x 128 tiles (the up-scaler's
    n_hidden -> n_hidden convolution).  Forward: [pixels, 9 C] x [C', 9 C]^T with the nine shifted views of x read in
    place (gt_hip.h: cv_*).  Data gradient: the same product on gy with the taps reversed and the channel roles
    swapped.  Weight gradient: nine pixel-contracted products, one per tap, cut into K chunks on one launch of the ring
    kernel (images at least 16 pixels wide); GT_CONV_WGRAD=miopen (and narrower images) use the library's channels-last
    wrw kernel on the same buffers instead -- the two tie at B = 128."""

    @staticmethod
    def forward(ctx, x, weight, act2: bool = False):
        H.need_f32_cuda(x, weight)
        B, Hh, Ww, Cin = x.shape
        Cout = weight.shape[0]
        xc = _c(x)
        wf = _filter_fwd(weight, Cout, Cin)      # [Cout][tap][Cin] -> k order
        y = torch.empty(B, Hh, Ww, Cout, dtype=torch.float32, device=x.device)
        ctx.prec = H.get_precision()             # the backward products run in the arithmetic of the forward
        ctx.save_for_backward(xc, weight)
        if not act2:
            H.gemm(xc, wf, y, B * Hh * Ww, Cout, 9 * Cin, lda=Cin, ldb=9 * Cin, ldc=Cout, conv=(Hh, Ww, Cin),
                   precision=ctx.prec)
            return y
        # act2: y = silu(silu(conv)) on the product's epilogue (GT_ACT_SILU2) + the factor silu' * silu'(silu), which the
        # CONSUMER's backward multiplies the gradient with (ops.upsample_fc(in_factor=fac)): what arrives here is then
        # already the gradient of the convolution's own output, and the backward below is the plain one
        need = any(ctx.needs_input_grad)         # (grad mode itself is off inside Function.forward)
        fac = torch.empty_like(y) if need else None
        H.gemm(xc, wf, y, B * Hh * Ww, Cout, 9 * Cin, lda=Cin, ldb=9 * Cin, ldc=Cout, conv=(Hh, Ww, Cin),
               act=H.ACT_SILU2, pre=fac, ldpre=Cout, precision=ctx.prec)
        if fac is None:
            fac = y.new_empty(0)
        ctx.mark_non_differentiable(fac)
        ctx.set_materialize_grads(False)         # (autograd filled a zero gradient the size of `fac` per step: 388 MB at C2)
        return y, fac

    @staticmethod
    def backward(ctx, gy, _gfac=None):
        if gy is None:
            return None, None, None
        xc, weight = ctx.saved_tensors
        B, Hh, Ww, Cin = xc.shape
        Cout = weight.shape[0]
        g = _c(gy)
        dx = dw = None
        dev = g.device
        if ctx.needs_input_grad[0]:
            # dx[pix][ci] = sum_tap sum_co gy[pix - shift(tap)][co] W[co][ci][tap]: tap' = 8 - tap has the opposite shift
            wd = _filter_dgrad(weight, Cin, Cout)        # [Cin][tap'][Cout]
            dx = torch.empty(B, Hh, Ww, Cin, dtype=torch.float32, device=g.device)
            with H.side_branch(dev, B * Hh * Ww):        # the data gradient next to the weight gradient below
                try:
                    H.gemm(g, wd, dx, B * Hh * Ww, Cin, 9 * Cout, lda=Cout, ldb=9 * Cout, ldc=Cin, conv=(Hh, Ww, Cout),
                           precision=ctx.prec)
                except H.GtNotSupported:         # gt_hip.h: on GT_ENOTSUP the caller takes the library convolution
                    dx = _library_conv_bwd(g, xc, weight, False)
        if ctx.needs_input_grad[1]:
            # dw[co][ci][tap] = sum_pix gy[pix][co] x[pix + shift(tap)][ci]
            dw = _conv3x3_wgrad(g.reshape(-1, Cout), Cout, xc.reshape(-1, Cin), Cin, weight, B, Hh, Ww, Cin, Cout, 1.0,
                                ctx.prec, wide=True)
        H.join_side(dev)
        return dx, dw, None


def conv3x3_nhwc_implicit(x) -> bool:
    """True when conv3x3_nhwc(x, .) runs the implicit GEMM (and so can carry act2)."""
    return x.shape[0] * x.shape[1] * x.shape[2] >= 96 and H.get_precision() != "f32"


def conv3x3_nhwc(x, weight, act2: bool = False):
    """x (B, H, W, Cin) channels-last, weight (Cout, Cin, 3, 3) -> (B, H, W, Cout); see Conv3x3NhwcFn.  Less than one
    tile of pixels (< 96) goes to the library convolution on the same buffers.
    act2: returns (silu(silu(conv)), fac) -- the caller hands `fac` to the ONLY consumer of the first result, whose backward
    must multiply the gradient by it (ops.upsample_fc(in_factor=fac)); implicit-GEMM path only (conv3x3_nhwc_implicit)."""
    if not conv3x3_nhwc_implicit(x):
        if act2:
            raise H.GtNotSupported("conv3x3_nhwc(act2=True) outside the implicit-GEMM path")
        # (the implicit GEMM exists on the split-operand engine only: gt_hip.h says GT_ENOTSUP -> the library convolution)
        return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), weight, padding=1).permute(0, 2, 3, 1).contiguous()
    if act2:
        return Conv3x3NhwcFn.apply(x, weight, True)
    return Conv3x3NhwcFn.apply(x, weight)


# ----------------------------------------------------------------------------------- down-scaler convolution chain
_scaler_chain = [os.environ.get("GT_SCALER_CHAIN", "1") != "0"]          # A/B switch (tools / tests)


def scaler_chain_ok(convs, act_name: str) -> bool:
    """True when the three narrow 3x3 convolutions of Interp2dEncoder (layers.py:431-512: conv1, conv2, conv3, each
    conv -> dropout -> ReLU, outputs concatenated) can run as ``scaler_conv_chain``: plain 3x3 / stride 1 / zero padding 1 /
    bias-free, chained channel counts, the first input a multiple of 16 channels, ReLU (it commutes with the dropout
    scale, so both ride on the product's epilogue) or SiLU (round 6: the epilogue applies the dropout in front of it,
    GT_ACT_DROP_SILU), the split-operand arithmetic."""
    if not (_scaler_chain[0] and act_name in ("relu", "silu") and H.get_precision() in H.SPLIT_EXACT and len(convs) == 3):
        return False
    if not all(_plain_conv3x3(c) for c in convs):
        return False
    c1, c2, c3 = convs
    return (c1.in_channels % 16 == 0 and c2.in_channels == c1.out_channels and c3.in_channels == c2.out_channels
            and 32 <= max(c.out_channels for c in convs) <= 64)


class ScalerConvChainFn(Function):
    """cat[x1, x2, x3] with x_i = act(dropout(conv3x3(x_{i-1}, w_i))), act = ReLU or SiLU, channels-last, as three implicit
    GEMMs that write straight into ONE buffer [B, H, W, 3 CP] (CP = the widest output rounded up to 16: each convolution
    owns a 16-byte aligned CP-column segment, its padding columns come out of the product as exact zeros because the padded
    filter rows are zero, and the next convolution reads its input segment in place -- no cat, no copies, no layout change).
    Reference: Interp2dEncoder.forward, layers.py:497-507 (conv1 -> conv2 -> conv3 -> torch.cat) with Conv2dResBlock
    (layers.py:88-150: conv -> dropout -> activation).  Dropout and activation sit in the epilogue of the product.
    ReLU commutes with the non-negative dropout scale and the backward needs only the activated outputs: y > 0 <=> kept
    and pre-activation > 0.  SiLU (Interp2dEncoder's default, ex3's down-scaler; round 6) does not: the epilogue applies
    the dropout in FRONT of it (GT_ACT_DROP_SILU) and leaves the factor of the backward, keepscale * silu'(u), in a second
    buffer `fac` of the same layout (returned, non-differentiable: bilinear_resize_seg(in_factor=fac) multiplies the
    gradient with it on the way out).  Backward: per convolution (last to first) the data gradient is an implicit GEMM on
    the tap-reversed filter whose epilogue multiplies by the previous segment's mask / factor and adds that segment's own
    masked gradient (into a buffer of the backward: the incoming gradient is read-only), and the weight gradient runs next
    to it on the side stream."""

    @staticmethod
    def forward(ctx, x0, w1, w2, w3, p_drop: float, grad_masked: bool = False, act: int = H.ACT_RELU):
        H.need_f32_cuda(x0, w1, w2, w3)
        B, Hh, Ww, C0 = x0.shape
        ws = (w1, w2, w3)
        CP = (max(w.shape[0] for w in ws) + 15) // 16 * 16
        T = B * Hh * Ww
        dev = x0.device
        x0c = _c(x0)
        silu = act == H.ACT_SILU
        cat = torch.empty(T, 3 * CP, dtype=torch.float32, device=dev)
        fac = torch.empty(T, 3 * CP, dtype=torch.float32, device=dev) if silu else None
        salt = _next_salt(3)
        cin = (C0, CP, CP)
        ctx.prec = H.get_precision()             # bf16x3 or f16x2 (scaler_chain_ok); the backward runs in the same arithmetic
        for i, w in enumerate(ws):
            wf = _filter_fwd(w, CP, cin[i])      # [CP, 9 cin] in k order
            A = x0c.reshape(T, C0) if i == 0 else cat[:, (i - 1) * CP:i * CP]
            H.gemm(A, wf, cat[:, i * CP:(i + 1) * CP], T, CP, 9 * cin[i], lda=(C0 if i == 0 else 3 * CP), ldb=9 * cin[i],
                   ldc=3 * CP, conv=(Hh, Ww, cin[i]), act=H.ACT_DROP_SILU if silu else H.ACT_RELU,
                   pre=fac[:, i * CP:(i + 1) * CP] if silu else None, ldpre=3 * CP,
                   drop=H.dropout_desc(p_drop, salt + i, dev) if p_drop > 0 else None, precision=ctx.prec)
        if _scaler_mask_sink[0] is not None:
            # ReLU: kept and positive.  SiLU: kept (the factor keepscale * silu'(u) vanishes only where the dropout struck)
            c4 = (fac if silu else cat).view(B, Hh, Ww, 3 * CP)
            _scaler_mask_sink[0].append([(c4[..., i * CP:i * CP + w.shape[0]] != 0) if silu else
                                         (c4[..., i * CP:i * CP + w.shape[0]] > 0) for i, w in enumerate(ws)])
        ctx.save_for_backward(x0c, w1, w2, w3, cat, fac)
        ctx.cfg = (p_drop, CP, grad_masked, silu)
        out = cat.view(B, Hh, Ww, 3 * CP)
        if not silu:
            return out
        fac4 = fac.view(B, Hh, Ww, 3 * CP)
        ctx.mark_non_differentiable(fac4)
        ctx.set_materialize_grads(False)         # (no zero gradient the size of `fac` from autograd)
        return out, fac4

    @staticmethod
    def backward(ctx, g, _gfac=None):
        if g is None:
            return (None,) * 7
        x0c, w1, w2, w3, cat, fac = ctx.saved_tensors
        p_drop, CP, grad_masked, silu = ctx.cfg
        prec = ctx.prec
        B, Hh, Ww, C0 = x0c.shape
        T = B * Hh * Ww
        dev = g.device
        ws = (w1, w2, w3)
        cin = (C0, CP, CP)
        # ReLU: the dropout scale rides on the products' alpha; SiLU: it is part of `fac`
        scale = 1.0 if silu else 1.0 / (1.0 - p_drop)
        # masked gradient of the three activated outputs in one pass
        # (grad_masked: the consumer -- bilinear_resize_seg(relu_input=True / in_factor=fac) -- has already applied it).
        # The incoming gradient is never written: the completed gradients of segments 0 and 1 (their own masked gradient
        # + the data gradient of the convolution behind them) go to a buffer of this function, so a hook / retain_grad on
        # the chain's output, or a second consumer summed by autograd, sees and produces what it should.
        g2 = _c(g).reshape(T, 3 * CP)
        gsrc = g2 if grad_masked else (g2 * fac if silu else H.act_bwd(g2, cat, H.ACT_RELU))
        acc = torch.empty(T, 2 * CP, dtype=torch.float32, device=dev)
        dws = [None, None, None]
        dx0 = None
        for i in (2, 1, 0):
            seg, ldseg = (gsrc[:, 2 * CP:], 3 * CP) if i == 2 else (acc[:, i * CP:(i + 1) * CP], 2 * CP)
            xin, ldx = (x0c.reshape(T, C0), C0) if i == 0 else (cat[:, (i - 1) * CP:i * CP], 3 * CP)
            if ctx.needs_input_grad[1 + i]:
                with H.side_branch(dev, T):
                    dws[i] = _conv3x3_wgrad(seg, ldseg, xin, ldx, ws[i], B, Hh, Ww, cin[i], CP, scale, prec, wide=False)
            # dx[pix][ci] = scale * sum_tap sum_co dpre[pix - shift(tap)][co] W[co][ci][tap]: tap' = 8 - tap
            if i > 0 or ctx.needs_input_grad[0]:
                wd = _filter_dgrad(ws[i], cin[i], CP)    # [cin, 9 CP] in k order
                if i == 0:
                    dx0 = torch.empty(T, C0, dtype=torch.float32, device=dev)
                    H.gemm(seg, wd, dx0, T, C0, 9 * CP, lda=ldseg, ldb=9 * CP, ldc=C0, conv=(Hh, Ww, CP), alpha=scale,
                           precision=prec)
                else:       # + the segment's own masked gradient (res), through its ReLU / dropout mask or its SiLU factor (aux)
                    aux = (fac if silu else cat)[:, (i - 1) * CP:i * CP]
                    H.gemm(seg, wd, acc[:, (i - 1) * CP:i * CP], T, CP, 9 * CP, lda=ldseg, ldb=9 * CP, ldc=2 * CP,
                           conv=(Hh, Ww, CP), alpha=scale, aux_op=H.AUX_MUL if silu else H.AUX_GT0, aux=aux, ldaux=3 * CP,
                           res=gsrc[:, (i - 1) * CP:i * CP], ldr=3 * CP, precision=prec)
            H.join_side(dev)        # the next weight gradient reads the segment this data gradient has just completed
        return (None if dx0 is None else dx0.view(B, Hh, Ww, C0)), dws[0], dws[1], dws[2], None, None, None


def scaler_conv_chain(x0, w1, w2, w3, p_drop: float = 0.0, training: bool = True, grad_masked: bool = False,
                      act: str = "relu"):
    """x0 (B, H, W, C0) channels-last -> (B, H, W, 3 CP): see ScalerConvChainFn; column segment i holds x_{i+1} in its
    first w_i.shape[0] columns, zeros behind them.  grad_masked: the ONLY consumer of the result is
    bilinear_resize_seg(relu_input=True) (act='silu': in_factor=fac), whose backward hands the gradient over already
    multiplied by [result > 0] (by fac) -- the masking pass of the backward is then skipped; the gradient itself is only
    read.  act='silu' returns (buffer, fac)."""
    if act not in ("relu", "silu"):
        raise NotImplementedError(f"scaler_conv_chain: activation {act!r}")
    return ScalerConvChainFn.apply(x0, w1, w2, w3, float(p_drop) if training else 0.0, bool(grad_masked), H.ACT_CODE[act])
