"""Dense operators: Linear, the regression head, FeedForward, and the zero-copy view over packed parameters.
"""
from __future__ import annotations

import os

import torch
from torch.autograd import Function

from .. import _hip as H
from ._handoff import _hint_output_mask, _offer_twin, _relu_mask_sink, _take_gate, _take_twin, _wanted_mask
from .elementwise import _c, _next_salt


_ffn_bwd_fused = [os.environ.get("GT_FFN_BWD_FUSED", "1") != "0"]      # data half of the FeedForward backward in one launch (gt_ffn_bwd)


class _PackedParamsFn(Function):
    """cat(params, dim 0) of parameters that lie back to back in memory: the result is a VIEW over them (no copy), and
    the gradient is handed back as slices of the packed gradient (no copies either)."""

    @staticmethod
    def forward(ctx, *params):
        ctx.rows = [p.shape[0] for p in params]
        p0 = params[0]
        rows = sum(ctx.rows)
        out = p0.detach().as_strided((rows,) + tuple(p0.shape[1:]), p0.stride())
        return out

    @staticmethod
    def backward(ctx, g):
        outs, r0 = [], 0
        for r in ctx.rows:
            outs.append(g[r0:r0 + r])
            r0 += r
        return tuple(outs)


def packed_params(params):
    """torch.cat(params, 0) -- as a zero-copy view when the tensors follow each other in memory (FlatClipAdam(model=...)
    lays SimpleAttention's groups out that way), else as the copy it always was.  1-D parameters of equal length stack to
    [len(params) * n] (callers view it)."""
    ok = all(p.is_contiguous() and p.dtype == params[0].dtype and p.shape[1:] == params[0].shape[1:] for p in params)
    if ok:
        nxt = params[0].data_ptr()
        for p in params:
            if p.data_ptr() != nxt:
                ok = False
                break
            nxt += p.numel() * p.element_size()
    if ok and params[0].is_cuda:
        st = params[0].untyped_storage()
        last = params[-1]
        ok = last.data_ptr() + last.numel() * last.element_size() <= st.data_ptr() + st.nbytes()
    if ok and params[0].is_cuda:
        return _PackedParamsFn.apply(*params)
    return torch.cat(list(params), dim=0)


# ----------------------------------------------------------------------------------- Linear
class LinearFn(Function):
    """y = res + out_scale * dropout(act(x W^T + b + extra W_e^T)).

    ``extra`` (optional, [.., p] with small p) folds ``torch.cat([x, extra], -1)`` followed by a Linear
    over the concatenation into one GEMM + rank-p epilogue (model.py:615-617, 507-512); W then has
    in_features = K + p.  Replaces nn.Linear (+ activation + nn.Dropout) at layers.py:964-987,
    model.py:615-629.  Returns y (and keeps the pre-activation for SiLU backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, extra, act: int, p_drop: float):
        H.need_f32_cuda(x, weight, bias, extra)
        K = x.shape[-1]
        N = weight.shape[0]
        pe = 0 if extra is None else extra.shape[-1]
        assert weight.shape[1] == K + pe
        x2 = _c(x).reshape(-1, K)
        T = x2.shape[0]
        w = _c(weight)
        y = torch.empty(T, N, dtype=torch.float32, device=x.device)
        pre = torch.empty(T, N, dtype=torch.float32, device=x.device) if act == H.ACT_SILU else None
        e2 = None if extra is None else _c(extra).reshape(T, pe)
        salt = _next_salt()
        drop = H.dropout_desc(p_drop, salt, x.device) if p_drop > 0 else None
        H.gemm(x2, w, y, T, N, K, lda=K, ldb=K + pe, ldc=N, bias=bias, act=act,
               rp=pe, rp_a=e2, rp_lda=pe, rp_b=(w[:, K:] if pe else None), rp_ldb=K + pe,
               pre=pre, ldpre=N, drop=drop)
        ctx.save_for_backward(x2, w, e2, pre if act == H.ACT_SILU else (y if act == H.ACT_RELU else None))
        ctx.cfg = (act, p_drop, salt, K, N, pe, bias is not None, x.shape)
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, gy):
        x2, w, e2, saved = ctx.saved_tensors
        act, p_drop, salt, K, N, pe, has_bias, xshape = ctx.cfg
        dev = gy.device
        T = x2.shape[0]
        g = _c(gy).reshape(T, N)
        # dpre = g * dropmask * act'(pre)
        if act == H.ACT_NONE and p_drop == 0:
            gp = g
        else:
            gp = torch.empty_like(g)
            if act == H.ACT_SILU:
                gp = H.act_bwd(g, saved, H.ACT_SILU)
                if p_drop > 0:
                    gp = H.dropout_apply(gp, H.dropout_desc(p_drop, salt, dev))
            elif act == H.ACT_RELU:
                # y = relu(pre)*mask*s : y>0 <=> kept and pre>0
                gp = H.act_bwd(g, saved, H.ACT_RELU)
                if p_drop > 0:
                    gp = gp * (1.0 / (1.0 - p_drop))
            else:
                gp = H.dropout_apply(g, H.dropout_desc(p_drop, salt, dev))
        dx = de = dw = db = None
        want_db = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:     # weight gradient on the side stream, next to the data gradient (H.side_branch)
            dw = torch.empty(N, K + pe, dtype=torch.float32, device=dev)
            if want_db:         # the bias gradient rides on the weight-gradient GEMM (row sums of its A)
                db = torch.empty(N, dtype=torch.float32, device=dev)
            with H.side_branch(dev, T):
                H.gemm(gp, x2, dw, N, K, T, layout_a=1, layout_b=1, lda=N, ldb=K, ldc=K + pe, split_k=0,
                       a_colsum=db)
                if pe:
                    H.gemm(gp, e2, dw[:, K:], N, pe, T, layout_a=1, layout_b=1, lda=N, ldb=pe, ldc=K + pe,
                           split_k=0)
        elif want_db:
            db = H.colsum(gp, T, N, N)
        if ctx.needs_input_grad[0]:
            dx = torch.empty(T, K, dtype=torch.float32, device=dev)
            H.gemm(gp, w, dx, T, K, N, layout_b=1, lda=N, ldb=K + pe, ldc=K)
            dx = dx.reshape(xshape)
        H.join_side(dev)
        return dx, dw, db, de, None, None


def linear(x, weight, bias=None, extra=None, act: str = None, p_drop: float = 0.0):
    if extra is not None and extra.requires_grad:
        raise NotImplementedError("ops.linear: `extra` (the concatenated coordinates) gets no gradient")
    return LinearFn.apply(x, weight, bias, extra, H.ACT_CODE[act], float(p_drop))


class MlpHeadFn(Function):
    """y = W2 act(W1 x + b1) + b2 with a narrow output (n_out <= 4) and hidden width <= 128: the tail of
    SpectralRegressor / PointwiseRegressor (model.py:575-580, 625-629).  The [T, hidden] activation never
    reaches HBM in forward (row-dot epilogue); backward recomputes the pre-activation inside the GEMM that
    produces dL/dh and gets dW2 as a by-product of the same launch."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act: int):
        H.need_f32_cuda(x, w1, b1, w2, b2)
        K, N, no = x.shape[-1], w1.shape[0], w2.shape[0]
        x2 = _c(x).reshape(-1, K)
        T = x2.shape[0]
        w1c, w2c = _c(w1), _c(w2)
        out = torch.empty(T, no, dtype=torch.float32, device=x.device)
        ctx.prec = H.get_precision()              # the backward runs in the arithmetic of the forward
        if H.mlp_head_supported(K, N, no):       # dedicated one-pass kernel (gt_mlp_head_fwd)
            H.mlp_head_fwd(x2, w1c, b1, w2c, b2, act, out, precision=ctx.prec)
        else:
            H.gemm(x2, w1c, None, T, N, K, lda=K, ldb=K, ldc=N, bias=b1, act=act, ep_mode=H.EP_ROWDOT, w2=w2c,
                   b2=b2, out2=out)
        gate = _take_gate(x2) if ctx.needs_input_grad[0] else None
        ctx.save_for_backward(x2, w1c, b1, w2c, gate)
        ctx.cfg = (act, K, N, no, b1 is not None, b2 is not None, x.shape)
        return out.reshape(*x.shape[:-1], no)

    @staticmethod
    def backward(ctx, gy):
        x2, w1c, b1, w2c, gate = ctx.saved_tensors
        act, K, N, no, hb1, hb2, xshape = ctx.cfg
        dev, T = gy.device, x2.shape[0]
        g = _c(gy).reshape(T, no)
        f32 = dict(dtype=torch.float32, device=dev)
        if H.mlp_head_supported(K, N, no):       # everything in one pass over x (gt_mlp_head_bwd)
            dx = torch.empty(T, K, **f32) if ctx.needs_input_grad[0] else None
            dw1, dw2 = torch.empty(N, K, **f32), torch.empty(no, N, **f32)
            db1 = torch.empty(N, **f32) if hb1 else None
            db2 = torch.empty(no, **f32) if hb2 else None
            H.mlp_head_bwd(x2, w1c, b1, w2c, act, g, dx, dw1, db1, dw2, db2, precision=ctx.prec,
                           dx_gate=None if gate is None else gate.reshape(T, K))
            return (dx.reshape(xshape) if dx is not None else None), dw1, db1, dw2, db2, None
        dh, dw2 = torch.empty(T, N, **f32), torch.empty(no, N, **f32)
        H.gemm(x2, w1c, dh, T, N, K, lda=K, ldb=K, ldc=N, bias=b1, act=act, ep_mode=H.EP_MLP_BWD, w2=w2c, g2=g,
               dw2=dw2)
        db2 = H.colsum(g, T, no, no) if hb2 else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(T, K, **f32)
            H.gemm(dh, w1c, dx, T, K, N, layout_b=1, lda=N, ldb=K, ldc=K)
            if gate is not None:
                dx = H.act_bwd(dx, gate.reshape(T, K), H.ACT_SILU)
            dx = dx.reshape(xshape)
        dw1 = torch.empty(N, K, **f32)
        db1 = torch.empty(N, **f32) if hb1 else None
        H.gemm(dh, x2, dw1, N, K, T, layout_a=1, layout_b=1, lda=N, ldb=K, ldc=K, split_k=0, a_colsum=db1)
        return dx, dw1, db1, dw2, db2, None


def mlp_head(x, w1, b1, w2, b2, act: str = "silu"):
    """Fused two-layer pointwise head when it fits the kernel (hidden <= 128, n_out <= 4), else two linears."""
    if w1.shape[0] <= 128 and w2.shape[0] <= 4 and w2.shape[1] == w1.shape[0]:
        return MlpHeadFn.apply(x, w1, b1, w2, b2, H.ACT_CODE[act])
    return linear(linear(x, w1, b1, act=act), w2, b2)


def _check_res_is_x(res, x, what: str):
    """The fused backward passes return d(res) folded into d(x): only valid when the residual input IS x."""
    if res is not None and res is not x and not (res.data_ptr() == x.data_ptr() and res.shape == x.shape
                                                 and res.stride() == x.stride()):
        raise ValueError(f"ops.{what}: `res` must be the input tensor itself (or None)")


# ----------------------------------------------------------------------------------- FFN
class FeedForwardFn(Function):
    """out = res + dropout2(lr2(dropout_h(act(lr1(x)))))   (layers.py:979-987 + model.py:131-132).

    res=None gives the bare FeedForward.forward."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, res, act: int, p_h: float, p_out: float):
        H.need_f32_cuda(x, w1, b1, w2, b2, res)
        if act not in (H.ACT_RELU, H.ACT_SILU):
            raise NotImplementedError("FeedForward HIP path implements relu and silu")
        d, f, dout = x.shape[-1], w1.shape[0], w2.shape[0]
        xc = _c(x).reshape(-1, d)
        T = xc.shape[0]
        dev = x.device
        w1c, w2c = _c(w1), _c(w2)
        salt = _next_salt()
        hid = torch.empty(T, f, dtype=torch.float32, device=dev)
        pre = torch.empty(T, f, dtype=torch.float32, device=dev) if act == H.ACT_SILU else None
        out = torch.empty(T, dout, dtype=torch.float32, device=dev)
        rc = None if res is None else _c(res).reshape(T, dout)
        d_h = H.dropout_desc(p_h, salt, dev) if p_h > 0 else None
        d_o = H.dropout_desc(p_out, salt + 1, dev) if p_out > 0 else None
        bits = None
        if dout == d and H.ffn_fwd_supported(T, d, f, act):
            # both products in ONE launch, the hidden tile of 64 token rows kept in LDS between them (gt_ffn.hip): hid is
            # written for the backward (dW2) and never read back here; the ReLU / dropout decisions go along as one bit per
            # value for the fused data half of the backward
            bits = H.ffn_fwd(xc, w1c, b1, w2c, b2, rc, d_h, d_o, act, hid, out,
                             want_bits=bool(act == H.ACT_RELU and _ffn_bwd_fused[0] and any(ctx.needs_input_grad[:5])))
        else:
            H.gemm(xc, w1c, hid, T, f, d, lda=d, ldb=d, ldc=f, bias=b1, act=act, pre=pre, ldpre=f, drop=d_h, weight_b=True)
            H.gemm(hid, w2c, out, T, dout, f, lda=f, ldb=f, ldc=dout, bias=b2, drop=d_o, res=rc, ldr=dout, weight_b=True)
        if _relu_mask_sink[0] is not None and act == H.ACT_RELU and p_h == 0:
            _relu_mask_sink[0].append(hid > 0)
        ctx.save_for_backward(xc, w1c, w2c, hid, pre, bits)
        ctx.cfg = (act, p_h, p_out, salt, d, f, dout, b1 is not None, b2 is not None, res is not None,
                   x.shape)
        ctx.in_mask = _wanted_mask(xc)            # the producer of x wants d(x) under its own output mask too
        _hint_output_mask(out, p_out, salt + 1)
        return out.reshape(*x.shape[:-1], dout)

    @staticmethod
    def backward(ctx, gy):
        xc, w1c, w2c, hid, pre, bits = ctx.saved_tensors
        act, p_h, p_out, salt, d, f, dout, hb1, hb2, has_res, xshape = ctx.cfg
        dev = gy.device
        T = xc.shape[0]
        g = _c(gy).reshape(T, dout)
        # the masked gradient g*mask_out feeds three contractions: one elementwise pass is cheaper than
        # regenerating the mask in each GEMM's operand loader (measured: 257 -> 135 us on the gh GEMM at B=64)
        gm = g
        if p_out > 0:           # the masked copy the consumer of our output wrote next to d(out), else the elementwise pass
            gm = _take_twin(g, p_out, salt + 1)
            if gm is None:
                gm = H.dropout_apply(g, H.dropout_desc(p_out, salt + 1, dev))
        # gh = (gm W2) * mask_h * act'(pre)
        gh = torch.empty(T, f, dtype=torch.float32, device=dev)
        # bias gradients ride on the weight-gradient GEMMs (row sums of their A operand); the weight gradients run on
        # the side stream next to the data-gradient GEMMs (H.side_branch)
        dw2 = torch.empty(dout, f, dtype=torch.float32, device=dev)
        db2 = torch.empty(dout, dtype=torch.float32, device=dev) if hb2 else None
        with H.side_branch(dev, T):
            H.gemm(gm, hid, dw2, dout, f, T, layout_a=1, layout_b=1, lda=dout, ldb=f, ldc=f, split_k=0,
                   a_colsum=db2)
        dx = torch.empty(T, d, dtype=torch.float32, device=dev)
        same = has_res and dout == d
        dxm, want = None, ctx.in_mask
        if want is not None:
            dxm = torch.empty_like(dx)
        fused_bwd = bits is not None and act == H.ACT_RELU
        if fused_bwd:
            # gh = (gm W2) through the forward's decision bits, dx = g + gh W1 and its masked twin: ONE launch, the hidden
            # activation is not read (gt_ffn_bwd); dW1 = gh^T x follows on the side stream
            H.ffn_bwd(gm, w2c, w1c, bits, 1.0 / (1.0 - p_h), g if same else None, gh, dx, dxm,
                      H.dropout_desc(want[0], want[1], dev) if want else None)
        elif act == H.ACT_RELU:
            H.gemm(gm, w2c, gh, T, f, dout, layout_b=1, lda=dout, ldb=f, ldc=f,
                   aux_op=H.AUX_GT0, aux=hid, ldaux=f, aux_scale=1.0 / (1.0 - p_h), weight_b=True)
        else:
            H.gemm(gm, w2c, gh, T, f, dout, layout_b=1, lda=dout, ldb=f, ldc=f,
                   aux_op=H.AUX_DSILU, aux=pre, ldaux=f,
                   drop=H.dropout_desc(p_h, salt, dev) if p_h > 0 else None, weight_b=True)
        dw1 = torch.empty(f, d, dtype=torch.float32, device=dev)
        db1 = torch.empty(f, dtype=torch.float32, device=dev) if hb1 else None
        with H.side_branch(dev, T):
            H.gemm(gh, xc, dw1, f, d, T, layout_a=1, layout_b=1, lda=f, ldb=d, ldc=d, split_k=0, a_colsum=db1)
        if not fused_bwd:
            H.gemm(gh, w1c, dx, T, d, f, layout_b=1, lda=f, ldb=d, ldc=d, res=g if same else None, ldr=d, weight_b=True,
                   c_masked=dxm, ldc_masked=d, c_mask=H.dropout_desc(want[0], want[1], dev) if want else None)
        if dxm is not None:
            _offer_twin(dx, dxm, *want)
        H.join_side(dev)
        dx = dx.reshape(xshape)
        # the residual input is x itself: its gradient g is already folded into dx (res epilogue above), so the
        # `res` slot contributes nothing (None) -- no zero fill, no extra add in autograd
        dres = None if (not has_res or same) else gy
        return dx, dw1, db1, dw2, db2, dres, None, None, None


def feed_forward(x, w1, b1, w2, b2, res=None, act="relu", p_h=0.0, p_out=0.0):
    """res must be x itself (or None): the fused backward folds d(res) into d(x)."""
    _check_res_is_x(res, x, "feed_forward")
    return FeedForwardFn.apply(x, w1, b1, w2, b2, res, H.ACT_CODE[act], float(p_h), float(p_out))


class FeedForwardBNFn(Function):
    """out = res + dropout2(lr2(BatchNorm1d(dropout_h(act(lr1(x))))))   (layers.py:979-987 with batch_norm=True).

    The norm keeps one mean and one biased variance per hidden channel over all T = B n token rows and sits BEHIND the
    hidden dropout, so its statistics see the dropped, rescaled values.  training: batch statistics, running_mean /
    running_var updated in place; else the running buffers are the statistics and the backward has no mean terms.  The two
    products are FeedForwardFn's unfused pair; between them gt_batchnorm_fwd writes z next to hid (the backward needs both:
    dW2 contracts z, the norm's backward recomputes xh and the ReLU gate from hid)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, running_mean, running_var, res, act: int, p_h: float, p_out: float,
                eps: float, momentum: float, training: bool):
        H.need_f32_cuda(x, w1, b1, w2, b2, gamma, beta, running_mean, running_var, res)
        if act not in (H.ACT_RELU, H.ACT_SILU):
            raise NotImplementedError("FeedForward HIP path with batch_norm implements relu and silu")
        d, f, dout = x.shape[-1], w1.shape[0], w2.shape[0]
        xc = _c(x).reshape(-1, d)
        T = xc.shape[0]
        dev = x.device
        if training and T < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        if H.lib().gt_batchnorm_ws_bytes(T, f) == 0:      # refused before anything is launched
            raise H.GtNotSupported(f"gt_batchnorm_fwd: no kernel for a hidden width of {f} (a multiple of 4 is needed)")
        w1c, w2c, gc = _c(w1), _c(w2), _c(gamma)
        salt = _next_salt()
        hid = torch.empty(T, f, dtype=torch.float32, device=dev)
        pre = torch.empty(T, f, dtype=torch.float32, device=dev) if act == H.ACT_SILU else None
        out = torch.empty(T, dout, dtype=torch.float32, device=dev)
        rc = None if res is None else _c(res).reshape(T, dout)
        d_h = H.dropout_desc(p_h, salt, dev) if p_h > 0 else None
        d_o = H.dropout_desc(p_out, salt + 1, dev) if p_out > 0 else None
        H.gemm(xc, w1c, hid, T, f, d, lda=d, ldb=d, ldc=f, bias=b1, act=act, pre=pre, ldpre=f, drop=d_h, weight_b=True)
        z, stats, _ = H.batchnorm_fwd(hid, gc, _c(beta), eps, running_mean, running_var, momentum, training)
        H.gemm(z, w2c, out, T, dout, f, lda=f, ldb=f, ldc=dout, bias=b2, drop=d_o, res=rc, ldr=dout, weight_b=True)
        ctx.save_for_backward(xc, w1c, w2c, hid, pre, z, gc, stats)
        ctx.cfg = (act, p_h, p_out, salt, d, f, dout, b1 is not None, b2 is not None, res is not None, x.shape,
                   bool(training))
        ctx.in_mask = _wanted_mask(xc)            # the producer of x wants d(x) under its own output mask too
        _hint_output_mask(out, p_out, salt + 1)
        return out.reshape(*x.shape[:-1], dout)

    @staticmethod
    def backward(ctx, gy):
        xc, w1c, w2c, hid, pre, z, gc, stats = ctx.saved_tensors
        act, p_h, p_out, salt, d, f, dout, hb1, hb2, has_res, xshape, training = ctx.cfg
        dev = gy.device
        T = xc.shape[0]
        g = _c(gy).reshape(T, dout)
        gm = g
        if p_out > 0:           # the masked copy the consumer of our output wrote next to d(out), else the elementwise pass
            gm = _take_twin(g, p_out, salt + 1)
            if gm is None:
                gm = H.dropout_apply(g, H.dropout_desc(p_out, salt + 1, dev))
        # weight gradients on the side stream, bias gradients as row sums of their A operand (as in FeedForwardFn)
        dw2 = torch.empty(dout, f, dtype=torch.float32, device=dev)
        db2 = torch.empty(dout, dtype=torch.float32, device=dev) if hb2 else None
        with H.side_branch(dev, T):
            H.gemm(gm, z, dw2, dout, f, T, layout_a=1, layout_b=1, lda=dout, ldb=f, ldc=f, split_k=0, a_colsum=db2)
        # dz = gm W2, then the norm's backward with the activation / dropout gate on its store: gh is written once
        dz = torch.empty(T, f, dtype=torch.float32, device=dev)
        H.gemm(gm, w2c, dz, T, f, dout, layout_b=1, lda=dout, ldb=f, ldc=f, weight_b=True)
        if act == H.ACT_RELU:
            gate = (H.AUX_GT0, None, 1.0 / (1.0 - p_h), None)
        else:
            gate = (H.AUX_DSILU, pre, 1.0, H.dropout_desc(p_h, salt, dev) if p_h > 0 else None)
        gh, dgamma, dbeta = H.batchnorm_bwd(hid, dz, gc, stats, training, gate=gate, out=dz)
        dw1 = torch.empty(f, d, dtype=torch.float32, device=dev)
        db1 = torch.empty(f, dtype=torch.float32, device=dev) if hb1 else None
        with H.side_branch(dev, T):
            H.gemm(gh, xc, dw1, f, d, T, layout_a=1, layout_b=1, lda=f, ldb=d, ldc=d, split_k=0, a_colsum=db1)
        dx = torch.empty(T, d, dtype=torch.float32, device=dev)
        same = has_res and dout == d
        dxm, want = None, ctx.in_mask
        if want is not None:
            dxm = torch.empty_like(dx)
        H.gemm(gh, w1c, dx, T, d, f, layout_b=1, lda=f, ldb=d, ldc=d, res=g if same else None, ldr=d, weight_b=True,
               c_masked=dxm, ldc_masked=d, c_mask=H.dropout_desc(want[0], want[1], dev) if want else None)
        if dxm is not None:
            _offer_twin(dx, dxm, *want)
        H.join_side(dev)
        dx = dx.reshape(xshape)
        dres = None if (not has_res or same) else gy      # res is x: its gradient is folded into dx
        return (dx, dw1, db1, dw2, db2, dgamma, dbeta, None, None, dres) + (None,) * 6


def feed_forward_bn(x, w1, b1, w2, b2, gamma, beta, running_mean, running_var, res=None, act="relu", p_h=0.0, p_out=0.0,
                    eps=1e-5, momentum=0.1, training=True):
    """FeedForward with BatchNorm1d(gamma, beta, running_mean, running_var) between the hidden dropout and lr2.  res must
    be x itself (or None): the fused backward folds d(res) into d(x).  training=True updates the running buffers in place
    (num_batches_tracked is the module's business); act: 'relu' or 'silu' -- 'gelu' raises NotImplementedError, the GEMM
    epilogues and the norm's gate carry relu / silu only."""
    _check_res_is_x(res, x, "feed_forward_bn")
    return FeedForwardBNFn.apply(x, w1, b1, w2, b2, gamma, beta, running_mean, running_var, res, H.ACT_CODE[act],
                                 float(p_h), float(p_out), float(eps), float(momentum), bool(training))
