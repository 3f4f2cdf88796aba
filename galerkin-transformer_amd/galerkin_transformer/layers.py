"""Layer modules with the reference's names, constructor arguments, forward signatures and
state_dict keys (reference: libs/layers.py), whose hot-path arithmetic runs in libgt_hip.so.

Hot path (HIP):  SimpleAttention (:764), FeedForward (:954), SpectralConv1d (:1040),
SpectralConv2d (:1109).  Not on the hot path (plain PyTorch-ROCm / MIOpen, as SURVEY.md section 8
scopes them): the conv + bilinear-interpolation scalers (:88-150, :431-512, :624-670).  The 'conv' scaler modes
(Conv2dEncoder :284-341, DeConv2dBlock :515-559) run their pools and transposed convolutions on HIP operators.
"""
from __future__ import annotations

import copy
import math
import os

import numpy as np

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, xavier_normal_, xavier_uniform_
from torch.nn.parameter import Parameter

from . import _hip as H
from . import ops, spectral
from .ops import get_attention_dropout, push_attention_masks, set_attention_dropout  # noqa: F401


def default(value, d):
    return d if value is None else value


_LINEAR_FAMILY = ("linear", "galerkin", "global")
_HIP_ATTENTION = ("galerkin", "fourier", "integral", "local", "linear", "global")
_SOFTMAX_ATTENTION = ("softmax",)      # on the HIP path too, with coordinates only (SimpleAttention.fused_forward)
_CAUSAL_ATTENTION = ("causal",)        # causal linear attention (the decoder layer's second block), with or without coordinates


def _act_module(name, fallback="silu"):
    return nn.SiLU() if default(name, fallback) == "silu" else nn.ReLU()


def _act_name(module) -> str:
    if isinstance(module, nn.SiLU):
        return "silu"
    if isinstance(module, nn.ReLU):
        return "relu"
    if isinstance(module, nn.GELU) and getattr(module, "approximate", "none") == "none":
        return "gelu"
    if isinstance(module, (nn.Identity, Identity)):
        return "none"
    raise NotImplementedError(f"activation {type(module).__name__} has no HIP path")


# --------------------------------------------------------------------------------------- small helpers
class Identity(nn.Module):
    """Pass-through, or a Linear when both feature sizes are given (layers.py:21-41)."""

    def __init__(self, in_features=None, out_features=None, *args, **kwargs):
        super().__init__()
        if in_features is not None and out_features is not None:
            self.id = nn.Linear(in_features, out_features)
        else:
            self.id = nn.Identity()

    def forward(self, x, edge=None, grid=None):
        if isinstance(self.id, nn.Linear):
            return ops.linear(x, self.id.weight, self.id.bias)
        return x


class PositionalEncoding(nn.Module):
    """Sinusoidal table added to (B, n, d) inputs (layers.py:60-85); unused by the shipped configs."""

    def __init__(self, d_model, dropout=0.1, max_len=2 ** 13):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        position = torch.arange(max_len, dtype=torch.float).unsqueeze(1)
        freq = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(2 ** 13) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(position * freq)
        pe[:, 1::2] = torch.cos(position * freq)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return ops.dropout(x + self.pe[:, :x.size(1), :], self.dropout.p, self.training)


# --------------------------------------------------------------------------------------- CNN scalers (torch/MIOpen)
class Conv2dResBlock(nn.Module):
    """conv (no bias) -> dropout [-> act -> conv -> dropout] -> (+ shortcut) -> act (layers.py:88-150)."""

    def __init__(self, in_dim, out_dim, kernel_size=3, padding=1, dilation=1, dropout=0.1, stride=1,
                 bias=False, residual=False, basic_block=False, activation_type="silu"):
        super().__init__()
        self.activation = _act_module(activation_type)
        self.add_res = residual
        self.conv = nn.Sequential(
            nn.Conv2d(in_dim, out_dim, kernel_size=kernel_size, padding=padding, dilation=dilation,
                      stride=stride, bias=bias),
            nn.Dropout(dropout))
        self.basic_block = basic_block
        if basic_block:
            self.conv1 = nn.Sequential(
                self.activation,
                nn.Conv2d(out_dim, out_dim, kernel_size=kernel_size, padding=padding, bias=bias),
                nn.Dropout(dropout))
        self.apply_shortcut = in_dim != out_dim
        if residual:
            self.res = _Shortcut2d(in_dim, out_dim) if self.apply_shortcut else Identity()

    def forward(self, x):
        # nn.Dropout members are kept for the module tree / state_dict; the masks come from the
        # library's stateless RNG (ops.dropout) so the whole step shares one graph-safe seed.
        h = self.res(x) if self.add_res else None
        act = _act_name(self.activation)
        if self.basic_block:      # activation(dropout(conv(x))) is one elementwise pass (ops.drop_act)
            x = self.conv1[1](ops.drop_act(self.conv[0](x), self.conv[1].p, act, self.training))
            if not self.add_res:
                return ops.drop_act(x, self.conv1[2].p, act, self.training)
            x = ops.dropout(x, self.conv1[2].p, self.training)
        elif not self.add_res:
            return ops.drop_act(self.conv[0](x), self.conv[1].p, act, self.training)
        else:
            x = ops.dropout(self.conv[0](x), self.conv[1].p, self.training)
        return self.activation(x + h)

    def plain(self) -> bool:
        """conv -> dropout -> activation and nothing else (lets a caller fuse its own dropout/activation on)."""
        return not self.basic_block and not self.add_res


class _Shortcut2d(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.shortcut = nn.Linear(in_features, out_features)

    def forward(self, x, edge=None, grid=None):
        return self.shortcut(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


Shortcut2d = _Shortcut2d


# --------------------------------------------------------------------------------------- graph feature extractor
class GraphConvolution(nn.Module):
    """One GCN layer against a dense per-channel edge tensor (layers.py:153-198):
    out[b,c,i] = sum_j edge[b,c,i,j] (x W)[b,j,c] + bias[c].

    x is [B, n, in_features] or [B, in_features, n] (told apart by the reference's rule: a last axis that is not
    in_features means channels-first), edge [B, out_features, n, n]; returns [B, out_features, n] as the reference does.
    The product runs on gt_graphconv_* through ops.graph_conv_stack with one layer.  B = 1 keeps its batch axis (the
    reference's squeeze() drops it)."""

    def __init__(self, in_features, out_features, bias=True, debug=False):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.weight = Parameter(torch.empty(in_features, out_features))
        self.debug = debug
        if bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)

    def forward(self, x, edge):
        if x.size(-1) != self.in_features:
            x = x.transpose(-2, -1)
        assert x.size(1) == edge.size(-1)
        return ops.graph_conv_stack(x, edge, (self.weight,), (self.bias,), (False,)).permute(0, 2, 1)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class GraphAttention(nn.Module):
    """One GAT layer against a dense adjacency (layers.py:201-257), batched:
        h = node W;  e_ij = LeakyReLU_alpha(h_i . a[:F] + h_j . a[F:]) where adj keeps (i, j), else -9e15;
        out = ELU?(dropout(softmax_j(e)) h).
    adj keeps (i, j) where |adj_ij| > interaction_thresh (graph_lap) or adj_ij > 0.  The scores are rank-1 before the
    LeakyReLU, so the layer runs on the gt_graphattn_* kernels through ops.graph_attention_stack with one layer and never
    forms the reference's [B, n, n, 2F] input of the score product.  `dropout` is a plain float that follows
    module.training only (not set_attention_dropout); adj gets no gradient."""

    def __init__(self, in_features, out_features, alpha=1e-2, concat=True, graph_lap=True, interaction_thresh=1e-6,
                 dropout=0.1):
        super().__init__()
        self.dropout = dropout
        self.in_features = in_features
        self.out_features = out_features
        self.alpha = alpha
        self.concat = concat
        self.graph_lap = graph_lap
        self.thresh = interaction_thresh
        self.W = Parameter(torch.empty(in_features, out_features))
        xavier_normal_(self.W, gain=np.sqrt(2.0))
        self.a = Parameter(torch.empty(2 * out_features, 1))
        xavier_normal_(self.a, gain=np.sqrt(2.0))
        self.leakyrelu = nn.LeakyReLU(self.alpha)

    def stack_args(self):
        return dict(alpha=self.alpha, concat=self.concat, graph_lap=self.graph_lap, thresh=self.thresh,
                    p=float(self.dropout) if self.training else 0.0)

    def forward(self, node, adj):
        return ops.graph_attention_stack(node, adj, (self.W,), (self.a,), (False,), **self.stack_args())

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class EdgeEncoder(nn.Module):
    """Two 3x3 convolution blocks over the edge features, concatenated on the channel axis, the raw features in front with
    raw_laplacian (layers.py:260-281).  The convolutions are the library's (ops.edge_conv: with its deterministic weight
    gradient), their dropout -> SiLU tails ops.drop_act, as in Conv2dEncoder.  groups() hands GCN the pieces
    un-concatenated."""

    def __init__(self, out_dim: int, edge_feats: int, raw_laplacian=None):
        super().__init__()
        assert out_dim > edge_feats
        self.return_lap = raw_laplacian
        if self.return_lap:
            out_dim = out_dim - edge_feats
        conv_dim0 = int(out_dim / 3 * 2)
        conv_dim1 = int(out_dim - conv_dim0)
        self.lap_conv1 = Conv2dResBlock(edge_feats, conv_dim0)
        self.lap_conv2 = Conv2dResBlock(conv_dim0, conv_dim1)

    def _block(self, blk, x):
        # Conv2dResBlock's plain form, conv -> dropout -> activation, with the convolution through ops.edge_conv (the
        # library's kernels, its reproducible weight gradient) and the tail in one elementwise pass
        assert blk.plain()
        return ops.drop_act(ops.edge_conv(x, blk.conv[0]), blk.conv[1].p, _act_name(blk.activation), self.training)

    def groups(self, lap):
        edge1 = self._block(self.lap_conv1, lap)
        edge2 = self._block(self.lap_conv2, edge1)
        return (lap, edge1, edge2) if self.return_lap else (edge1, edge2)

    def forward(self, lap):
        return torch.cat(self.groups(lap), dim=1)


def _resize(x, size, act_module=None, in_nhwc=False, out_nhwc=False):
    """activation(F.interpolate(x, ..., mode='bilinear', align_corners=True)) on the HIP resize kernel;
    a ReLU is fused into the kernel, any other activation is applied on its output."""
    name = "none" if act_module is None else _act_name(act_module)
    y = ops.bilinear_resize(x, size, in_nhwc, out_nhwc, act="relu" if name == "relu" else None)
    return y if name in ("relu", "none") else act_module(y)


class Interp2dEncoder(nn.Module):
    """conv0 -> resize -> act -> conv1 -> conv2 -> conv3 -> cat -> resize -> act (layers.py:431-512)."""

    def __init__(self, in_dim, out_dim, kernel_size=3, stride=1, padding=1, dilation=1, interp_size=None,
                 residual=False, activation_type="silu", dropout=0.1, debug=False):
        super().__init__()
        c0 = out_dim // 3
        c1 = out_dim // 3
        c2 = int(out_dim - c0 - c1)
        pad1 = max(padding // 2, 1)
        pad2 = max(padding // 4, 1)
        activation_type = default(activation_type, "silu")
        self.interp_size = interp_size
        self.is_scale_factor = isinstance(interp_size[0], float) and isinstance(interp_size[1], float)
        common = dict(kernel_size=kernel_size, residual=residual, dropout=dropout,
                      activation_type=activation_type)
        self.conv0 = Conv2dResBlock(in_dim, out_dim, padding=padding, **common)
        self.conv1 = Conv2dResBlock(out_dim, c0, padding=pad1, stride=stride, **common)
        self.conv2 = Conv2dResBlock(c0, c1, dilation=dilation, padding=pad2, **common)
        self.conv3 = Conv2dResBlock(c1, c2, **common)
        self.activation = _act_module(activation_type)
        self.add_res = residual
        self.debug = debug

    def _fused_act(self, blocks):
        """'relu' / 'silu' when the encoder's own activation and every given block's are that one type, else None
        (Interp2dEncoder builds them all from one activation_type, layers.py:446-482)."""
        for name, cls in (("relu", nn.ReLU), ("silu", nn.SiLU)):
            if isinstance(self.activation, cls) and all(isinstance(c.activation, cls) for c in blocks):
                return name
        return None

    def _conv0_fusable(self, x) -> bool:
        """conv0 is the plain 3x3 / padding-1 / bias-free block on a <= 4-channel input that needs no
        gradient, with ReLU (or SiLU, round 6) on both sides of the resize: the case gt_conv3x3_resize_* implements."""
        c = self.conv0
        cv = c.conv[0]
        try:
            ops.out_size(x.shape[2], x.shape[3], self.interp_size[0])
        except NotImplementedError:     # per-axis scale factors
            return False
        return (self._fused_act((c,)) is not None and not c.add_res and not c.basic_block and ops._plain_conv3x3(cv)
                and cv.in_channels <= 4 and x.is_cuda and not (torch.is_grad_enabled() and x.requires_grad))

    def _chain_ok(self, x, out_nhwc) -> bool:
        """conv1 / conv2 / conv3 as ops.scaler_conv_chain: channels-last output wanted, plain ReLU (or SiLU) blocks without
        residual, equal dropout, widths [c, c, <= padded c] that the segment layout of the last resize describes."""
        cs = (self.conv1, self.conv2, self.conv3)
        act = self._fused_act(cs)
        if not (out_nhwc and x.is_cuda and not self.add_res and act is not None
                and all(c.plain() for c in cs)
                and len({c.conv[1].p for c in cs}) == 1):
            return False
        try:
            h1, w1 = ops.out_size(x.shape[2], x.shape[3], self.interp_size[0])
            h2, w2 = ops.out_size(h1, w1, self.interp_size[1])
        except NotImplementedError:     # per-axis scale factors
            return False
        if x.shape[0] * h1 * w1 < 1024 or w1 < 3 or h1 < 3:       # (16 384 until round 5: C2 at B <= 2 fell back to the library)
            return False
        convs = [c.conv[0] for c in cs]
        widths = [c.out_channels for c in convs]
        cp = (max(widths) + 15) // 16 * 16
        # what the segment resize kernels take: an even segment width (out_dim = 112 / 160 give 37 / 53: those run the
        # conv1 / conv2 / conv3 + cat path below), and an up-sampling factor below ~2 in the backward
        return (widths[0] == widths[1] and h2 > 0 and w2 > 0
                and H.bilinear2d_seg_supported(sum(widths), widths[0], cp, (h1, w1), (h2, w2))
                and ops.scaler_chain_ok(convs, act))

    def forward(self, x, out_nhwc=False):
        """x (B, C, H, W).  ``out_nhwc`` returns (B, H', W', C') with the layout change fused into the
        last resize (what DownScaler feeds the encoder)."""
        chain = self._chain_ok(x, out_nhwc)
        if self._conv0_fusable(x):
            # conv0 -> dropout -> act -> resize -> act in one pass; the out_dim-channel fine map never exists
            x = ops.conv3x3_resize(x, self.conv0.conv[0].weight, self.interp_size[0], self.conv0.conv[1].p,
                                   self.training, out_nhwc=chain, act=self._fused_act((self.conv0,)))
        else:
            x = _resize(self.conv0(x), self.interp_size[0], self.activation, out_nhwc=chain)
        if chain:
            # channels-last from here on: the three narrow convolutions (+ dropout + ReLU) write the column segments of
            # ONE padded buffer (implicit GEMMs, ops.scaler_conv_chain), the last resize reads the real channels out of it
            cs = (self.conv1, self.conv2, self.conv3)
            seg = cs[0].conv[0].out_channels
            n_out = sum(c.conv[0].out_channels for c in cs)
            act = self._fused_act(cs)
            buf = ops.scaler_conv_chain(x, *(c.conv[0].weight for c in cs), p_drop=cs[0].conv[1].p, training=self.training,
                                        grad_masked=True, act=act)
            if act == "silu":       # + the factor (dropout scale x silu') the last resize hands the gradient back through
                buf, fac = buf
                return ops.bilinear_resize_seg(buf, n_out, self.interp_size[1], seg, buf.shape[-1] // 3, act="silu",
                                               in_factor=fac)
            return ops.bilinear_resize_seg(buf, n_out, self.interp_size[1], seg, buf.shape[-1] // 3, act="relu",
                                           relu_input=True)
        x1 = self.conv1(x)
        x2 = self.conv2(x1)
        x3 = self.conv3(x2)
        out = torch.cat([x1, x2, x3], dim=1)
        if self.add_res:
            out = out + x
        return _resize(out, self.interp_size[1], self.activation, out_nhwc=out_nhwc)


class Conv2dEncoder(nn.Module):
    """conv0 -> AvgPool2d(2) -> act -> conv1 -> conv2 -> conv3 -> cat -> AvgPool2d(2) -> act (layers.py:284-341): the block
    of DownScaler(downsample_mode='conv'), about 1/4 subsampling.

    As in the reference the four Conv2dResBlocks get neither ``activation_type`` nor a dropout: they keep their own defaults
    (SiLU, Dropout(0.1)) whatever the encoder's activation is; only the two activations behind the pools follow
    ``activation_type``.  The pools (floor: an odd trailing row / column is dropped) and those activations are one HIP pass
    each (ops.avgpool2_act); ``pool0`` / ``pool1`` are kept for the module tree.  Only scaling_factor=2 has a kernel."""

    def __init__(self, in_dim: int, out_dim: int, kernel_size: int = 3, stride: int = 1, padding: int = 1, dilation: int = 1,
                 scaling_factor: int = 2, residual=False, activation_type="silu", debug=False):
        super().__init__()
        c0 = out_dim // 3
        c1 = out_dim // 3
        c2 = int(out_dim - c0 - c1)
        pad1 = max(padding // 2, 1)
        pad2 = max(padding // 4, 1)
        activation_type = default(activation_type, "silu")
        self.conv0 = Conv2dResBlock(in_dim, out_dim, kernel_size=kernel_size, padding=padding, residual=residual)
        self.conv1 = Conv2dResBlock(out_dim, c0, kernel_size=kernel_size, padding=pad1, stride=stride, residual=residual)
        self.conv2 = Conv2dResBlock(c0, c1, kernel_size=kernel_size, dilation=dilation, padding=pad2, residual=residual)
        self.conv3 = Conv2dResBlock(c1, c2, kernel_size=kernel_size, residual=residual)
        self.pool0 = nn.AvgPool2d(kernel_size=scaling_factor, stride=scaling_factor)
        self.pool1 = nn.AvgPool2d(kernel_size=scaling_factor, stride=scaling_factor)
        self.activation = _act_module(activation_type)
        self.debug = debug

    def _pool_act(self, pool, x, out_nhwc=False):
        k, s = pool.kernel_size, pool.stride
        if not (k in (2, (2, 2)) and s in (2, (2, 2)) and pool.padding in (0, (0, 0)) and not pool.ceil_mode):
            raise NotImplementedError(f"Conv2dEncoder: AvgPool2d(kernel_size={k}, stride={s}) has no HIP path "
                                      "(scaling_factor=2 only)")
        return ops.avgpool2_act(x, _act_name(self.activation), in_nhwc=False, out_nhwc=out_nhwc)

    def forward(self, x, out_nhwc=False):
        """x (B, C, H, W).  ``out_nhwc`` returns (B, H', W', C') with the layout change fused into the last pool."""
        H.need_f32_cuda(x)
        x = self._pool_act(self.pool0, self.conv0(x))
        x1 = self.conv1(x)
        x2 = self.conv2(x1)
        x3 = self.conv3(x2)
        return self._pool_act(self.pool1, torch.cat([x1, x2, x3], dim=1), out_nhwc=out_nhwc)


class DeConv2dBlock(nn.Module):
    """deconv0 -> dropout -> act -> deconv1 -> act (layers.py:515-559): the block of UpScaler(upsample_mode='conv'), about
    4x upsampling.  Both layers are nn.ConvTranspose2d(kernel_size=3, stride=2, output_padding) with bias, deconv0 with
    ``padding`` and deconv1 with max(padding // 2, 1); there is no dropout behind deconv1.  Each layer with what follows
    it is one operator (ops.conv_transpose3x3s2: a channel product on the GEMM engine + the gather kernel that adds bias,
    dropout and activation); the nn.ConvTranspose2d / nn.Dropout members hold the parameters and the module tree.
    Channel counts must be multiples of 4 (NotImplementedError otherwise), kernel_size 3 and stride 2."""

    def __init__(self, in_dim: int, hidden_dim: int, out_dim: int, stride: int = 2, kernel_size: int = 3, padding: int = 2,
                 output_padding: int = 1, dropout=0.1, activation_type="silu", debug=False):
        super().__init__()
        pad1 = max(padding // 2, 1)
        self.deconv0 = nn.ConvTranspose2d(in_channels=in_dim, out_channels=hidden_dim, kernel_size=kernel_size, stride=stride,
                                          output_padding=output_padding, padding=padding)
        self.deconv1 = nn.ConvTranspose2d(in_channels=hidden_dim, out_channels=out_dim, kernel_size=kernel_size,
                                          stride=stride, output_padding=output_padding, padding=pad1)
        self.activation = nn.SiLU() if activation_type == "silu" else nn.ReLU()       # (None is ReLU here, layers.py:548)
        self.dropout = nn.Dropout(dropout)
        self.debug = debug

    def _deconv(self, layer, x, p_drop):
        same = lambda v, want: tuple(v) == (want, want)
        if not (same(layer.kernel_size, 3) and same(layer.stride, 2) and same(layer.dilation, 1) and layer.groups == 1
                and layer.padding[0] == layer.padding[1] and layer.output_padding[0] == layer.output_padding[1]):
            raise NotImplementedError("DeConv2dBlock: only ConvTranspose2d(kernel_size=3, stride=2) with square padding has a "
                                      "HIP path")
        return ops.conv_transpose3x3s2(x, layer.weight, layer.bias, layer.padding[0], layer.output_padding[0], p_drop,
                                       _act_name(self.activation), self.training)

    def forward(self, x, in_nhwc=False, out_nhwc=False):
        """x (B, C, H, W), or (B, H, W, C) with ``in_nhwc``; the operators themselves are channels-last."""
        H.need_f32_cuda(x)
        if not in_nhwc:
            x = x.permute(0, 2, 3, 1)
        x = self._deconv(self.deconv0, x, self.dropout.p)
        x = self._deconv(self.deconv1, x, 0.0)
        return x if out_nhwc else x.permute(0, 3, 1, 2).contiguous()


_fuse_act2 = [os.environ.get("GT_CONV_ACT2", "1") != "0"]      # A/B switch: the up-scaler's two SiLUs on the convolution's epilogue


class Interp2dUpsample(nn.Module):
    """resize -> conv block -> dropout -> act -> resize (layers.py:624-670)."""

    def __init__(self, in_dim, out_dim, kernel_size=3, padding=1, residual=False, conv_block=True,
                 interp_mode="bilinear", interp_size=None, activation_type="silu", dropout=0.1, debug=False):
        super().__init__()
        self.activation = _act_module(activation_type)
        self.dropout = nn.Dropout(dropout)
        if conv_block:
            self.conv = nn.Sequential(
                Conv2dResBlock(in_dim, out_dim, kernel_size=kernel_size, padding=padding, residual=residual,
                               dropout=dropout, activation_type=default(activation_type, "silu")),
                self.dropout, self.activation)
        self.conv_block = conv_block
        self.interp_size = interp_size
        self.interp_mode = interp_mode
        self.debug = debug

    def features_nhwc(self) -> bool:
        """True when the conv block runs channels-last on the implicit-GEMM convolution (ops.conv3x3_nhwc): the
        intermediate feature map is then (B, H1, W1, C) and no layout change happens anywhere in the scaler."""
        return (self.conv_block and self.interp_mode == "bilinear" and self.conv[0].plain()
                and ops.conv3x3_nhwc_ok(self.conv[0].conv[0]))

    def forward_features(self, x, in_nhwc=False, out_nhwc=False, want_factor=False):
        """Everything but the final resize, at the intermediate size: (B, C, H1, W1) channels-first, or (B, H1, W1, C)
        with ``out_nhwc`` (only when ``features_nhwc()``).
        ``want_factor``: returns (features, fac-or-None).  With a tensor in the second place the two SiLUs behind the
        convolution ran on its epilogue (ops.conv3x3_nhwc(act2=True): dropouts off, channels-last) and the caller MUST be
        the only consumer of the features and multiply their gradient by ``fac`` (ops.upsample_fc(in_factor=fac))."""
        if want_factor:
            return self._features(x, in_nhwc, out_nhwc, True)
        return self._features(x, in_nhwc, out_nhwc, False)[0]

    def _features(self, x, in_nhwc, out_nhwc, may_fuse):
        if self.interp_mode != "bilinear":
            raise NotImplementedError(f"interp_mode={self.interp_mode!r}: only bilinear has a HIP path")
        if out_nhwc and not self.features_nhwc():
            raise ValueError("Interp2dUpsample: channels-last features need the implicit-GEMM conv block")
        x = _resize(x, self.interp_size[0], None, in_nhwc=in_nhwc, out_nhwc=out_nhwc)
        if self.conv_block:
            blk = self.conv[0]
            if blk.plain():       # conv -> drop -> act -> drop -> act: the four elementwise stages in one pass
                no_drop = not self.training or (blk.conv[1].p == 0 and self.dropout.p == 0)
                if (may_fuse and out_nhwc and no_drop and _fuse_act2[0] and ops.conv3x3_nhwc_implicit(x)
                        and _act_name(blk.activation) == "silu" and _act_name(self.activation) == "silu"):
                    return ops.conv3x3_nhwc(x, blk.conv[0].weight, act2=True)       # ... or on the product's epilogue
                y = ops.conv3x3_nhwc(x, blk.conv[0].weight) if out_nhwc else blk.conv[0](x)
                x = ops.drop_act(y, blk.conv[1].p, _act_name(blk.activation), self.training,
                                 self.dropout.p, _act_name(self.activation))
            else:
                x = ops.drop_act(blk(x), self.dropout.p, _act_name(self.activation), self.training)
        return x, None

    def forward(self, x, in_nhwc=False, out_nhwc=False):
        """x (B, C, H, W), or (B, H, W, C) with ``in_nhwc``; the layout changes ride on the resizes."""
        mid = self.features_nhwc()
        return _resize(self.forward_features(x, in_nhwc, mid), self.interp_size[1], None, in_nhwc=mid,
                       out_nhwc=out_nhwc)


# --------------------------------------------------------------------------------------- attention (HIP)
class SimpleAttention(nn.Module):
    """Softmax-free attention with per-head LayerNorm and coordinate concatenation.

    Same parameters / state_dict keys as the reference (layers.py:793-828): ``linears.{0,1,2}``,
    ``norm_K.{i}``, ``norm_V.{i}`` (galerkin) or ``norm_Q.{i}`` (fourier, softmax), ``fc``.  The HIP path covers
    self-attention (query is key is value) and cross-attention (below) of the 'galerkin', 'linear' / 'global', 'fourier'
    ('integral', 'local') and 'softmax' types with norm_type='layer', and the Galerkin family with norm_type='instance': ``norm_K`` / ``norm_V`` are then
    ``nn.InstanceNorm1d(d_k, affine=True)`` per head (same keys and shapes, no buffers) and K, V are normalised over the
    tokens, one mean and variance per (sample, head, channel), before the coordinates are concatenated (layers.py:842-854).
    'softmax' (scaled dot-product attention, the dropout mask on the softmax output; fp32 arithmetic in every precision
    mode) needs coordinates: head tiles of width round4(d_k + pos_dim) in {20, 36, 52, 68, 100}, i.e. d_k in (16, 32, 48, 64,
    96) with pos_dim >= 1 (the shipped ex1 configuration, d_model 96 / one head, is the 100-wide one); the coordinate-free call (``pos is None`` or ``pos_dim == 0``) raises NotImplementedError.
    'fourier' with ``need_weights=False`` is fused (no n x n matrix in HBM) at the same five head-tile widths in every
    precision mode: the two-term fp16 kernel in the default arithmetic, the fp32-MFMA kernel (gt_fourier_attn, and
    gt_fourier_attn_wide at 68 / 100) under ``set_precision('f32')`` and the bf16 modes; other widths materialise.
    Cross-attention: ``forward(query, key, value, pos)`` with the three not one tensor (fused_forward_cross,
    ops.cross_attention) projects query [B, n_q, d] through linears[0] and key, value [B, n_kv, d] through linears[1], [2].
    The Galerkin family takes any n_q, n_kv without coordinates (with ``pos`` the same coordinates go to all three, so the
    counts are equal) and divides K'^T V' -- a sum over the n_kv memory tokens -- by n_q, as the reference does
    (layers.py:719, 728); fourier / softmax need n_q == n_kv (NotImplementedError otherwise).  Unequal key / value token
    counts, unequal batch sizes and ``pos`` with n_q != n_kv are AssertionErrors.
    'causal' (causal linear attention, reference layers.py:736-762; fp32 arithmetic in every precision mode, linear in n):
    with k^_j = keep_j K'_j / n and v^_j = keep_j V'_j, head output i is (sum_{j<=i} k^_j v^_j^T)^T Q'_i divided by
    (sum_{j<=i} k^_j + 1e-7) . Q'_i; ``norm_Q`` / ``norm_K`` as for fourier.  Head tiles round4(d_k + pos_dim) in {16, 32, 48,
    64, 96} (no coordinates) or {20, 36, 52, 68, 100}; self-attention and (query, key, value) with n_q == n_kv
    (AssertionError otherwise).  Three deviations from the reference, whose call sites of this kind do not run
    (INTEGRATION.md): ``mask`` is handed to the core as its ``kv_mask`` -- a torch.bool tensor [B, n_kv], True = keep, None
    keeps every token, not unsqueezed; anything else is a TypeError / AssertionError before a launch.  The reference's
    F.dropout(p = 0.5) acts on the [B, h, n, D, D] running state, which never exists here: no attention dropout is drawn,
    set_attention_dropout is not consulted, and ``attn_weight`` is None.  The operator is only as well-conditioned as its
    denominators (a sum of signed terms).
    Other variants of the reference are baselines outside the hot path."""

    def __init__(self, n_head, d_model, pos_dim: int = 1, attention_type="fourier", dropout=0.1,
                 xavier_init=1e-4, diagonal_weight=1e-2, symmetric_init=False, norm=False,
                 norm_type="layer", eps=1e-5, debug=False):
        super().__init__()
        assert d_model % n_head == 0
        self.attention_type = attention_type
        self.d_k = d_model // n_head
        self.n_head = n_head
        self.pos_dim = pos_dim
        self.linears = nn.ModuleList([nn.Linear(d_model, d_model) for _ in range(3)])
        self.xavier_init = xavier_init
        self.diagonal_weight = diagonal_weight
        self.symmetric_init = symmetric_init
        if self.xavier_init > 0:
            self._reset_parameters()
        self.add_norm = norm
        self.norm_type = norm_type
        self.eps = eps
        if norm:
            self._get_norm(eps=eps)
        if pos_dim > 0:
            self.fc = nn.Linear(d_model + n_head * pos_dim, d_model)
        self.attn_weight = None
        self.dropout = nn.Dropout(dropout)
        self.debug = debug

    # -- init contract of the reference (layers.py:901-913)
    def _reset_parameters(self):
        for param in self.linears.parameters():
            if param.ndim > 1:
                xavier_uniform_(param, gain=self.xavier_init)
                if self.diagonal_weight > 0.0:
                    param.data += self.diagonal_weight * torch.eye(param.size(-1), dtype=torch.float)
                if self.symmetric_init:
                    param.data += param.data.T
            else:
                constant_(param, 0)

    def _get_norm(self, eps):
        if self.norm_type == "instance":
            if self.attention_type not in _LINEAR_FAMILY:
                # layers.py:867 assigns the transposed VALUE to `query`; the coordinate concatenation then fails on the sizes
                raise NotImplementedError(f"norm_type='instance' with attention_type={self.attention_type!r}: that branch of "
                                          "the reference does not run (layers.py:867 mixes up query and value), so there "
                                          "are no semantics to match; 'instance' covers galerkin / linear / global")
            mk = lambda: nn.ModuleList([nn.InstanceNorm1d(self.d_k, eps=eps, affine=True) for _ in range(self.n_head)])
        elif self.norm_type == "layer":
            mk = lambda: nn.ModuleList([nn.LayerNorm(self.d_k, eps=eps) for _ in range(self.n_head)])
        else:
            raise NotImplementedError(f"norm_type={self.norm_type!r}: 'layer' and 'instance' have a HIP path")
        self.norm_K = mk()
        if self.attention_type in _LINEAR_FAMILY:
            self.norm_V = mk()
        else:
            self.norm_Q = mk()

    def _norm_pair(self):
        if self.attention_type in _LINEAR_FAMILY:
            return self.norm_K, self.norm_V, 0b110
        return self.norm_Q, self.norm_K, 0b011

    def _pack_groups(self):
        """The parameter lists _packed() concatenates, in concatenation order (optim.FlatClipAdam(model=...) lays each
        group out contiguously, and ops.packed_params then returns views instead of copies)."""
        groups = [[l.weight for l in self.linears]]
        if all(l.bias is not None for l in self.linears):
            groups.append([l.bias for l in self.linears])
        if self.add_norm:
            first, second, _ = self._norm_pair()
            groups.append([m.weight for m in first] + [m.weight for m in second])
            groups.append([m.bias for m in first] + [m.bias for m in second])
        return groups

    def _packed(self):
        wqkv = ops.packed_params([l.weight for l in self.linears])
        bqkv = ops.packed_params([l.bias for l in self.linears])
        gamma = beta = None
        mask = 0
        if self.add_norm:
            first, second, mask = self._norm_pair()
            gamma = ops.packed_params([m.weight for m in first] + [m.weight for m in second])
            beta = ops.packed_params([m.bias for m in first] + [m.bias for m in second])
            gamma = gamma.view(2, self.n_head, self.d_k)
            beta = beta.view(2, self.n_head, self.d_k)
        return wqkv, bqkv, gamma, beta, mask

    def _operator_args(self, pos, device):
        """What the self- and the cross-attention operator share: the checks of the attention type, then
        (pos or None, wfc, bfc, kind)."""
        if self.attention_type in _SOFTMAX_ATTENTION and (pos is None or self.pos_dim == 0):
            raise NotImplementedError("attention_type='softmax' without coordinates is outside the HIP hot path: the softmax "
                                      "kernels take head tiles of width 16*k + 4 (d_k in (16, 32, 48, 64, 96) plus pos_dim >= 1)")
        if self.attention_type not in _HIP_ATTENTION + _SOFTMAX_ATTENTION + _CAUSAL_ATTENTION:
            raise NotImplementedError(f"attention_type={self.attention_type!r} is outside the HIP hot path "
                                      "(galerkin / fourier / linear / softmax / causal only)")
        use_pos = pos is not None and self.pos_dim > 0
        if use_pos:
            assert pos.size(-1) == self.pos_dim
            wfc, bfc = self.fc.weight, self.fc.bias
        else:
            # reference layers.py:869-874, 894-897: without coordinates the heads are not widened and `fc` is skipped --
            # the same operator with zero coordinate columns and the identity in fc's place
            pos = None
            d = self.n_head * self.d_k
            key = (device, d)
            if getattr(self, "_eye", (None, None))[0] != key:
                self._eye = (key, torch.eye(d, dtype=torch.float32, device=device))
            wfc, bfc = self._eye[1], None
        if self.attention_type == "galerkin":
            kind = "galerkin"
        elif self.attention_type in ("linear", "global"):     # the reference treats the two names alike (layers.py:719)
            kind = "linear"
        elif self.attention_type in _SOFTMAX_ATTENTION:
            kind = "softmax"
        elif self.attention_type in _CAUSAL_ATTENTION:
            kind = "causal"
            # the width refusal needs no device: NotImplementedError("... no kernel ...") before anything else happens
            H.causal_check(H.round4(self.d_k + (self.pos_dim if use_pos else 0)))
        else:
            kind = "fourier"
        return pos, wfc, bfc, kind

    def fused_forward(self, x, pos=None, residual=None, sign=1.0, p_out=0.0, need_weights=True, kv_mask=None):
        """res + sign*dropout(attention(x)); the encoder layer's entry point.  ``need_weights=False`` lets the
        Fourier and softmax types run fused (no n x n matrix in HBM; the returned weight is None).  ``kv_mask``: the
        causal type's key / value mask (torch.bool [B, n], True = keep)."""
        return self._fused(ops.simple_attention, (x,), x, pos, kv_mask, residual, sign, p_out, need_weights)

    def fused_forward_cross(self, query, key, value, pos=None, residual=None, sign=1.0, p_out=0.0, need_weights=True,
                            kv_mask=None):
        """The same for query [B, n_q, d], key and value [B, n_kv, d] that are not one tensor (ops.cross_attention):
        res + sign*dropout(attention(query, key, value)) with ``residual`` = ``query`` or None.  Shape contracts are
        AssertionErrors, raised before anything is launched."""
        ops.check_cross_shapes(query, key, value, pos if self.pos_dim > 0 else None)
        return self._fused(ops.cross_attention, (query, key, value), key, pos, kv_mask, residual, sign, p_out, need_weights)

    def _fused(self, operator, inputs, key, pos, kv_mask, residual, sign, p_out, need_weights):
        """fused_forward / fused_forward_cross behind their own checks: ``operator`` (ops.simple_attention or
        ops.cross_attention) on ``inputs`` with this module's packed parameters; ``key`` is what ``kv_mask`` masks."""
        pos, wfc, bfc, kind = self._operator_args(pos, inputs[0].device)
        keep = self._keep_vector(kv_mask, key)
        wqkv, bqkv, gamma, beta, mask = self._packed()
        out, w = operator(*inputs, pos, wqkv, bqkv, gamma, beta, wfc, bfc,
                          kind=kind, n_head=self.n_head, norm_mask=mask, eps=self.eps,
                          res=residual, sign=sign, p_out=p_out, need_weights=need_weights,
                          token_norm=self.add_norm and self.norm_type == "instance", keep=keep)
        self.attn_weight = w
        return out, w

    def _keep_vector(self, kv_mask, key):
        """The causal type's ``mask`` -> the kernels' keep vector [B, n_kv] (uint8) or None; the checks of ops.check_kv_mask."""
        if kv_mask is None:
            return None
        if self.attention_type not in _CAUSAL_ATTENTION:
            raise ValueError("kv_mask is the key / value mask of attention_type='causal'")
        return ops.check_kv_mask(kv_mask, key.size(0), key.size(1))

    def forward(self, query, key, value, pos=None, mask=None, weight=None):
        if self.attention_type in _CAUSAL_ATTENTION:
            # (the reference's call passes mask= to a function that takes kv_mask=, and asserts a mask is given: INTEGRATION.md)
            if weight is not None:
                raise NotImplementedError("weighted attention is outside the HIP hot path")
            if not (query is key and key is value):
                return self.fused_forward_cross(query, key, value, pos, kv_mask=mask)
            return self.fused_forward(query, pos, kv_mask=mask)
        if mask is not None:
            if self.attention_type in _LINEAR_FAMILY:
                raise RuntimeError("linear attention does not support casual mask.")
            raise NotImplementedError("attention masks are outside the HIP hot path")
        if weight is not None:
            raise NotImplementedError("weighted attention is outside the HIP hot path")
        if not (query is key and key is value):
            return self.fused_forward_cross(query, key, value, pos)
        return self.fused_forward(query, pos)


class FeedForward(nn.Module):
    """lr1 -> act -> dropout -> [BatchNorm1d] -> lr2 (layers.py:954-987); one fused HIP operator.

    batch_norm=True puts nn.BatchNorm1d(dim_feedforward) (the reference's `bn`, same state_dict keys) between the hidden
    dropout and lr2: one mean and one biased variance per hidden channel over all B n token rows, on the gt_batchnorm_*
    kernels (ops.feed_forward_bn).  In training mode the batch statistics are used and `running_mean`, `running_var` and
    `num_batches_tracked` are updated on the device; in eval mode the running buffers are the statistics.  Under
    data-parallel training every rank keeps its own statistics and buffers (torch's behaviour without SyncBatchNorm).
    Not implemented, and raising NotImplementedError: activation='gelu' together with batch_norm, a `bn` changed to
    momentum=None, affine=False or track_running_stats=False (none reachable from this constructor), and a hidden width
    that is no multiple of 4."""

    def __init__(self, in_dim=256, dim_feedforward: int = 1024, out_dim=None, batch_norm=False,
                 activation="relu", dropout=0.1):
        super().__init__()
        out_dim = default(out_dim, in_dim)
        self.lr1 = nn.Linear(in_dim, dim_feedforward)
        if activation == "silu":
            self.activation = nn.SiLU()
        elif activation == "gelu":
            self.activation = nn.GELU()
        else:
            self.activation = nn.ReLU()
        self.batch_norm = batch_norm
        if batch_norm:
            self.bn = nn.BatchNorm1d(dim_feedforward)
        self.lr2 = nn.Linear(dim_feedforward, out_dim)
        self.dropout = nn.Dropout(dropout)

    def _fused_forward_bn(self, x, residual, p_h, p_out):
        bn = self.bn
        if bn.momentum is None or not bn.affine or not bn.track_running_stats:
            # a cumulative average (momentum=None) needs the step counter on the host; the other two have no kernel
            raise NotImplementedError("batch_norm=True on the HIP path needs BatchNorm1d with a momentum, affine=True and "
                                      "track_running_stats=True")
        if isinstance(self.activation, nn.GELU):
            raise NotImplementedError("batch_norm=True with activation='gelu' is outside the HIP hot path")
        try:
            out = ops.feed_forward_bn(x, self.lr1.weight, self.lr1.bias, self.lr2.weight, self.lr2.bias, bn.weight, bn.bias,
                                      bn.running_mean, bn.running_var, res=residual, act=_act_name(self.activation),
                                      p_h=p_h, p_out=p_out, eps=bn.eps, momentum=bn.momentum, training=bn.training)
        except H.GtNotSupported as e:
            raise NotImplementedError(f"batch_norm=True: no HIP kernel for dim_feedforward={self.lr1.out_features} "
                                      f"(a multiple of 4 is needed): {e}") from e
        if bn.training:
            bn.num_batches_tracked.add_(1)      # on the device: no host read-back, capturable in a HIP graph
        return out

    def fused_forward(self, x, residual=None, p_out=0.0):
        p_h = self.dropout.p if self.training else 0.0
        if self.batch_norm:
            return self._fused_forward_bn(x, residual, p_h, p_out)
        if isinstance(self.activation, nn.GELU):
            # activation='gelu' (reference layers.py:968; no config selects it): the two GEMMs with the erf GELU and its
            # dropout as one elementwise pass between them -- the GEMM epilogues carry relu / silu only
            hid = ops.drop_act(ops.linear(x, self.lr1.weight, self.lr1.bias), 0.0, _act_name(self.activation),
                               training=True, p2=p_h)
            y = ops.linear(hid, self.lr2.weight, self.lr2.bias, p_drop=p_out)
            return y if residual is None else residual + y
        return ops.feed_forward(x, self.lr1.weight, self.lr1.bias, self.lr2.weight, self.lr2.bias,
                                res=residual, act=_act_name(self.activation), p_h=p_h, p_out=p_out)

    def forward(self, x):
        return self.fused_forward(x)


# --------------------------------------------------------------------------------------- spectral convs (HIP)
class SpectralConv1d(nn.Module):
    def __init__(self, in_dim, out_dim, modes: int, n_grid=None, dropout=0.1, return_freq=False,
                 activation="silu", debug=False):
        super().__init__()
        self.linear = nn.Linear(in_dim, out_dim)
        self.modes = modes
        self.activation = _act_module(activation)
        self.n_grid = n_grid
        self.fourier_weight = Parameter(torch.empty(in_dim, out_dim, modes, 2))
        xavier_normal_(self.fourier_weight, gain=1 / (in_dim * out_dim))
        self.dropout = nn.Dropout(dropout)
        self.return_freq = return_freq
        self.debug = debug

    def forward(self, x):
        act = _act_name(self.activation)
        args = (self.linear.weight, self.linear.bias, self.fourier_weight, self.modes)
        if self.training and self.dropout.p > 0:
            # the reference drops the input of the FFT branch only (layers.py:1083-1084: res = linear(x); x = dropout(x)).
            # By linearity  spec(xs) + lin(x) = [spec(xs) + lin(xs)] + lin(x - xs): the fused operator on the dropped input
            # plus one pointwise Linear on the difference (p is 0 in every shipped config)
            xs = ops.dropout(x, self.dropout.p, True)
            pre = spectral.spectral_conv1d(xs, *args, "none", return_freq=self.return_freq)
            pre, ft = pre if self.return_freq else (pre, None)
            y = self.activation(pre + ops.linear(x - xs, self.linear.weight, None))
            return (y, ft) if self.return_freq else y
        return spectral.spectral_conv1d(x, *args, act, return_freq=self.return_freq)


class SpectralConv2d(nn.Module):
    def __init__(self, in_dim, out_dim, modes: int, n_grid=None, dropout=0.1, norm="ortho",
                 activation="silu", return_freq=False, debug=False):
        super().__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.linear = nn.Linear(in_dim, out_dim)
        self.modes = modes
        self.activation = _act_module(activation)
        self.n_grid = n_grid
        self.fourier_weight = nn.ParameterList(
            [Parameter(torch.empty(in_dim, out_dim, modes, modes, 2)) for _ in range(2)])
        for param in self.fourier_weight:
            xavier_normal_(param, gain=1 / (in_dim * out_dim) * np.sqrt(in_dim + out_dim))
        self.dropout = nn.Dropout(dropout)
        self.norm = norm
        self.return_freq = return_freq
        self.debug = debug

    def forward(self, x):
        if x.ndim == 4:
            n = x.size(1)
            assert x.size(1) == x.size(2)
        elif x.ndim == 3:
            n = int(x.size(1) ** 0.5)
        else:
            raise ValueError("Dimension not implemented")
        if self.norm != "ortho":
            raise NotImplementedError("only norm='ortho' (the reference default) has a HIP path")
        B, flat = x.size(0), x.ndim == 3
        h = x.reshape(B, n, n, self.in_dim)
        args = (self.linear.weight, self.linear.bias, self.fourier_weight[0], self.fourier_weight[1], self.modes)
        ft = None
        if self.training and self.dropout.p > 0:
            # dropout on the input of the FFT branch only (layers.py:1172-1173); see SpectralConv1d.forward
            hs = ops.dropout(h, self.dropout.p, True)
            pre = spectral.spectral_conv2d(hs, *args, "none", return_freq=self.return_freq)
            pre, ft = pre if self.return_freq else (pre, None)
            y = self.activation(pre + ops.linear(h - hs, self.linear.weight, None))
        else:
            y = spectral.spectral_conv2d(h, *args, _act_name(self.activation), return_freq=self.return_freq)
            y, ft = y if self.return_freq else (y, None)
        y = y.reshape(B, n * n, self.out_dim) if flat else y
        return (y, ft) if self.return_freq else y


# --------------------------------------------------------------------------------------- random-feature attention (HIP)
def _orthogonal_random_matrix(rows: int, columns: int, device, generator=None) -> torch.Tensor:
    """[rows, columns] in blocks of ``rows`` columns: each block is the Q factor of a Gaussian [rows, rows] matrix with
    column c scaled by the norm of the Gaussian's row c (norms distributed like those of N(0, I) vectors).  The QR runs on
    ``device`` when its solver library is available, else on the host."""
    w = torch.zeros(rows, columns, device=device)
    for start in range(0, columns, rows):
        end = min(start + rows, columns)
        block = torch.randn(rows, rows, device=device, generator=generator)
        norms = block.pow(2).sum(1).sqrt()
        try:
            q, _ = torch.linalg.qr(block)
        except RuntimeError:                 # no device QR in this build: the draw is plumbing, the host does it
            q = torch.linalg.qr(block.cpu())[0].to(device)
        w[:, start:end] = q[:, :end - start] * norms[None, :end - start]
    return w


class RandomFourierFeatures(nn.Module):
    """phi(x) = sqrt(2 / n_dims) [cos u, sin u], u = (x d^(-1/4)) omega: random Fourier features of the Gaussian kernel
    (reference examples/ex1_burgers_random_fourier_features.py:84-148), ``omega`` [query_dimensions, n_dims // 2] a buffer.

    ``new_feature_map`` redraws ``omega`` (standard normal; block-orthogonal with ``orthogonal=True``) unless
    ``deterministic_eval`` is set in eval mode, as the reference does, or the attribute ``redraw`` is False (tests, captured
    training steps).  The Gaussian redraw can be part of a captured graph; the orthogonal one (a QR) cannot.  The attention
    modules never call ``forward``: the fused kernels evaluate phi in registers; it is the definition in torch, for
    comparisons."""
    kind = "rfa"

    def __init__(self, query_dimensions, n_dims=None, orthogonal=False, deterministic_eval=False):
        super().__init__()
        self.n_dims = n_dims or query_dimensions
        self.query_dims = self.query_dimensions = query_dimensions
        self.orthogonal = orthogonal
        self.softmax_temp = 1 / math.sqrt(query_dimensions)
        self.deterministic_eval = deterministic_eval
        self.redraw = True
        self.register_buffer("omega", torch.zeros(self.query_dimensions, self.n_dims // 2))

    @classmethod
    def factory(cls, *args, **kwargs):
        def inner(query_dims):
            return cls(query_dims, *args, **kwargs)
        return inner

    def new_feature_map(self, device):
        if (self.deterministic_eval and not self.training) or not self.redraw:
            return
        rows, cols = self.query_dimensions, self.n_dims // 2
        if self.orthogonal:
            self.omega = _orthogonal_random_matrix(rows, cols, device)
        else:
            self.omega = torch.randn(rows, cols, device=device)

    def _u(self, x):
        return (x * math.sqrt(self.softmax_temp)) @ self.omega

    def forward(self, x):
        u = self._u(x)
        return torch.cat([torch.cos(u), torch.sin(u)], dim=-1) * math.sqrt(2 / self.n_dims)


class Favor(RandomFourierFeatures):
    """phi(x) = [exp(u - c), exp(-u - c)], c = |x d^(-1/4)|^2 / 2 + log(n_dims) / 2: the positive orthogonal random features
    of the Performer (reference example :151-205)."""
    kind = "favor"

    def __init__(self, query_dimensions, n_dims=None, orthogonal=True, deterministic_eval=False):
        super().__init__(query_dimensions, n_dims=n_dims, orthogonal=orthogonal, deterministic_eval=deterministic_eval)

    def forward(self, x):
        u = self._u(x)
        c = 0.5 * self.softmax_temp * x.pow(2).sum(-1, keepdim=True) + 0.5 * math.log(self.n_dims)
        return torch.cat([torch.exp(u - c), torch.exp(-u - c)], dim=-1)


class RandomFourierAttention(nn.Module):
    """Linear-complexity attention through a random feature map (reference example :208-318), ONE head:
    out_projection([phi(Q) (phi(K)^T V) / (phi(Q) . sum phi(K) + eps), pos]) on the gt_rfattn_* kernels
    (ops.random_feature_attention).  ``attention_type``: 'favor' (Performer) or 'rfa'.

    The reference builds its feature map for d_model inputs and applies it to d_model / n_heads wide heads, so it only runs
    with n_heads == 1: any other value is a ValueError here.  d_model outside (32, 64, 96) has no kernel
    (NotImplementedError), ``pos`` is required (ValueError), and query, key and value must be one tensor.  ``omega`` is redrawn
    at every forward (see RandomFourierFeatures; ``redraw = False`` on this module freezes it)."""

    def __init__(self, d_model, n_heads, pos_dim=1, eps=1e-6, attention_type='favor', xavier_init=1.0, diagonal_weight=0.0):
        super().__init__()
        if n_heads != 1:
            raise ValueError(f"RandomFourierAttention: n_heads={n_heads}: the feature map is built for d_model inputs, so the "
                             "attention is defined for one head only (n_heads=1)")
        H.rfattn_check(d_model, attention_type)
        f = Favor if attention_type == 'favor' else RandomFourierFeatures
        self.feature_map = f(d_model, n_dims=d_model)
        self.query_projection = nn.Linear(d_model, d_model)
        self.key_projection = nn.Linear(d_model, d_model)
        self.value_projection = nn.Linear(d_model, d_model)
        self.out_projection = nn.Linear(d_model + pos_dim, d_model)
        self.n_heads = n_heads
        self.eps = eps
        self.attention_type = attention_type
        self.xavier_init = xavier_init
        self.diagonal_weight = diagonal_weight
        for layer in [self.query_projection, self.key_projection, self.value_projection]:
            self._reset_parameters(layer)

    def _reset_parameters(self, layer):
        for param in layer.parameters():
            if param.ndim > 1:
                xavier_uniform_(param, gain=self.xavier_init)
                if self.diagonal_weight > 0.0:
                    param.data += self.diagonal_weight * torch.diag(torch.ones(param.size(-1), dtype=torch.float))
            else:
                constant_(param, 0)

    @property
    def redraw(self) -> bool:
        return self.feature_map.redraw

    @redraw.setter
    def redraw(self, flag: bool):
        self.feature_map.redraw = bool(flag)

    def fused_forward(self, x, pos, residual=None, p_out=0.0):
        if pos is None:
            raise ValueError("RandomFourierAttention: `pos` is required (it is concatenated in front of the output "
                             "projection unconditionally)")
        self.feature_map.new_feature_map(x.device)
        q, k, v = self.query_projection, self.key_projection, self.value_projection
        wqkv = ops.packed_params([q.weight, k.weight, v.weight])
        bqkv = ops.packed_params([q.bias, k.bias, v.bias])
        return ops.random_feature_attention(x, pos, wqkv, bqkv, self.feature_map.omega, self.out_projection.weight,
                                            self.out_projection.bias, kind=self.feature_map.kind, eps=self.eps,
                                            res=residual, p_out=p_out)

    def forward(self, queries, keys=None, values=None, pos=None):
        keys = queries if keys is None else keys
        values = keys if values is None else values
        if keys is not queries or values is not queries:
            raise NotImplementedError("RandomFourierAttention: queries, keys and values must be one tensor (self-attention)")
        return self.fused_forward(queries, pos)
