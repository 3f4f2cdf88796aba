"""Model assembly with the reference's module API (reference: libs/model.py): same class names,
constructor keywords / config keys, forward signatures, return dicts and state_dict keys, so that
released checkpoints load and ``examples/ex{1,2,3}*.py`` run unchanged.  The encoder layers and
the spectral / pointwise decoders run on the HIP operators of ``ops`` / ``spectral``.
"""
from __future__ import annotations

import copy
import os
import sys
from collections import defaultdict

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, xavier_uniform_

from . import _hip as H
from . import ops
from .layers import (Conv2dEncoder, DeConv2dBlock, EdgeEncoder, FeedForward, GraphAttention, GraphConvolution, Identity, Interp2dEncoder,
                     Interp2dUpsample, PositionalEncoding, RandomFourierAttention, SimpleAttention, SpectralConv1d, SpectralConv2d, _act_module,
                     _act_name, default)

current_path = os.path.dirname(os.path.abspath(__file__))
SRC_ROOT = os.path.dirname(current_path)

ADDITIONAL_ATTR = ['normalizer', 'raw_laplacian', 'return_latent', 'residual_type', 'norm_type',
                   'norm_eps', 'boundary_condition', 'upscaler_size', 'downscaler_size', 'spacial_dim',
                   'spacial_fc', 'regressor_activation', 'attn_activation', 'downscaler_activation',
                   'upscaler_activation', 'encoder_dropout', 'decoder_dropout', 'ffn_dropout']


class SimpleTransformerEncoderLayer(nn.Module):
    """x <- x +/- drop(attn(x)); [LN]; x <- x + drop(ff(x)); [LN]      (reference model.py:33-140).

    batch_norm=True gives the FeedForward an nn.BatchNorm1d(dim_feedforward) behind its hidden dropout (FeedForward's
    docstring: batch statistics and running buffers per rank, relu / silu only)."""

    def __init__(self, d_model=96, pos_dim=1, n_head=2, dim_feedforward=512, attention_type='fourier',
                 pos_emb=False, layer_norm=True, attn_norm=None, norm_type='layer', norm_eps=None,
                 batch_norm=False, attn_weight=False, xavier_init: float = 1e-2,
                 diagonal_weight: float = 1e-2, symmetric_init=False, residual_type='add',
                 activation_type='relu', dropout=0.1, ffn_dropout=None, debug=False):
        super().__init__()
        dropout = default(dropout, 0.05)
        if attention_type in ['linear', 'softmax']:
            dropout = 0.1
        ffn_dropout = default(ffn_dropout, dropout)
        norm_eps = default(norm_eps, 1e-5)
        attn_norm = default(attn_norm, not layer_norm)
        if (not layer_norm) and (not attn_norm):
            attn_norm = True
        norm_type = default(norm_type, 'layer')
        self.attn = SimpleAttention(n_head=n_head, d_model=d_model, attention_type=attention_type,
                                    diagonal_weight=diagonal_weight, xavier_init=xavier_init,
                                    symmetric_init=symmetric_init, pos_dim=pos_dim, norm=attn_norm,
                                    norm_type=norm_type, eps=norm_eps, dropout=dropout)
        self.d_model = d_model
        self.n_head = n_head
        self.pos_dim = pos_dim
        self.add_layer_norm = layer_norm
        self.norm_eps = norm_eps
        if layer_norm:
            self.layer_norm1 = nn.LayerNorm(d_model, eps=norm_eps)
            self.layer_norm2 = nn.LayerNorm(d_model, eps=norm_eps)
        dim_feedforward = default(dim_feedforward, 2 * d_model)
        self.ff = FeedForward(in_dim=d_model, dim_feedforward=dim_feedforward, batch_norm=batch_norm,
                              activation=activation_type, dropout=ffn_dropout)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.residual_type = residual_type
        self.add_pos_emb = pos_emb
        if self.add_pos_emb:
            self.pos_emb = PositionalEncoding(d_model)
        self.debug = debug
        self.attn_weight = attn_weight
        self.__name__ = attention_type.capitalize() + 'TransformerEncoderLayer'

    def forward(self, x, pos=None, weight=None):
        if weight is not None:
            raise NotImplementedError("weighted attention is outside the HIP hot path")
        if self.add_pos_emb:
            x = self.pos_emb(x)
        sign = 1.0 if (self.residual_type in ['add', 'plus'] or self.residual_type is None) else -1.0
        p1 = self.dropout1.p if self.training else 0.0
        p2 = self.dropout2.p if self.training else 0.0
        x, attn_weight = self.attn.fused_forward(x, pos, residual=x, sign=sign, p_out=p1,
                                                 need_weights=bool(self.attn_weight))
        if self.add_layer_norm:
            x = ops.layer_norm(x, self.layer_norm1.weight, self.layer_norm1.bias, self.norm_eps)
        x = self.ff.fused_forward(x, residual=x, p_out=p2)
        if self.add_layer_norm:
            x = ops.layer_norm(x, self.layer_norm2.weight, self.layer_norm2.bias, self.norm_eps)
        return (x, attn_weight) if self.attn_weight else x


# the reference's README / eval notebooks still use the pre-rename class name
FourierTransformerEncoderLayer = SimpleTransformerEncoderLayer


class _TransformerEncoderLayer(nn.Module):
    """The classic post-LN Transformer encoder layer around nn.MultiheadAttention, batch first (reference model.py:244-322):
        src <- [norm1](src + drop1(out_proj(attention(src))));  src <- [norm2](src + drop2(linear2(drop(relu(linear1(src))))))
    with P = softmax(q k^T / sqrt(d_k)) and the module's own dropout on P in training.  Parameters, state_dict keys and
    initialisation are the reference's (self_attn.in_proj_weight / in_proj_bias / out_proj.*, linear1, linear2, norm1,
    norm2; both norms exist even with layer_norm=False).  ``self_attn`` only holds the parameters: its forward is never
    called, the attention runs on ops.multihead_attention (tail-free fused softmax kernels; the materialised route with
    attn_weight=True, which returns the head mean of the dropped-out P, detached).

    forward(src, pos=None, weight=None, src_mask=None, src_key_padding_mask=None): ``pos`` is concatenated in FRONT of
    src and the width must then be d_model (AssertionError otherwise, as torch's); ``weight`` is ignored, as in the
    reference; the reference uses the masks only when both are given -- that raises NotImplementedError here, one alone is
    ignored.  set_attention_dropout does not act on this layer."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, layer_norm=True, attn_weight=False):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.add_layer_norm = layer_norm
        self.attn_weight = attn_weight
        self.activation = nn.ReLU()

    def _pack_groups(self):
        return []       # in_proj_weight / in_proj_bias are packed parameters already

    def forward(self, src, pos=None, weight=None, src_mask=None, src_key_padding_mask=None):
        if pos is not None:
            src = torch.cat([pos, src], dim=-1)
        mha = self.self_attn
        assert src.size(-1) == mha.embed_dim, \
            f"was expecting embedding dimension of {mha.embed_dim}, but got {src.size(-1)}"
        if src_mask is not None and src_key_padding_mask is not None:
            raise NotImplementedError("attention masks are outside the HIP hot path")
        train = self.training
        src, w = ops.multihead_attention(src, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                         n_head=mha.num_heads, p_attn=mha.dropout if train else 0.0, res=src,
                                         p_out=self.dropout1.p if train else 0.0, need_weights=bool(self.attn_weight))
        if self.add_layer_norm:
            src = ops.layer_norm(src, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        src = ops.feed_forward(src, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, res=src,
                               act="relu", p_h=self.dropout.p if train else 0.0, p_out=self.dropout2.p if train else 0.0)
        if self.add_layer_norm:
            src = ops.layer_norm(src, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        return (src, w) if self.attn_weight else src


class GalerkinTransformerDecoderLayer(nn.Module):
    """The decoder layer on causal linear attention (reference model.py:142-241), three post-LN blocks:
        x <- [norm1](x + drop1(self_attn(x, x, x, mask=tgt_mask)))
        x <- [norm2](x + drop2(multihead_attn(x, memory, memory, mask=memory_mask)))      attention_type='causal'
        x <- [norm3](x + drop(ff(x)))
    Constructor arguments, parameter names and shapes are the reference's: ``self_attn`` / ``multihead_attn`` (each with its
    ``fc``, which the coordinate-free calls never use), ``ff``, the unused ``linear2``, ``norm1..3`` only with ``layer_norm``.
    No ``pos`` is passed to either attention.  ``memory`` has as many tokens as ``x`` (AssertionError otherwise).

    The reference's forward does not run (its two attention calls raise TypeError, and the causal branch asserts a mask the
    decoder does not give); the repairs are SimpleAttention's (its docstring): ``memory_mask`` is the causal
    core's key / value mask, torch.bool [B, n] with True = keep, or None; ``tgt_mask`` goes to ``self_attn`` as ``mask`` --
    with the default 'galerkin' a mask that is not None raises the linear family's RuntimeError, with fourier / softmax
    NotImplementedError, with 'causal' it is that core's key / value mask; the causal core draws no attention dropout."""

    def __init__(self, d_model, nhead, pos_dim=1, dim_feedforward=512, attention_type='galerkin', layer_norm=True,
                 attn_norm=None, norm_type='layer', norm_eps=1e-5, xavier_init: float = 1e-2,
                 diagonal_weight: float = 1e-2, dropout=0.05, ffn_dropout=None, activation_type='relu', device=None,
                 dtype=None, debug=False):
        super().__init__()
        factory_kwargs = {'device': device, 'dtype': dtype}
        ffn_dropout = default(ffn_dropout, dropout)
        self.debug = debug
        attn = dict(pos_dim=pos_dim, norm=attn_norm, eps=norm_eps, norm_type=norm_type, diagonal_weight=diagonal_weight,
                    xavier_init=xavier_init, dropout=dropout)
        self.self_attn = SimpleAttention(nhead, d_model, attention_type=attention_type, **attn)
        self.multihead_attn = SimpleAttention(nhead, d_model, attention_type='causal', **attn)
        dim_feedforward = default(dim_feedforward, 2 * d_model)
        self.ff = FeedForward(in_dim=d_model, dim_feedforward=dim_feedforward, activation=activation_type,
                              dropout=ffn_dropout)
        self.dropout = nn.Dropout(ffn_dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model, **factory_kwargs)
        self.add_layer_norm = layer_norm
        self.norm_eps = norm_eps
        if self.add_layer_norm:
            self.norm1 = nn.LayerNorm(d_model, eps=norm_eps, **factory_kwargs)
            self.norm2 = nn.LayerNorm(d_model, eps=norm_eps, **factory_kwargs)
            self.norm3 = nn.LayerNorm(d_model, eps=norm_eps, **factory_kwargs)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.activation = F.relu

    def _norm(self, norm, x):
        return ops.layer_norm(x, norm.weight, norm.bias, self.norm_eps)

    def forward(self, x, memory, tgt_mask=None, memory_mask=None):
        train = self.training
        sa = self.self_attn
        if sa.attention_type == 'causal':
            x = sa.fused_forward(x, None, residual=x, p_out=self.dropout1.p if train else 0.0, kv_mask=tgt_mask)[0]
        else:
            if tgt_mask is not None:
                sa(x, x, x, mask=tgt_mask)      # the refusal of that attention type
            x = sa.fused_forward(x, None, residual=x, p_out=self.dropout1.p if train else 0.0, need_weights=False)[0]
        if self.add_layer_norm:
            x = self._norm(self.norm1, x)
        x = self.multihead_attn.fused_forward_cross(x, memory, memory, None, residual=x,
                                                    p_out=self.dropout2.p if train else 0.0, kv_mask=memory_mask)[0]
        if self.add_layer_norm:
            x = self._norm(self.norm2, x)
        x = self.ff.fused_forward(x, residual=x, p_out=self.dropout.p if train else 0.0)
        if self.add_layer_norm:
            x = self._norm(self.norm3, x)
        return x


class TransformerEncoderWrapper(nn.Module):
    """num_layers deep copies of an encoder layer, then ``norm`` if given (reference model.py:325-373)."""

    __constants__ = ['norm']

    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = norm

    def forward(self, src, mask=None, src_key_padding_mask=None):
        output = src
        for mod in self.layers:
            output = mod(output, src_mask=mask, src_key_padding_mask=src_key_padding_mask)
        if self.norm is not None:
            if isinstance(self.norm, nn.LayerNorm) and self.norm.elementwise_affine:
                output = ops.layer_norm(output, self.norm.weight, self.norm.bias, self.norm.eps)
            else:
                output = self.norm(output)
        return output


class PointwiseRegressor(nn.Module):
    """[fc(cat[x, grid])] -> num_layers x (Linear + act + dropout) -> Linear   (model.py:472-529)."""

    def __init__(self, in_dim, n_hidden, out_dim, num_layers: int = 2, spacial_fc: bool = False,
                 spacial_dim=1, dropout=0.1, activation='silu', return_latent=False, debug=False):
        super().__init__()
        dropout = default(dropout, 0.1)
        self.spacial_fc = spacial_fc
        activ = nn.SiLU() if activation == 'silu' else nn.ReLU()
        if self.spacial_fc:
            self.fc = nn.Linear(in_dim + spacial_dim, n_hidden)
        self.ff = nn.ModuleList([nn.Sequential(nn.Linear(n_hidden, n_hidden), activ)
                                 for _ in range(max(num_layers, 1))])
        self.dropout = nn.Dropout(dropout)
        self.out = nn.Linear(n_hidden, out_dim)
        self.return_latent = return_latent
        self.debug = debug

    def forward(self, x, grid=None):
        if self.spacial_fc:
            x = ops.linear(x, self.fc.weight, self.fc.bias, extra=grid)
        p = self.dropout.p if self.training else 0.0
        for layer in self.ff:
            x = ops.linear(x, layer[0].weight, layer[0].bias, act=_act_name(layer[1]), p_drop=p)
        x = ops.linear(x, self.out.weight, self.out.bias)
        return (x, None) if self.return_latent else x


class SpectralRegressor(nn.Module):
    """[fc(cat[x, grid])] -> N x SpectralConv -> Linear . act . Linear [-> un-normalise] (model.py:532-637)."""

    def __init__(self, in_dim, n_hidden, freq_dim, out_dim, modes: int, num_spectral_layers: int = 2,
                 n_grid=None, dim_feedforward=None, spacial_fc=False, spacial_dim=2, return_freq=False,
                 return_latent=False, normalizer=None, activation='silu', last_activation=True,
                 dropout=0.1, debug=False):
        super().__init__()
        if spacial_dim == 2:
            conv = SpectralConv2d
        elif spacial_dim == 1:
            conv = SpectralConv1d
        else:
            raise NotImplementedError("3D not implemented.")
        activation = default(activation, 'silu')
        self.activation = _act_module(activation)
        dropout = default(dropout, 0.1)
        self.spacial_fc = spacial_fc
        if self.spacial_fc:
            self.fc = nn.Linear(in_dim + spacial_dim, n_hidden)
        dims = [n_hidden] + [freq_dim] * num_spectral_layers
        self.spectral_conv = nn.ModuleList(
            [conv(in_dim=dims[j], out_dim=dims[j + 1], n_grid=n_grid, modes=modes, dropout=dropout,
                  activation=activation, return_freq=return_freq, debug=debug)
             for j in range(num_spectral_layers)])
        if not last_activation:
            self.spectral_conv[-1].activation = Identity()
        self.n_grid = n_grid
        self.dim_feedforward = default(dim_feedforward, 2 * spacial_dim * freq_dim)
        self.regressor = nn.Sequential(nn.Linear(freq_dim, self.dim_feedforward), self.activation,
                                       nn.Linear(self.dim_feedforward, out_dim))
        self.normalizer = normalizer
        self.return_freq = return_freq
        self.return_latent = return_latent
        self.debug = debug

    def forward(self, x, edge=None, pos=None, grid=None, upsample_to=None, x_nhwc=False, in_factor=None):
        """``upsample_to=(Ho, Wo)``: x is the (B, C, H1, W1) feature map -- (B, H1, W1, C) with ``x_nhwc`` -- BEFORE the
        scaler's final bilinear resize; the resize is then commuted behind ``fc`` (ops.upsample_fc).  ``in_factor``: see
        Interp2dUpsample.forward_features(want_factor=True)."""
        x_latent = []
        if upsample_to is not None:
            assert self.spacial_fc
            x = ops.upsample_fc(x, upsample_to, self.fc.weight, self.fc.bias, grid, x_nhwc=x_nhwc,
                                in_factor=in_factor if in_factor is not None and in_factor.numel() else None)
        elif self.spacial_fc:
            x = ops.linear(x, self.fc.weight, self.fc.bias, extra=grid)
        # every intermediate of the stack has exactly one consumer (unless the latents are handed out): the SiLU backward of
        # a layer rides on the kernel that forms its result's gradient (ops.silu_gate_scope)
        with ops.silu_gate_scope(not self.return_latent):
            for layer in self.spectral_conv:
                x = layer(x)
                if self.return_latent:
                    x_latent.append(x.contiguous())
            x = ops.mlp_head(x, self.regressor[0].weight, self.regressor[0].bias, self.regressor[2].weight,
                             self.regressor[2].bias, act=_act_name(self.activation))
        if self.normalizer:
            x = self.normalizer.inverse_transform(x)
        if self.return_freq or self.return_latent:
            return x, dict(preds_freq=[], preds_latent=x_latent)
        return x


class _ToChannelsLast(torch.autograd.Function):
    """(B,C,H,W) -> (B,H,W,C), both dense.  The backward hands the CNN a dense NCHW gradient: the
    MIOpen / interpolate backward kernels are only exercised by PyTorch with that layout (a
    permuted-stride gradient from the token side faulted in the torch CNN backward on gfx950)."""

    @staticmethod
    def forward(ctx, x):
        return x.permute(0, 2, 3, 1).contiguous()

    @staticmethod
    def backward(ctx, g):
        return g.permute(0, 3, 1, 2).contiguous()


class _ToChannelsFirst(torch.autograd.Function):
    """(B,H,W,C) -> (B,C,H,W), both dense; dense NHWC gradient back to the token side."""

    @staticmethod
    def forward(ctx, x):
        return x.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, g):
        return g.permute(0, 2, 3, 1).contiguous()


class DownScaler(nn.Module):
    """(B, n, n, in) -> (B, n_s, n_s, out) (model.py:640-687).  downsample_mode='interp': conv + bilinear interpolation to
    ``interp_size``.  downsample_mode='conv' (the default): two Conv2dEncoders, the second with ``padding`` -- convolutions and
    2x2 average pools, n -> n_s fixed by the layers (13, 16, 21, 33, 35 -> 3, 4, 4, 5, 5); ``dropout`` and ``interp_size`` are
    not used in this mode, as in the reference."""

    def __init__(self, in_dim, out_dim, dropout=0.1, padding=5, downsample_mode='conv',
                 activation_type='silu', interp_size=None, debug=False):
        super().__init__()
        if downsample_mode == 'conv':
            self.downsample = nn.Sequential(
                Conv2dEncoder(in_dim=in_dim, out_dim=out_dim, activation_type=activation_type, debug=debug),
                Conv2dEncoder(in_dim=out_dim, out_dim=out_dim, padding=padding, activation_type=activation_type, debug=debug))
        elif downsample_mode == 'interp':
            self.downsample = Interp2dEncoder(in_dim=in_dim, out_dim=out_dim, interp_size=interp_size,
                                              activation_type=activation_type, dropout=dropout, debug=debug)
        else:
            raise NotImplementedError("downsample mode not implemented.")
        self.in_dim = in_dim
        self.out_dim = out_dim

    def forward(self, x):
        n_grid, bsz = x.size(1), x.size(0)
        x = x.reshape(bsz, n_grid, n_grid, self.in_dim)
        # one input channel: channels-last and channels-first are the same bytes
        x = x.reshape(bsz, 1, n_grid, n_grid) if self.in_dim == 1 else _ToChannelsFirst.apply(x)
        if isinstance(self.downsample, nn.Sequential):      # 'conv': the last pool of the second encoder writes channels-last
            return self.downsample[1](self.downsample[0](x), out_nhwc=True)
        return self.downsample(x, out_nhwc=True)


class UpScaler(nn.Module):
    """(B, n_s, n_s, in) -> (B, n, n, out) (model.py:690-749).  upsample_mode='interp': interp -> conv -> interp to
    ``interp_size``.  upsample_mode='conv' / 'deconv' (the default): two DeConv2dBlocks of transposed convolutions, channels-last
    throughout, n_s -> 16 n_s - 45 with the default padding=2, output_padding=0 (5 -> 35).  As in the reference the second
    block is built from ``in_dim`` again, so this mode needs out_dim == in_dim."""

    def __init__(self, in_dim: int, out_dim: int, hidden_dim=None, padding=2, output_padding=0, dropout=0.1,
                 upsample_mode='conv', activation_type='silu', interp_mode='bilinear', interp_size=None,
                 debug=False):
        super().__init__()
        hidden_dim = default(hidden_dim, in_dim)
        if upsample_mode in ['conv', 'deconv']:
            self.upsample = nn.Sequential(
                DeConv2dBlock(in_dim=in_dim, out_dim=out_dim, hidden_dim=hidden_dim, padding=padding,
                              output_padding=output_padding, dropout=dropout, activation_type=activation_type, debug=debug),
                DeConv2dBlock(in_dim=in_dim, out_dim=out_dim, hidden_dim=hidden_dim, padding=padding * 2,
                              output_padding=output_padding, dropout=dropout, activation_type=activation_type, debug=debug))
        elif upsample_mode == 'interp':
            self.upsample = Interp2dUpsample(in_dim=in_dim, out_dim=out_dim, interp_mode=interp_mode,
                                             interp_size=interp_size, dropout=dropout,
                                             activation_type=activation_type, debug=debug)
        else:
            raise NotImplementedError("upsample mode not implemented.")
        self.in_dim = in_dim
        self.out_dim = out_dim

    def forward(self, x):
        if isinstance(self.upsample, nn.Sequential):        # 'conv' / 'deconv'
            for block in self.upsample:
                x = block(x, in_nhwc=True, out_nhwc=True)
            return x
        return self.upsample(x, in_nhwc=True, out_nhwc=True)


class GCN(nn.Module):
    """Graph feature extractor: a learned edge encoder, then num_gcn_layers graph convolutions that share its output
    (reference model.py:376-427; state_dict keys edge_learner.lap_conv{1,2}.conv.0.weight, gcn_layer0.*, gcn_layers.{i}.*).

    forward(x [B, n, node_feats], edge [B, n, n, edge_feats]) -> [B, n, out_features]:
        E = EdgeEncoder(edge.permute(0, 3, 1, 2))                      [B, C, n, n], kept as its channel groups
        h_0 = x;  h_{l+1}[b,i,c] = sum_j E[b,c,i,j] (h_l W_l)[b,j,c] + bias_l[c]
    with a ReLU behind the layers 1 .. L-2 only, and only if `activation` is truthy: never behind gcn_layer0 or the last
    layer, so two layers have none.  The whole layer stack is one operator, ops.graph_conv_stack, on the gt_graphconv_*
    kernels; `dropout` and `relu` sit unused on the module tree as in the reference.

    Deviations from the reference, both accidents of its GraphConvolution.forward:
      * B = 1: its squeeze() drops the batch axis and the next layer fails; here B = 1 gives the natural result;
      * n == out_features: it decides whether to transpose by x.size(-1) != in_features, takes the [B, C, n] output of
        the previous layer for [B, n, C] and contracts the later layers over the wrong axis (0.79 relative L2 away from
        the formula above); here the formula holds for every n.
    num_gcn_layers = 1 (an IndexError in the reference's forward) is refused at construction."""

    def __init__(self, node_feats=4, out_features=96, num_gcn_layers=2, edge_feats=6, activation=True,
                 raw_laplacian=False, dropout=0.1, debug=False):
        super().__init__()
        if num_gcn_layers < 2:
            raise ValueError("num_gcn_layers >= 2")
        self.edge_learner = EdgeEncoder(out_dim=out_features, edge_feats=edge_feats, raw_laplacian=raw_laplacian)
        self.gcn_layer0 = GraphConvolution(in_features=node_feats, out_features=out_features, debug=debug)
        self.gcn_layers = nn.ModuleList([copy.deepcopy(GraphConvolution(
            in_features=out_features, out_features=out_features, debug=debug)) for _ in range(1, num_gcn_layers)])
        self.activation = activation
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(dropout)
        self.edge_feats = edge_feats
        self.debug = debug

    def forward(self, x, edge):
        H.need_f32_cuda(x, edge)
        assert edge.size(-1) == self.edge_feats
        layers = [self.gcn_layer0] + list(self.gcn_layers)
        L = len(layers)
        relu = [bool(self.activation) and 0 < l < L - 1 for l in range(L)]
        groups = self.edge_learner.groups(edge.permute(0, 3, 1, 2).contiguous())
        return ops.graph_conv_stack(x, groups, [g.weight for g in layers], [g.bias for g in layers], relu)


class GAT(nn.Module):
    """Graph feature extractor: num_gcn_layers graph-attention layers over one adjacency (reference model.py:430-469;
    state_dict keys gat_layer0.{W,a}, gat_layers.{i}.{W,a}).

    forward(x [B, n, node_feats], edge [B, n, n, E]) -> [B, n, out_features] with adj = edge[..., 0], read in place (the
    reference copies it out): gat_layer0, then
    gat_layers[:-1], each of THOSE followed by a ReLU iff `activation`, then gat_layers[-1].  Every layer keeps concat=True,
    so an ELU follows every layer, the last included.  The whole stack is one operator, ops.graph_attention_stack, on the
    gt_graphattn_* kernels: the keep bits of adj are packed once for all layers and both directions.  Each layer's dropout
    follows its own `dropout` float and module.training.  edge_feats and `relu` sit unused as in the reference.
    num_gcn_layers = 1 (an IndexError in the reference's forward) is refused at construction."""

    def __init__(self, node_feats=4, out_features=96, num_gcn_layers=2, edge_feats=None, activation=False, debug=False):
        super().__init__()
        if num_gcn_layers < 2:
            raise ValueError("num_gcn_layers >= 2")
        self.gat_layer0 = GraphAttention(in_features=node_feats, out_features=out_features)
        self.gat_layers = nn.ModuleList([copy.deepcopy(GraphAttention(
            in_features=out_features, out_features=out_features)) for _ in range(1, num_gcn_layers)])
        self.activation = activation
        self.relu = nn.ReLU()
        self.debug = debug

    def forward(self, x, edge):
        H.need_f32_cuda(x, edge)
        layers = [self.gat_layer0] + list(self.gat_layers)
        L = len(layers)
        relu = [bool(self.activation) and 0 < l < L - 1 for l in range(L)]
        args = [g.stack_args() for g in layers]
        if any(a != args[0] for a in args[1:]):        # layers edited apart after construction: one operator call each
            out = x
            adj = edge[..., 0]
            for g, r in zip(layers, relu):
                out = ops.graph_attention_stack(out, adj, (g.W,), (g.a,), (r,), **g.stack_args())
            return out
        return ops.graph_attention_stack(x, edge[..., 0], [g.W for g in layers], [g.a for g in layers], relu,
                                         **args[0])


class _ConfiguredModel(nn.Module):
    """Config-dict plumbing shared by the three model classes: every config key (and every name in
    ADDITIONAL_ATTR) becomes an attribute, missing keys read as None (model.py:1071-1074)."""

    _hip_attention = ('fourier', 'integral', 'local', 'galerkin', 'linear', 'global', 'softmax')

    def _read_config(self, kwargs):
        self.config = defaultdict(lambda: None, **kwargs)
        for key in list(self.config.keys()) + ADDITIONAL_ATTR:
            setattr(self, key, self.config[key])
        self.dim_feedforward = default(self.dim_feedforward, 2 * self.n_hidden)
        self.dropout = default(self.dropout, 0.05)
        self.dpo = nn.Dropout(self.dropout)
        if self.decoder_type == 'attention':
            self.num_encoder_layers += 1

    def _graph_extractor(self, node_feats):
        """The GCN of feat_extract_type='gcn' with num_feat_layers > 0 (model.py:847-856, 1084-1093), or None."""
        if not (self.num_feat_layers and self.num_feat_layers > 0):
            return None
        if self.feat_extract_type == 'gat':
            # GraphAttention / GAT exist on the HIP path; the switch stays unwired because
            # tests/test_graph_conv_cpu.py::test_refusals pins this refusal (and a message that names GCN)
            raise NotImplementedError("feat_extract_type='gat' is not wired into the config switch yet (GCN, "
                                      "feat_extract_type='gcn', is); the modules exist: build the model without a graph "
                                      "extractor and assign model.feat_extract = GAT(node_feats, out_features=n_hidden, "
                                      "num_gcn_layers=...), which forward() calls as feat_extract(node, edge)")
        if self.feat_extract_type != 'gcn':
            return None
        return GCN(node_feats=node_feats, edge_feats=self.edge_feats, num_gcn_layers=self.num_feat_layers,
                   out_features=self.n_hidden, activation=self.graph_activation, raw_laplacian=self.raw_laplacian,
                   debug=self.debug)

    def _stack_encoders(self, official=False, **extra):
        if official and self.attention_type == 'official':
            # the classic Transformer layer (model.py:888-895); the 1-D model only -- the 2-D models' branch does not run
            # in the reference
            layer = _TransformerEncoderLayer(d_model=self.n_hidden, nhead=self.n_head,
                                             dim_feedforward=self.dim_feedforward, layer_norm=self.layer_norm,
                                             attn_weight=self.return_attn_weight, dropout=self.encoder_dropout)
            self.encoder_layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(self.num_encoder_layers)])
            return
        if self.attention_type not in self._hip_attention:
            raise NotImplementedError(f"attention_type={self.attention_type!r}: only the galerkin / fourier / linear / softmax "
                                      "encoders are on the HIP hot path")
        layer = SimpleTransformerEncoderLayer(
            d_model=self.n_hidden, n_head=self.n_head, attention_type=self.attention_type,
            dim_feedforward=self.dim_feedforward, layer_norm=self.layer_norm, attn_norm=self.attn_norm,
            pos_dim=self.pos_dim, xavier_init=self.xavier_init, diagonal_weight=self.diagonal_weight,
            dropout=self.encoder_dropout, ffn_dropout=self.ffn_dropout, debug=self.debug, **extra)
        # all layers start as deep copies of one initialised layer (model.py:896-897, 1153-1154)
        self.encoder_layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(self.num_encoder_layers)])

    @staticmethod
    def _initialize_layer(layer, gain=1e-2):
        for param in layer.parameters():
            if param.ndim > 1:
                xavier_uniform_(param, gain=gain)
            else:
                constant_(param, 0)

    def print_config(self):
        for a in self.config.keys():
            if not a.startswith('__'):
                print(f"{a}: \t", getattr(self, a))

    def _drop(self, x):
        return ops.dropout(x, self.dpo.p, self.training)


class SimpleTransformer(_ConfiguredModel):
    """1-D model of ex1 (Burgers): Linear -> N encoder layers -> spectral/pointwise decoder (model.py:752)."""

    def __init__(self, **kwargs):
        super().__init__()
        self._read_config(kwargs)
        self.spacial_dim = default(self.spacial_dim, self.pos_dim)
        self.spacial_fc = default(self.spacial_fc, False)
        self.feat_extract = (self._graph_extractor(self.node_feats)
                             or Identity(in_features=self.node_feats, out_features=self.n_hidden))
        self._stack_encoders(official=True, norm_type=self.norm_type, batch_norm=self.batch_norm,
                             symmetric_init=self.symmetric_init, attn_weight=self.return_attn_weight,
                             residual_type=self.residual_type, activation_type=self.attn_activation)
        if self.n_freq_targets and self.n_freq_targets > 0:
            raise NotImplementedError("frequency-target regressors are outside the HIP hot path")
        if self.decoder_type == 'pointwise':
            self.regressor = PointwiseRegressor(in_dim=self.n_hidden, n_hidden=self.n_hidden,
                                                out_dim=self.n_targets, spacial_fc=self.spacial_fc,
                                                spacial_dim=self.spacial_dim,
                                                activation=self.regressor_activation,
                                                dropout=self.decoder_dropout, debug=self.debug)
            self._initialize_layer(self.regressor)
        elif self.decoder_type == 'ifft':
            self.regressor = SpectralRegressor(in_dim=self.n_hidden, n_hidden=self.n_hidden,
                                               freq_dim=self.freq_dim, out_dim=self.n_targets,
                                               num_spectral_layers=self.num_regressor_layers,
                                               modes=self.fourier_modes, spacial_dim=self.spacial_dim,
                                               spacial_fc=self.spacial_fc, dim_feedforward=self.freq_dim,
                                               activation=self.regressor_activation,
                                               dropout=self.decoder_dropout)
        else:
            raise NotImplementedError("Decoder type not implemented")
        self.config = dict(self.config)
        self.__name__ = self.attention_type.capitalize() + 'Transformer'

    def forward(self, node, edge, pos, grid=None, weight=None):
        x_latent, attn_weights = [], []
        x = self.feat_extract(node, edge)
        if self.spacial_residual or self.return_latent:
            res = x.contiguous()
            x_latent.append(res)
        for encoder in self.encoder_layers:
            if self.return_attn_weight:
                x, w = encoder(x, pos, weight)
                attn_weights.append(w)
            else:
                x = encoder(x, pos, weight)
            if self.return_latent:
                x_latent.append(x.contiguous())
        if self.spacial_residual:
            x = res + x
        x = self._drop(x)
        x = self.regressor(x, grid=grid)
        return dict(preds=x, preds_freq=None, preds_latent=x_latent, attn_weights=attn_weights)

    def get_encoder(self):
        return self.encoder_layers


class FourierTransformer2D(_ConfiguredModel):
    """2-D model of ex2/ex3 (Darcy): CNN downscaler -> N encoder layers -> upscaler -> decoder (model.py:945)."""

    def __init__(self, **kwargs):
        super().__init__()
        self._read_config(kwargs)
        self.feat_extract = self._graph_extractor(self.n_hidden) or Identity()
        if self.downscaler_size:
            self.downscaler = DownScaler(in_dim=self.node_feats, out_dim=self.n_hidden,
                                         downsample_mode=self.downsample_mode,
                                         interp_size=self.downscaler_size, dropout=self.downscaler_dropout,
                                         activation_type=self.downscaler_activation)
        else:
            self.downscaler = Identity(in_features=self.node_feats + self.spacial_dim,
                                       out_features=self.n_hidden)
        if self.upscaler_size:
            self.upscaler = UpScaler(in_dim=self.n_hidden, out_dim=self.n_hidden,
                                     upsample_mode=self.upsample_mode, interp_size=self.upscaler_size,
                                     dropout=self.upscaler_dropout, activation_type=self.upscaler_activation)
        else:
            self.upscaler = Identity()
        self._stack_encoders(batch_norm=self.batch_norm, symmetric_init=self.symmetric_init,
                             attn_weight=self.return_attn_weight, norm_eps=self.norm_eps)
        if self.decoder_type == 'pointwise':
            self.regressor = PointwiseRegressor(in_dim=self.n_hidden, n_hidden=self.n_hidden,
                                                out_dim=self.n_targets,
                                                num_layers=self.num_regressor_layers,
                                                spacial_fc=self.spacial_fc, spacial_dim=self.spacial_dim,
                                                activation=self.regressor_activation,
                                                dropout=self.decoder_dropout,
                                                return_latent=self.return_latent, debug=self.debug)
        elif self.decoder_type == 'ifft2':
            self.regressor = SpectralRegressor(in_dim=self.n_hidden, n_hidden=self.freq_dim,
                                               freq_dim=self.freq_dim, out_dim=self.n_targets,
                                               num_spectral_layers=self.num_regressor_layers,
                                               modes=self.fourier_modes, spacial_dim=self.spacial_dim,
                                               spacial_fc=self.spacial_fc,
                                               activation=self.regressor_activation,
                                               last_activation=self.last_activation,
                                               dropout=self.decoder_dropout,
                                               return_latent=self.return_latent, debug=self.debug)
        else:
            raise NotImplementedError("Decoder type not implemented")
        self.config = dict(self.config)
        self.__name__ = self.attention_type.capitalize() + 'Transformer2D'

    def forward(self, node, edge, pos, grid, weight=None, boundary_value=None):
        bsz = node.size(0)
        n_s = int(pos.size(1) ** 0.5)
        x_latent, attn_weights = [], []
        if not self.downscaler_size:
            node = torch.cat([node, pos.contiguous().view(bsz, n_s, n_s, -1)], dim=-1)
        x = self.downscaler(node)
        x = x.reshape(bsz, -1, self.n_hidden)
        x = self.feat_extract(x, edge)
        x = self._drop(x)
        for encoder in self.encoder_layers:
            if self.return_attn_weight:
                x, w = encoder(x, pos, weight)
                attn_weights.append(w)
            else:
                x = encoder(x, pos, weight)
            if self.return_latent:
                x_latent.append(x.contiguous())
        x = x.view(bsz, n_s, n_s, self.n_hidden)
        up = getattr(self.upscaler, 'upsample', None)
        if (isinstance(up, Interp2dUpsample) and up.interp_mode == 'bilinear' and not self.return_latent
                and isinstance(self.regressor, SpectralRegressor) and self.regressor.spacial_fc
                and grid is not None and not (self.training and self.dpo.p > 0)):
            # nothing sits between the upscaler's last resize and the regressor's fc: run fc at the coarse
            # resolution and interpolate its freq_dim channels instead of the n_hidden ones
            mid = up.features_nhwc()
            feat, fac = up.forward_features(x, in_nhwc=True, out_nhwc=mid, want_factor=True)
            x = self.regressor(feat, grid=grid, upsample_to=tuple(up.interp_size[1]), x_nhwc=mid, in_factor=fac)
        else:
            x = self.upscaler(x)
            if self.return_latent:
                x_latent.append(x.contiguous())
            x = self._drop(x)
            if self.return_latent:
                x, xr_latent = self.regressor(x, grid=grid)
                x_latent.append(xr_latent)
            else:
                x = self.regressor(x, grid=grid)
        if self.normalizer:
            x = self.normalizer.inverse_transform(x)
        if self.boundary_condition == 'dirichlet':
            x = F.pad(x[:, 1:-1, 1:-1].contiguous(), (0, 0, 1, 1, 1, 1), "constant", 0)
            if boundary_value is not None:
                assert x.size() == boundary_value.size()
                x = x + boundary_value
        return dict(preds=x, preds_latent=x_latent, attn_weights=attn_weights)

    # the normalizer is a plain object holding tensors: move it with the module (model.py:1026-1042)
    def cuda(self, device=None):
        self = super().cuda(device)
        if self.normalizer:
            self.normalizer = self.normalizer.cuda(device)
        return self

    def cpu(self):
        self = super().cpu()
        if self.normalizer:
            self.normalizer = self.normalizer.cpu()
        return self

    def to(self, *args, **kwargs):
        self = super().to(*args, **kwargs)
        if self.normalizer:
            self.normalizer = self.normalizer.to(*args, **kwargs)
        return self


FourierTransformer = SimpleTransformer      # pre-rename alias used by the reference's eval notebooks


class FourierTransformer2DLite(_ConfiguredModel):
    """Navier-Stokes (ex4) model: Linear(cat[node, pos]) -> N encoder layers -> spectral decoder
    (model.py:1186-1283)."""

    def __init__(self, **kwargs):
        super().__init__()
        self._read_config(kwargs)
        self.spacial_dim = default(self.spacial_dim, self.pos_dim)
        self.spacial_fc = default(self.spacial_fc, False)
        self.feat_extract = Identity(in_features=self.node_feats, out_features=self.n_hidden)
        self._stack_encoders(norm_type=self.norm_type)
        self.regressor = SpectralRegressor(in_dim=self.n_hidden, n_hidden=self.n_hidden,
                                           freq_dim=self.freq_dim, out_dim=self.n_targets,
                                           num_spectral_layers=self.num_regressor_layers,
                                           modes=self.fourier_modes, spacial_dim=self.spacial_dim,
                                           spacial_fc=self.spacial_fc, dim_feedforward=self.freq_dim,
                                           activation=self.regressor_activation,
                                           dropout=self.decoder_dropout)
        self.config = dict(self.config)

    def forward(self, node, edge, pos, grid=None):
        bsz, input_dim, n_grid = node.size(0), node.size(-1), grid.size(1)
        node = torch.cat([node.reshape(bsz, -1, input_dim), pos], dim=-1)
        x = self.feat_extract(node, edge)
        for encoder in self.encoder_layers:
            x = encoder(x, pos)
        x = self._drop(x)
        x = x.view(bsz, n_grid, n_grid, -1)
        x = self.regressor(x, grid=grid)
        return dict(preds=x, preds_freq=None, preds_latent=None, attn_weights=None)


# --------------------------------------------------------------------------------------- random-feature baselines
class RandomFeatureEncoderLayer(nn.Module):
    """x <- LN1(x + drop1(attn(x, x, x, pos))); x <- LN2(x + drop2(ff(x))): the post-norm encoder layer of the reference's
    examples/ex1_burgers_random_fourier_features.py (:321-386) around RandomFourierAttention, always with both LayerNorms.
    Arguments, defaults and state-dict keys are the example's; ``pos_dim`` is added (the example fixes it at 1)."""

    def __init__(self, d_model=96, n_head=2, dim_feedforward=512, attention_type='favor', layer_norm=True, attn_norm=None,
                 norm_type='layer', norm_eps=None, xavier_init: float = 1e-2, diagonal_weight: float = 1e-2,
                 activation_type='relu', dropout=0.1, ffn_dropout=None, debug=False, pos_dim=1):
        super().__init__()
        dropout = default(dropout, 0.05)
        ffn_dropout = default(ffn_dropout, dropout)
        norm_eps = default(norm_eps, 1e-5)
        self.attn = RandomFourierAttention(d_model, n_head, pos_dim=pos_dim, attention_type=attention_type,
                                           xavier_init=xavier_init, diagonal_weight=diagonal_weight)
        self.d_model = d_model
        self.n_head = n_head
        self.norm_eps = norm_eps
        self.layer_norm1 = nn.LayerNorm(d_model, eps=norm_eps)
        self.layer_norm2 = nn.LayerNorm(d_model, eps=norm_eps)
        dim_feedforward = default(dim_feedforward, 2 * d_model)
        self.ff = FeedForward(in_dim=d_model, dim_feedforward=dim_feedforward, activation=activation_type,
                              dropout=ffn_dropout)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.debug = debug

    def forward(self, x, pos=None):
        p1 = self.dropout1.p if self.training else 0.0
        p2 = self.dropout2.p if self.training else 0.0
        x = self.attn.fused_forward(x, pos, residual=x, p_out=p1)
        x = ops.layer_norm(x, self.layer_norm1.weight, self.layer_norm1.bias, self.norm_eps)
        x = self.ff.fused_forward(x, residual=x, p_out=p2)
        return ops.layer_norm(x, self.layer_norm2.weight, self.layer_norm2.bias, self.norm_eps)


class RandomFeatureTransformer(_ConfiguredModel):
    """The model of the reference's random-feature example (its ``SimpleTransformer``, :389-480): cat([node, pos]) ->
    Identity feature layer -> N RandomFeatureEncoderLayer -> dropout -> SpectralRegressor.  Config keys as in the example:
    node_feats (coordinates included), pos_dim, n_hidden, n_head (1), num_encoder_layers, dim_feedforward,
    attention_type ('favor' / 'rfa'), xavier_init, diagonal_weight, encoder_dropout, ffn_dropout, dropout, and the
    regressor's n_targets, freq_dim, num_regressor_layers, fourier_modes, spacial_dim, spacial_fc, regressor_activation,
    decoder_dropout."""

    def __init__(self, **kwargs):
        super().__init__()
        self._read_config(kwargs)
        if self.attention_type not in ('favor', 'rfa'):
            raise ValueError(f"RandomFeatureTransformer: attention_type={self.attention_type!r} (use 'favor' or 'rfa'; the "
                             "other types are SimpleTransformer's)")
        self.pos_dim = default(self.pos_dim, 1)
        self.spacial_dim = default(self.spacial_dim, self.pos_dim)
        self.spacial_fc = default(self.spacial_fc, False)
        layer = RandomFeatureEncoderLayer(d_model=self.n_hidden, n_head=self.n_head, dim_feedforward=self.dim_feedforward,
                                          layer_norm=self.layer_norm, attention_type=self.attention_type,
                                          attn_norm=self.attn_norm, norm_type=self.norm_type, xavier_init=self.xavier_init,
                                          diagonal_weight=self.diagonal_weight, dropout=self.encoder_dropout,
                                          ffn_dropout=self.ffn_dropout, debug=self.debug, pos_dim=self.pos_dim)
        self.feat_extract = Identity(in_features=self.node_feats, out_features=self.n_hidden)
        self.encoder_layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(self.num_encoder_layers)])
        self.regressor = SpectralRegressor(in_dim=self.n_hidden, n_hidden=self.n_hidden, freq_dim=self.freq_dim,
                                           out_dim=self.n_targets, num_spectral_layers=self.num_regressor_layers,
                                           modes=self.fourier_modes, spacial_dim=self.spacial_dim,
                                           spacial_fc=self.spacial_fc, dim_feedforward=self.freq_dim,
                                           activation=self.regressor_activation, dropout=self.decoder_dropout)
        self.config = dict(self.config)
        self.__name__ = self.attention_type.capitalize() + 'Transformer'

    def set_redraw(self, flag: bool):
        """Freeze (False) or release (True) the per-forward redraw of every layer's ``omega``."""
        for layer in self.encoder_layers:
            layer.attn.redraw = flag

    def forward(self, node, edge, pos, grid=None):
        x = self.feat_extract(torch.cat([node, pos], dim=-1), edge)
        for encoder in self.encoder_layers:
            x = encoder(x, pos)
        x = self._drop(x)
        x = self.regressor(x, grid=grid)
        return dict(preds=x, preds_freq=None, preds_latent=None, attn_weights=None)
