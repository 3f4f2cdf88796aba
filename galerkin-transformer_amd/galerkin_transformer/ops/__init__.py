"""Autograd operators of the hot path, built on the C ABI (``_hip``).

Each ``torch.autograd.Function`` here enqueues hand-written HIP kernels for forward and
backward; torch only owns the tensors and the autograd graph.  Reference call sites
(the reference's libs/) are cited per operator.

One module per operator family; this file only re-exports (every name is the object of its home module):

``_handoff``     what one operator leaves for the next: the masked twins of data gradients, the SiLU gates, the two
                 parity sinks
``elementwise``  dropout, the dropout / activation tails, row LayerNorm, ``_c``
``resize``       bilinear resize, the segment resize behind the convolution chain, ``upsample_fc``; ``out_size``, the
                 one statement of the size-or-scale-factor rule
``conv``         conv0 + resize, the wide channels-last 3x3 convolution, the chain of three narrow ones; their filter
                 layouts, weight-gradient route, library fallback, eligibility functions and switches
``scaler_conv`` the 'conv' scaler modes: 2x2 average pool + activation, the 3x3 / stride-2 transposed convolution,
                 ``deconv_out_size``
``dense``        ``packed_params``, Linear, the regression head, FeedForward, FeedForward with BatchNorm1d
``graph``        the graph-convolution stack of the GCN feature extractor, ``graph_conv_stack``; the edge encoder's
                 library convolution with a reproducible weight gradient, ``edge_conv``
``loss``         the weighted-L2 / H1 objectives per sample: ``H1Loss2dFn`` (2-D), ``H1Loss1dFn`` (1-D)
``rfattn``       random-feature attention ('rfa' / 'favor'): ``RandomFeatureAttentionFn``, ``random_feature_attention``
``attention``    the attention-dropout mode, mask queue and call setup; ``AttnConfig``, the core table ``_CORES`` (kind ->
                 forward and backward core) with its checks and per-call namespace; ``SimpleAttentionFn`` with its
                 projection stage, ``CrossAttentionFn`` on the same table, ``multihead_attention`` (nn.MultiheadAttention's
                 arithmetic), ``causal_linear_attention`` (the causal core alone on [B, h, n, D] tensors)
"""
from ._handoff import (_fold_masks, _fold_seq, _gate_depth, _gate_fold, _hint_output_mask, _mask_hints,  # noqa: F401
                       _masked_twins, _offer_gate, _offer_twin, _relu_mask_sink, _scaler_mask_sink, _silu_gates,
                       _take_gate, _take_twin, _wanted_mask, set_relu_mask_sink, set_scaler_mask_sink, silu_gate_scope)
from .attention import (CausalLinearAttnFn, CrossAttentionFn, SimpleAttentionFn, _dkv_ln_fused, _plain_tiles,  # noqa: F401
                        _qkvnorm_fused, causal_linear_attention, check_cross_shapes, check_kv_mask, cross_attention,
                        get_attention_dropout, multihead_attention,
                        push_attention_masks, set_attention_dropout, simple_attention)
from .conv import (Conv3x3NhwcFn, Conv3x3ResizeFn, ScalerConvChainFn, _conv_implicit, _conv_k_order,  # noqa: F401
                   _conv_wgrad, _conv_wgrad_planes, _crb_bits, _gather_cache, _gathered,
                   _pad_filter, _plain_conv3x3, _scaler_chain, _scaler_wgrad_hip, conv3x3_nhwc, conv3x3_nhwc_implicit,
                   conv3x3_nhwc_ok, conv3x3_resize, scaler_chain_ok, scaler_conv_chain)
from .dense import (FeedForwardBNFn, FeedForwardFn, LinearFn, MlpHeadFn, _check_res_is_x, _ffn_bwd_fused,  # noqa: F401
                    feed_forward, feed_forward_bn, linear, mlp_head, packed_params)
from .elementwise import (DropActFn, DropoutFn, LayerNormFn, _c, _next_salt, drop_act, dropout,  # noqa: F401
                          layer_norm)
from .graph import (EdgeConvFn, GraphAttentionStackFn, GraphConvStackFn, edge_conv, graph_attention_stack,  # noqa: F401
                    graph_conv_stack)
from .loss import H1Loss1dFn, H1Loss2dFn, weighted_l2_terms_1d, weighted_l2_terms_2d  # noqa: F401
from .resize import (ResizeFn, ResizeSegFn, UpsampleFcFn, bilinear_resize, bilinear_resize_seg, out_size,  # noqa: F401
                     upsample_fc)
from .rfattn import RandomFeatureAttentionFn, random_feature_attention  # noqa: F401
from .scaler_conv import (AvgPool2ActFn, ConvTranspose3x3S2Fn, avgpool2_act, conv_transpose3x3s2,  # noqa: F401
                          deconv_out_size)
