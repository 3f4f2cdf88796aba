"""The rules of the scaler family that are stated once (ops/resize.py: out_size; ops/conv.py: _plain_conv3x3, _filter_fwd,
_filter_dgrad; _hip.bilinear2d_seg_supported), and the surface of the ``ops`` package.  None of this needs the built library."""
import importlib

import pytest
import torch
from torch import nn


def test_out_size_is_the_reference_floor_rule_cpu():
    """A float is F.interpolate's recompute_scale_factor=True rule; a pair of ints passes through; a per-axis float pair
    has no HIP path."""
    from galerkin_transformer import ops
    cases = (((141, 141, 0.5), (70, 70)), ((78, 78, 0.555), (43, 43)), ((211, 211, 0.54), (113, 113)),
             ((5, 7, 1.5), (7, 10)), ((43, 43, 3.3), (141, 141)), ((421, 421, 1 / 3), (140, 140)))
    for (h, w, s), want in cases:
        ref = torch.nn.functional.interpolate(torch.zeros(1, 1, h, w), scale_factor=s, mode="bilinear", align_corners=True,
                                              recompute_scale_factor=True)
        assert tuple(ref.shape[2:]) == want, (h, w, s)
        assert ops.out_size(h, w, s) == want, (h, w, s)
    assert ops.out_size(9, 9, (3, 4)) == (3, 4) and ops.out_size(9, 9, [3, 4]) == (3, 4)
    with pytest.raises(NotImplementedError, match="per-axis scale factors"):
        ops.out_size(9, 9, (0.5, 0.5))


def test_plain_conv3x3_refuses_every_single_deviation_cpu():
    from galerkin_transformer.ops.conv import _plain_conv3x3
    assert _plain_conv3x3(nn.Conv2d(16, 32, 3, padding=1, bias=False))
    deviations = dict(bias=nn.Conv2d(16, 32, 3, padding=1),
                      stride=nn.Conv2d(16, 32, 3, padding=1, stride=2, bias=False),
                      padding=nn.Conv2d(16, 32, 3, padding=0, bias=False),
                      dilation=nn.Conv2d(16, 32, 3, padding=1, dilation=2, bias=False),
                      groups=nn.Conv2d(16, 32, 3, padding=1, groups=2, bias=False),
                      kernel=nn.Conv2d(16, 32, 5, padding=1, bias=False),
                      reflect=nn.Conv2d(16, 32, 3, padding=1, padding_mode="reflect", bias=False),
                      linear=nn.Linear(16, 32, bias=False))
    for name, conv in deviations.items():
        assert not _plain_conv3x3(conv), name


def test_filter_layouts_equal_the_former_expressions_cpu():
    """The wide convolution's two layouts were written without padding, the chain's with it; both are now _filter_fwd /
    _filter_dgrad.  The former expressions are written out here on _conv_k_order / _pad_filter, the reference arrangement."""
    from galerkin_transformer.ops import conv
    k_order, pad = conv._conv_k_order, conv._pad_filter
    torch.manual_seed(0)
    # Conv3x3NhwcFn at (Cout, Cin) = (128, 96): no padding
    w = torch.randn(128, 96, 3, 3)
    Cout, Cin = 128, 96
    assert torch.equal(conv._filter_fwd(w, Cout, Cin), k_order(w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)))
    assert torch.equal(conv._filter_dgrad(w, Cin, Cout), k_order(w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9, Cout)))
    # ... which is one index_select and no mask multiply
    for key in (("conv_fwd", Cout, Cin), ("conv_dgrad", Cin, Cout)):
        idx, mask, _ = conv._gather_cache[(key, (128, 96, 3, 3), "cpu")]
        assert mask is None and idx.numel() == w.numel()
    # ScalerConvChainFn: first convolution (C0 = 128 -> 42, CP = 48) and a later one (CP -> 44: input segment padded too)
    for shape, CP, ci_p in (((42, 128, 3, 3), 48, 128), ((44, 42, 3, 3), 48, 48)):
        w = torch.randn(*shape)
        assert torch.equal(conv._filter_fwd(w, CP, ci_p), k_order(pad(w, CP, ci_p)))
        assert torch.equal(conv._filter_dgrad(w, ci_p, CP), k_order(pad(w.flip(2, 3).transpose(0, 1), ci_p, CP)))
        assert conv._gather_cache[(("conv_fwd", CP, ci_p), shape, "cpu")][1] is not None       # padded: zero mask


def test_bilinear2d_seg_supported_mirrors_the_segment_kernels_cpu():
    """The cases of test_scaler_chain_eligibility_mirrors_the_segment_kernels_cpu on the mirror itself (gt_resize.hip:
    check_seg, taps_fit)."""
    from galerkin_transformer import _hip as H
    assert H.RS_MAXT == 6

    def ok(widths, out, inp=78):
        return H.bilinear2d_seg_supported(sum(widths), widths[0], (max(widths) + 15) // 16 * 16, (inp, inp), (out, out))

    assert ok((42, 42, 44), 43)
    assert not ok((37, 37, 38), 43) and not ok((53, 53, 54), 43)         # odd segments
    assert ok((42, 42, 44), 150) and not ok((42, 42, 44), 240)           # 2 (no - 1)/(ni - 1) + 2 <= 6  <=>  no <= 155 from 78
    assert ok((42, 42, 44), 155) and not ok((42, 42, 44), 156)
    assert H.bilinear2d_seg_supported(128, 42, 48, (1, 78), (6, 43)) and not H.bilinear2d_seg_supported(128, 42, 48, (1, 78), (7, 43))
    assert not H.bilinear2d_seg_supported(126, 42, 48, (78, 78), (43, 43))       # C not a multiple of 4
    assert not H.bilinear2d_seg_supported(84, 42, 48, (78, 78), (43, 43))        # no third segment
    assert not H.bilinear2d_seg_supported(136, 42, 48, (78, 78), (43, 43))       # third segment wider than its padding


# what layers.py, model.py, spectral.py, tests/ and tools/ reach as ops.NAME (or import from the package)
_SURFACE = """SimpleAttentionFn _c _conv_implicit _conv_k_order _conv_wgrad _crb_bits _fold_masks _gate_depth _gate_fold
_masked_twins _offer_gate _pad_filter _qkvnorm_fused _scaler_chain _silu_gates _take_gate bilinear_resize
bilinear_resize_seg conv3x3_nhwc conv3x3_nhwc_implicit conv3x3_nhwc_ok conv3x3_resize drop_act dropout feed_forward
get_attention_dropout layer_norm linear mlp_head packed_params push_attention_masks scaler_chain_ok scaler_conv_chain
set_attention_dropout set_relu_mask_sink set_scaler_mask_sink silu_gate_scope simple_attention upsample_fc""".split()

# every switch cell and registry, with its home module
_CELLS = dict(_handoff="_fold_masks _mask_hints _masked_twins _fold_seq _gate_fold _gate_depth _silu_gates _relu_mask_sink "
                       "_scaler_mask_sink",
              conv="_crb_bits _conv_implicit _conv_wgrad _conv_wgrad_planes _scaler_chain _scaler_wgrad_hip _gather_cache",
              dense="_ffn_bwd_fused", attention="_plain_tiles _dkv_ln_fused _qkvnorm_fused")


def test_ops_package_keeps_the_surface_of_the_module_cpu():
    from galerkin_transformer import ops
    for name in _SURFACE:
        assert hasattr(ops, name), name
    assert not hasattr(ops, "_attn_mode")        # rebound with `global`: lives in ops.attention with its readers
    for module, names in _CELLS.items():
        home = importlib.import_module(f"galerkin_transformer.ops.{module}")
        for name in names.split():
            assert getattr(ops, name) is getattr(home, name), name
            assert isinstance(getattr(ops, name), (list, dict)), name
    for name in _SURFACE:                        # and every re-exported function or class is its home module's object
        obj = getattr(ops, name)
        if hasattr(obj, "__module__"):
            home = importlib.import_module(obj.__module__)
            assert obj.__module__.startswith("galerkin_transformer.") and getattr(home, name) is obj, name
