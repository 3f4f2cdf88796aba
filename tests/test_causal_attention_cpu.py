"""attention_type='causal' and GalerkinTransformerDecoderLayer, CPU side: the plain-torch restatement (tests/_causal_ref.py)
against the fixtures recorded from the reference function (tests/golden/causal/), the decoder layer's state_dict against the
reference's recorded names and shapes, the refusals, and the host-visible surface of the new kernels.  No GPU needed.

Relative error of a tensor: max |difference| over its scale.  The scale of the output is max |reference|.  The scale of a
gradient is max(max |reference|, max |cot| max |out| / max |input|), the size of the terms the gradient is a difference of:
the operator is homogeneous of degree 0 in q and in k up to eps, and at n = 1 its output does not depend on q, k at all but
through eps, so the recorded dq, dk there (1e-6 against terms of size 1) are the remainder of a cancellation that float64
itself -- the reference's included -- carries to 1e-9 of their own size only.  Measured (test_restatement_matches_fixture
prints them): out <= 6e-16, gradients <= 3.1e-15 of max |reference| at n = 65, 130; at n = 1 dq 3.2e-08 and dk 1.0e-08 of
max |reference|, 1e-15 of the scale.

The scan formulation (causal_ref_scan) is what stands in for the reference function where that does not exist (the GPU
tests): test_scan_form_rounds_like_the_reference_function holds its float32 error against float64, per tensor, within a
factor 2 either way of the reference function's own recorded float32 error.  Measured: the ratio of the two errors lies
between 0.63 and 1.61 over the sixteen tensors (printed by the test)."""
import ctypes
import os

import pytest
import torch

from _causal_ref import (CASES, CAUSAL_DIR, CausalGolden, causal_grads, condition, decoder_state_dict_shapes, err)

GRADS = ("out", "dq", "dk", "dv")

REF_TOL = 1e-12
NEW_SYMBOLS = ("gt_causal_attn_state_bytes", "gt_causal_attn_bwd_ws_bytes", "gt_causal_attn_fwd", "gt_causal_attn_bwd")


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_fixture(name):
    g = CausalGolden(name)
    assert g.meta["masked"] == (g.kv_mask is not None)
    assert condition(g.q, g.k, g.kv_mask) <= 2
    out, dq, dk, dv = causal_grads(g.q, g.k, g.v, g.kv_mask, g.cot, torch.float64)
    assert out.dtype == torch.float64 and g.out.dtype == torch.float64 and out.shape == g.out.shape
    e_out = err(out, g.out)
    print(f"{name}: out {e_out:.1e}")
    assert e_out < REF_TOL
    term = float(g.cot.abs().max() * g.out.abs().max())
    for what, got, ref, x in (("dq", dq, g.dq, g.q), ("dk", dk, g.dk, g.k), ("dv", dv, g.dv, g.v)):
        diff = float((got - ref).abs().max())
        scale = max(float(ref.abs().max()), term / float(x.abs().max()))
        print(f"{name}: {what} {diff / float(ref.abs().max()):.1e} of max |reference|, {diff / scale:.1e} of the scale")
        assert diff < REF_TOL * scale, what
    if g.kv_mask is not None:
        assert not g.kv_mask[:, :2].any() and g.kv_mask[:, 2].all()
        assert float(g.out[:, :, :2].abs().max()) == 0.0 and float(out[:, :, :2].abs().max()) == 0.0
        drop = ~g.kv_mask[:, None, :, None].expand_as(g.dk)
        assert float(g.dk[drop].abs().max()) == 0.0 and float(g.dv[drop].abs().max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_scan_form_matches_fixture_in_float64(name):
    g = CausalGolden(name)
    got = causal_grads(g.q, g.k, g.v, g.kv_mask, g.cot, torch.float64, form="scan")
    term = float(g.cot.abs().max() * g.out.abs().max())
    for what, t, ref, x in zip(GRADS, got, (g.out, g.dq, g.dk, g.dv), (None, g.q, g.k, g.v)):
        scale = float(ref.abs().max()) if x is None else max(float(ref.abs().max()), term / float(x.abs().max()))
        assert float((t - ref).abs().max()) < REF_TOL * scale, what


@pytest.mark.parametrize("name", [c for c in CASES if c != "n1_d16"])
def test_scan_form_rounds_like_the_reference_function(name):
    """(n = 1 is left out: there the float32 dq, dk of either are rounding noise of a cancelled quantity, module docstring.)"""
    g = CausalGolden(name)
    ref64 = dict(zip(GRADS, (g.out, g.dq, g.dk, g.dv)))
    got = dict(zip(GRADS, causal_grads(g.q, g.k, g.v, g.kv_mask, g.cot, torch.float32, form="scan")))
    for k in GRADS:
        assert got[k].dtype == g.f32[k].dtype == torch.float32
        e_scan, e_fn = err(got[k], ref64[k]), err(g.f32[k], ref64[k])
        print(f"{name} {k}: scan form {e_scan:.2e}, reference function {e_fn:.2e}, ratio {e_scan / e_fn:.2f}")
        assert 0.5 * e_fn <= e_scan <= 2 * e_fn, k


def test_fixture_files_are_small_arrays():
    import numpy as np
    files = sorted(os.listdir(CAUSAL_DIR))
    assert "decoder_state_dict.json" in files
    for f in files:
        assert os.path.getsize(os.path.join(CAUSAL_DIR, f)) < 200 * 1000, f
        if f.endswith(".npz"):
            z = np.load(os.path.join(CAUSAL_DIR, f), allow_pickle=False)
            assert all(z[k].dtype.kind in "fu" for k in z.files), f


def test_decoder_state_dict_is_the_reference():
    import galerkin_transformer as gt
    import libs
    import libs.model
    assert libs.model.GalerkinTransformerDecoderLayer is gt.GalerkinTransformerDecoderLayer is libs.GalerkinTransformerDecoderLayer
    want = decoder_state_dict_shapes()
    layer = gt.GalerkinTransformerDecoderLayer(64, 2)
    got = {k: list(v.shape) for k, v in layer.state_dict().items()}
    assert got == want
    assert "linear2.weight" in got and "norm3.weight" in got                     # the unused linear2; norms with layer_norm
    assert got["self_attn.fc.weight"] == got["multihead_attn.fc.weight"] == [64, 66]
    assert layer.self_attn.attention_type == "galerkin" and layer.multihead_attn.attention_type == "causal"
    res = layer.load_state_dict({k: torch.zeros(s) for k, s in want.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    bare = gt.GalerkinTransformerDecoderLayer(64, 2, layer_norm=False)
    assert not any(k.startswith("norm") for k in bare.state_dict())
    normed = gt.GalerkinTransformerDecoderLayer(64, 2, attn_norm=True)
    keys = set(normed.state_dict())
    assert {"self_attn.norm_K.0.weight", "self_attn.norm_V.1.bias", "multihead_attn.norm_Q.0.weight",
            "multihead_attn.norm_K.1.bias"} <= keys
    assert not any(k.startswith("multihead_attn.norm_V") or k.startswith("self_attn.norm_Q") for k in keys)
    assert normed.multihead_attn._norm_pair()[2] == 0b011


def test_causal_is_a_kind_of_its_own():
    import galerkin_transformer as gt
    from galerkin_transformer import layers, model
    assert "causal" not in layers._HIP_ATTENTION
    assert layers._CAUSAL_ATTENTION == ("causal",)
    assert "causal" not in model._ConfiguredModel._hip_attention
    from test_softmax_attention_cpu import LITE
    with pytest.raises(NotImplementedError):
        gt.FourierTransformer2DLite(attention_type="causal", **LITE)


def test_refusals_before_any_launch():
    import galerkin_transformer as gt
    from galerkin_transformer import ops
    attn = gt.SimpleAttention(n_head=2, d_model=64, attention_type="causal", pos_dim=1)
    x, mem = torch.rand(2, 8, 64), torch.rand(2, 8, 64)
    keep = torch.ones(2, 8, dtype=torch.bool)
    for call in (lambda: attn(x, x, x), lambda: attn(x, mem, mem), lambda: attn(x, x, x, pos=torch.rand(2, 8, 1)),
                 lambda: attn(x, mem, mem, mask=keep)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(AssertionError):
        attn(x, torch.rand(2, 9, 64), torch.rand(2, 9, 64)[:, :9])          # key is not value, n_q != n_kv
    m9 = torch.rand(2, 9, 64)
    with pytest.raises(AssertionError):
        attn(x, m9, m9)
    for bad in (torch.ones(2, 8), torch.ones(2, 8, dtype=torch.uint8), [[True] * 8] * 2):
        with pytest.raises(TypeError):
            attn(x, mem, mem, mask=bad)
        with pytest.raises(TypeError):
            attn(x, x, x, mask=bad)
    for shape in ((2, 1, 8), (2, 9), (8,)):                                  # not unsqueezed, [B, n_kv] exactly
        with pytest.raises(AssertionError):
            attn(x, mem, mem, mask=torch.ones(shape, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        attn(x, x, x, weight=torch.ones(2, 8, 1))
    # d_k = 40 has no kernel: refused before the device is asked for
    with pytest.raises(NotImplementedError, match="no kernel"):
        gt.SimpleAttention(n_head=2, d_model=80, attention_type="causal")(torch.rand(1, 8, 80), torch.rand(1, 8, 80),
                                                                          torch.rand(1, 8, 80))
    x80, m80 = torch.rand(1, 8, 80), torch.rand(1, 8, 80)
    with pytest.raises(NotImplementedError, match="no kernel"):
        gt.GalerkinTransformerDecoderLayer(80, 2).multihead_attn(x80, m80, m80)
    # the operator on [B, h, n, D]
    q = torch.rand(2, 2, 8, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.causal_linear_attention(q, q, q)
    with pytest.raises(NotImplementedError, match="no kernel"):
        ops.causal_linear_attention(q[..., :8], q[..., :8], q[..., :8])
    with pytest.raises(TypeError):
        ops.causal_linear_attention(q, q, q, kv_mask=torch.ones(2, 8))
    with pytest.raises(AssertionError):
        ops.causal_linear_attention(q, q, q, kv_mask=torch.ones(2, 1, 8, dtype=torch.bool))
    with pytest.raises(AssertionError):
        ops.causal_linear_attention(q, q[:, :, :7], q)


def test_decoder_refusals():
    import galerkin_transformer as gt
    x, mem = torch.rand(2, 8, 64), torch.rand(2, 8, 64)
    keep = torch.ones(2, 8, dtype=torch.bool)
    dec = gt.GalerkinTransformerDecoderLayer(64, 2).eval()
    with pytest.raises(RuntimeError, match="casual mask"):
        dec(x, mem, tgt_mask=keep)
    with pytest.raises(NotImplementedError):
        gt.GalerkinTransformerDecoderLayer(64, 2, attention_type="fourier")(x, mem, tgt_mask=keep)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec(x, mem)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec(x, mem, memory_mask=keep)


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    assert "#define GT_ABI_VERSION 21" in hdr
    lib = ctypes.CDLL(_hip.lib_path())
    for s in NEW_SYMBOLS:
        assert " " + s + "(" in hdr, s
        assert s in _hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert _hip.lib().gt_abi_version() == 21 and _hip.ABI_VERSION == 21
    assert sorted(_hip.CAUSAL_DP) == [16, 20, 32, 36, 48, 52, 64, 68, 96, 100]
    L = _hip.lib()
    for DP in _hip.CAUSAL_DP:                       # ceil(130 / 64) = 3 chunks of (DP^2 + DP) floats per (sample, head)
        assert L.gt_causal_attn_state_bytes(2, 130, 3, DP) == 4 * 2 * 3 * 3 * (DP * DP + DP)
        assert L.gt_causal_attn_bwd_ws_bytes(2, 130, 3, DP) == 4 * 2 * 3 * 3 * (DP * DP + DP) + 4 * 2 * 3 * 130
    for DP in (8, 24, 40, 44, 72, 80, 104):         # never a nearest instance: the size queries answer 0 ...
        assert L.gt_causal_attn_state_bytes(2, 130, 3, DP) == 0 and L.gt_causal_attn_bwd_ws_bytes(2, 130, 3, DP) == 0
        # ... and the entry points GT_ENOTSUP, from the arguments alone (nothing is dereferenced or launched)
        assert L.gt_causal_attn_fwd(None, None, None, None, None, None, 2, 130, 3, DP, 1e-7, None, 0, None) == -4
        assert L.gt_causal_attn_bwd(*([None] * 11), 2, 130, 3, DP, DP, 1e-7, None, 0, None) == -4
        with pytest.raises(NotImplementedError, match="no kernel"):
            _hip.causal_check(DP)
