"""attention_type='official' (the classic Transformer encoder layer), CPU side: the plain-torch restatement
(tests/_official_ref.py) against the fixtures recorded from the reference (tests/golden/official/), its float32-vs-float64
envelope, state_dict keys, the refusals and ignored arguments of the modules, and the host-visible surface of the three new
kernels.  No GPU needed.

Deviation of the float32 restatement from float64 (test_restatement_fp64_envelope prints them): output at most 1.4e-07
(wrapper_official_2), largest tensor per fixture
    enc_official_d64h4 4.3e-07, enc_official_d128h4 4.9e-07, enc_official_d96h2_pos 3.8e-07, enc_official_d64h1 4.2e-07,
    enc_official_d96h1 4.5e-07 (all dW:self_attn.in_proj_weight), enc_official_weights 3.7e-07, wrapper_official_2 3.5e-07,
    model_burgers_official_small 3.8e-07 (all d(out_proj.weight)); no tensor above 2e-6."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _official_ref import OFFICIAL_GOLDEN, SUB, build_module, ref_grads, run_ref
from _util import GOLDEN, Golden, rel_l2

REF_TOL = 2e-6      # the bar of test_oracle_golden.py: fp32 round-off between two orderings of the same math
NEW_SYMBOLS = ("gt_softmax_attn_nopos_fwd", "gt_softmax_attn_nopos_bwd_q", "gt_softmax_attn_nopos_bwd_kv")


def _errors(got, ref):
    (o, di, dp), (ro, rdi, rdp) = got, ref
    errs = {"out": rel_l2(o, ro)}
    errs.update({"d" + k: rel_l2(v, rdi[k]) for k, v in di.items()})
    errs.update({"dW:" + k: rel_l2(v, rdp[k]) for k, v in dp.items()})
    return errs


@pytest.mark.parametrize("name", OFFICIAL_GOLDEN)
def test_state_dict_keys_and_strict_load(name):
    import galerkin_transformer as gt
    g = Golden(SUB + name)
    mod = build_module(gt, g)
    assert set(mod.state_dict()) == set(g.sd)
    for k, v in mod.state_dict().items():
        assert tuple(v.shape) == tuple(g.sd[k].shape), k
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # every parameter has a recorded gradient, except the two norms that layer_norm=False leaves unused
    unused = set(dict(mod.named_parameters())) - set(g.dparam)
    assert set(g.dparam) <= set(dict(mod.named_parameters()))
    layer_norm = g.meta["layer_norm"] if "layer_norm" in g.meta else g.meta["config"]["layer_norm"]
    assert bool(unused) == (not layer_norm)
    assert all(k.split(".")[-2] in ("norm1", "norm2") for k in unused), unused


def test_layer_keys_are_the_reference_names():
    import galerkin_transformer as gt
    layer = gt._TransformerEncoderLayer(64, 4, dim_feedforward=128, layer_norm=False)
    assert sorted(layer.state_dict()) == sorted(
        ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
         "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
         "norm2.bias"])                                              # the two norms exist even with layer_norm=False
    assert tuple(layer.self_attn.in_proj_weight.shape) == (192, 64)
    assert isinstance(layer.self_attn, torch.nn.MultiheadAttention) and layer.self_attn.dropout == 0.1
    import libs
    import libs.model
    assert libs.model._TransformerEncoderLayer is gt._TransformerEncoderLayer is libs._TransformerEncoderLayer
    assert libs.model.TransformerEncoderWrapper is gt.TransformerEncoderWrapper is libs.TransformerEncoderWrapper
    wrap = gt.TransformerEncoderWrapper(layer, 3)
    assert len(wrap.layers) == 3 and wrap.norm is None and all(m is not layer for m in wrap.layers)


@pytest.mark.parametrize("name", OFFICIAL_GOLDEN)
def test_restatement_matches_reference_golden(name):
    g = Golden(SUB + name)
    got = ref_grads(g, torch.float32)
    assert got[0].shape == g.out.shape
    errs = _errors(got, (g.out, g.din, g.dparam))
    assert errs["out"] < REF_TOL, errs["out"]
    bad = {k: v for k, v in errs.items() if k != "out" and not v < 5 * REF_TOL}
    assert not bad, bad


def test_restatement_returns_the_recorded_weights():
    g = Golden(SUB + "enc_official_weights")
    attn = torch.from_numpy(np.load(os.path.join(GOLDEN, "official", "enc_official_weights.npz"))["attn"])
    _, w = run_ref(g, g.sd, g.inputs, return_attn=True)
    assert w.shape == attn.shape == (2, 70, 70)
    assert rel_l2(w, attn) < REF_TOL
    assert torch.allclose(attn.sum(-1), torch.ones(2, 70), atol=1e-5)


@pytest.mark.parametrize("name", OFFICIAL_GOLDEN)
def test_restatement_fp64_envelope(name):
    """float32 restatement vs the float64 one: the numerical envelope the GPU bars use (module docstring)."""
    g = Golden(SUB + name)
    errs = _errors(ref_grads(g, torch.float32), ref_grads(g, torch.float64))
    worst = max(errs, key=errs.get)
    over = {k: f"{v:.1e}" for k, v in errs.items() if v > 2e-6}
    print(f"{name}: out {errs['out']:.2e}, worst {worst} {errs[worst]:.2e}, above 2e-6: {over}")
    assert errs["out"] < 1e-6, errs["out"]                 # the bar of test_oracle_fp64_envelope
    assert errs[worst] < 6e-5, (worst, errs[worst])        # a sanity ceiling of 1e3 x eps, not a parity bar


def test_fixtures_hold_arrays_only():
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "official")) if f.endswith(".npz"))
    assert len(files) == len(OFFICIAL_GOLDEN) + 1          # + the shared weights / inputs of enc_official_d128h4
    for f in files:
        path = os.path.join(GOLDEN, "official", f)
        assert os.path.getsize(path) < (1 << 20), f
        z = np.load(path, allow_pickle=False)
        for k in z.files:
            assert k in ("meta", "out", "cot", "attn") or k.split("/")[0] in ("sd", "in", "din", "dparam"), (f, k)
            assert z[k].dtype.kind in "fiub", (f, k, z[k].dtype)
        meta = json.loads(bytes(z["meta"]).decode())
        assert meta["kind"].startswith("official_") or meta["config"]["attention_type"] == "official"


def test_models_build_and_refuse():
    import galerkin_transformer as gt
    from test_softmax_attention_cpu import LITE
    g = Golden(SUB + "model_burgers_official_small")
    m = gt.SimpleTransformer(**g.meta["config"])
    assert len(m.encoder_layers) == 2 and all(isinstance(e, gt._TransformerEncoderLayer) for e in m.encoder_layers)
    assert m.encoder_layers[0] is not m.encoder_layers[1]
    assert m.encoder_layers[0].self_attn.num_heads == 2 and m.encoder_layers[0].linear1.out_features == 64
    with pytest.raises(NotImplementedError):
        gt.FourierTransformer2DLite(attention_type="official", **LITE)
    import bench
    with pytest.raises(NotImplementedError):
        gt.FourierTransformer2D(**dict(bench.darcy_config("ex2_darcy141"), attention_type="official"))
    for other in ("performer", "transformer", "Official"):          # every other unknown name keeps raising
        with pytest.raises(NotImplementedError):
            gt.SimpleTransformer(**dict(g.meta["config"], attention_type=other))


def test_layer_refusals_and_ignored_arguments():
    import galerkin_transformer as gt
    layer = gt._TransformerEncoderLayer(64, 4, dim_feedforward=128)
    x = torch.randn(2, 8, 64)
    mask, kpm = torch.zeros(8, 8), torch.zeros(2, 8, dtype=torch.bool)
    with pytest.raises(NotImplementedError):
        layer(x, src_mask=mask, src_key_padding_mask=kpm)
    with pytest.raises(NotImplementedError):
        gt.TransformerEncoderWrapper(layer, 2)(x, mask=mask, src_key_padding_mask=kpm)
    with pytest.raises(AssertionError, match="was expecting embedding dimension of 64"):
        layer(x, torch.rand(2, 8, 1))                      # 1 + 64 != d_model
    # weight and one mask alone are ignored: the call reaches the operator, which has no CPU fallback
    for kw in (dict(weight=torch.ones(2, 8, 1)), dict(src_mask=mask), dict(src_key_padding_mask=kpm)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(x, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(x[..., :62], torch.rand(2, 8, 2))            # 2 + 62 = d_model: accepted
    # d_k = 40 has no kernel: refused before the device is asked for
    with pytest.raises(NotImplementedError, match="no kernel"):
        gt._TransformerEncoderLayer(80, 2, dim_feedforward=64)(torch.randn(1, 8, 80))
    # the model hands its encoders (x, pos, weight): with pos given the width assertion fires, as in the reference
    m = gt.SimpleTransformer(**Golden(SUB + "model_burgers_official_small").meta["config"])
    with pytest.raises(AssertionError, match="was expecting embedding dimension of 32"):
        m.encoder_layers[0](torch.randn(1, 16, 32), torch.rand(1, 16, 1), None)


def test_simple_attention_keeps_refusing_softmax_without_coordinates():
    import galerkin_transformer as gt
    attn = gt.SimpleAttention(n_head=4, d_model=64, attention_type="softmax", pos_dim=2)
    x = torch.randn(1, 8, 64)
    with pytest.raises(NotImplementedError, match="without coordinates"):
        attn(x, x, x)


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    lib = ctypes.CDLL(_hip.lib_path())
    for s in NEW_SYMBOLS:
        assert "int " + s + "(" in hdr, s
        assert s in _hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert _hip.lib().gt_abi_version() == 21 and _hip.ABI_VERSION == 21
    assert _hip.SOFTMAX_DP_NOPOS == (16, 32, 48, 64, 96)
    assert _hip.SOFTMAX_DP == (20, 36, 52) and _hip.SOFTMAX_DP_WIDE == (68, 100)
    for DP in _hip.SOFTMAX_DP_NOPOS:
        assert [_hip._softmax_entry(DP, t) for t in ("fwd", "bwd_q", "bwd_kv")] == list(NEW_SYMBOLS)
    assert _hip._softmax_entry(20, "bwd_q") == "gt_softmax_attn_bwd_q"
    assert _hip._softmax_entry(100, "fwd") == "gt_softmax_attn_wide_fwd" and _hip._softmax_entry(40, "fwd") == "gt_softmax_attn_fwd"
