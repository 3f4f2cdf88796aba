"""norm_type='instance' (token-axis norm of K, V), CPU side: the plain-torch restatement (tests/_instance_ref.py) against
the fixtures recorded from the reference (tests/golden/instance/), its float32-vs-float64 envelope, and the host-visible
surface of the feature (exported symbols, module construction, checkpoint keys).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _instance_ref import (FAMILY, INSTANCE_GOLDEN, SHARED_INPUTS, attention_type_of, grad_errors, ref_grads,
                           zero_grad_params)
from _util import GOLDEN, Golden, rel_l2

REF_TOL = 2e-6      # the bar of test_oracle_golden.py: fp32 round-off between two orderings of the same math
NEW_SYMBOLS = ("gt_token_norm_ws_bytes", "gt_token_norm_fwd", "gt_token_norm_bwd")


@pytest.mark.parametrize("name", INSTANCE_GOLDEN)
def test_restatement_matches_reference_golden(name):
    g = Golden("instance/" + name)
    out, din, dparam = ref_grads(g, torch.float32)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(v, g.din[k]) for k, v in din.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dparam, g.dparam, g.sd, attention_type_of(g)).items()})
    print(name, {k: f"{v:.1e}" for k, v in errs.items() if v > 0.5 * REF_TOL})
    assert errs["out"] < REF_TOL, errs["out"]
    bad = {k: v for k, v in errs.items() if k != "out" and not v < 5 * REF_TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", INSTANCE_GOLDEN)
def test_restatement_fp64_envelope(name):
    """float32 restatement vs the float64 one: the numerical envelope the HIP path is judged in (the figures the GPU test's
    docstring quotes come from here)."""
    g = Golden("instance/" + name)
    at = attention_type_of(g)
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    errs = {"out": rel_l2(o32, o64)}
    errs.update({"d" + k: rel_l2(v, di64[k]) for k, v in di32.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, g.sd, at).items()})
    worst = max(errs, key=errs.get)
    over = {k: f"{v:.1e}" for k, v in errs.items() if v > 2e-6}
    print(f"{name}: out {errs['out']:.2e}, worst {worst} {errs[worst]:.2e}, above 2e-6: {over}")
    assert errs["out"] < 1e-6, errs["out"]                 # the bar of test_oracle_fp64_envelope
    # gradients: a sanity ceiling of 1e3 x eps as in test_linear_attention_cpu.py, not a parity bar; the figures are printed
    assert errs[worst] < 6e-5, (worst, errs[worst])


def test_zero_gradient_parameters_are_zero_in_float64():
    """The parameters grad_errors() measures absolutely really have a vanishing gradient: in float64 it is round-off of
    the sibling weight's gradient (the reasoning is in _instance_ref.zero_grad_params)."""
    for name, expect in (("enc_galerkin_inst_c2", 2), ("enc_linear_inst_c2", 2 + 4), ("enc_global_inst_c5", 2 + 1),
                         ("model_burgers_galerkin_inst_small", None)):
        g = Golden("instance/" + name)
        zero = zero_grad_params(g.sd, attention_type_of(g))
        assert zero and (expect is None or len(zero) == expect), zero
        _, _, dp64 = ref_grads(g, torch.float64)
        for k in zero:
            assert float(dp64[k].norm()) < 1e-12 * float(dp64[k[:-len("bias")] + "weight"].norm()), k


def test_fixtures_hold_arrays_only():
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "instance")) if f.endswith(".npz"))
    assert files == sorted(n + ".npz" for n in INSTANCE_GOLDEN + SHARED_INPUTS)
    for f in files:
        path = os.path.join(GOLDEN, "instance", f)
        assert os.path.getsize(path) < (1 << 20), f
        z = np.load(path, allow_pickle=False)
        for k in z.files:
            assert k == "meta" or k in ("out", "cot") or k.split("/")[0] in ("sd", "in", "din", "dparam", "mask"), (f, k)
            assert z[k].dtype.kind in "fiub", (f, k, z[k].dtype)
        meta = json.loads(bytes(z["meta"]).decode())
        cfg = meta if "attention_type" in meta else meta["config"]
        assert cfg["attention_type"] in FAMILY and cfg["norm_type"] == "instance"


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    lib = ctypes.CDLL(_hip.lib_path())
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in _hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert _hip.lib().gt_abi_version() == 21 and _hip.ABI_VERSION == 21
    # the workspace query is host code: positive for the head sizes of the Galerkin path, 0 for the others
    q = _hip.lib().gt_token_norm_ws_bytes
    for dk, p in ((16, 1), (32, 2), (48, 2), (64, 0), (96, 2)):
        assert q(4, 1849, 4, dk, p) > 0 and q(128, 1849, 4, dk, p) > 0
    assert q(4, 1849, 4, 40, 2) == 0 and q(4, 1849, 4, 32, 3) == 0
    # one (mean, M2) pair of column groups per chunk of at least 32 and at most 128 tokens, plus one pair per sample
    C4 = 4 * 36 // 4
    assert (4 * 15 + 4) * 2 * C4 * 16 <= q(4, 1849, 4, 32, 2) <= (4 * 58 + 4) * 2 * C4 * 16
    assert q(128, 1849, 4, 32, 2) == (128 * 15 + 128) * 2 * C4 * 16


@pytest.mark.parametrize("at", FAMILY)
def test_instance_layers_construct_and_reach_the_hip_operator(at):
    import galerkin_transformer as gt
    layer = gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type=at, layer_norm=False,
                                             norm_type="instance", norm_eps=1e-6)
    a = layer.attn
    assert not hasattr(a, "norm_Q") and len(a.norm_K) == 4 and len(a.norm_V) == 4
    for m in list(a.norm_K) + list(a.norm_V):
        assert type(m) is torch.nn.InstanceNorm1d and m.affine and not m.track_running_stats and m.eps == 1e-6
        assert m.num_features == 16 and not list(m.buffers())
        assert torch.equal(m.weight, torch.ones(16)) and torch.equal(m.bias, torch.zeros(16))
    ref = gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type=at, layer_norm=False)
    assert {k: v.shape for k, v in layer.state_dict().items()} == {k: v.shape for k, v in ref.state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # reaches the HIP operator, not NotImplementedError
        layer(torch.randn(1, 8, 64), torch.rand(1, 8, 2))


@pytest.mark.parametrize("at", ("fourier", "integral", "local"))
def test_fourier_family_with_instance_still_raises(at):
    import galerkin_transformer as gt
    with pytest.raises(NotImplementedError, match="instance"):
        gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type=at, layer_norm=False,
                                         norm_type="instance")
    with pytest.raises(NotImplementedError):
        gt.SimpleAttention(4, 64, pos_dim=2, attention_type=at, norm=True, norm_type="batch")


def test_models_construct_and_load_instance_state_dict():
    """The three model classes accept norm_type='instance'; the reference's state_dict of the Burgers fixture loads strictly."""
    import galerkin_transformer as gt
    g = Golden("instance/model_burgers_galerkin_inst_small")
    assert g.meta["config"]["norm_type"] == "instance"
    m = gt.SimpleTransformer(**g.meta["config"])
    res = m.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    norms = [x for x in m.modules() if isinstance(x, torch.nn.InstanceNorm1d)]
    assert norms and not any(isinstance(x, torch.nn.LayerNorm) for n_, x in m.named_modules() if ".norm_K." in n_)
    lite = dict(dropout=0.0, encoder_dropout=0.0, decoder_dropout=0.0, ffn_dropout=0.0, xavier_init=0.01,
                diagonal_weight=0.01, node_feats=12, pos_dim=2, n_targets=1, n_hidden=32, num_encoder_layers=1, n_head=2,
                dim_feedforward=64, layer_norm=False, attn_norm=True, decoder_type="ifft2", freq_dim=12,
                num_regressor_layers=1, fourier_modes=4, spacial_dim=2, spacial_fc=False, regressor_activation="silu",
                debug=False, norm_type="instance")
    for at in FAMILY:
        ml = gt.FourierTransformer2DLite(attention_type=at, **lite)
        assert any(isinstance(x, torch.nn.InstanceNorm1d) for x in ml.modules())
        ms = gt.SimpleTransformer(**dict(g.meta["config"], attention_type=at))
        assert any(isinstance(x, torch.nn.InstanceNorm1d) for x in ms.modules())
    # FourierTransformer2D: the reference does not hand norm_type to this model's encoder layers (its _get_encoder,
    # model.py:1125-1142, leaves the argument out), so they keep the per-head LayerNorm whatever the config says
    g2 = Golden("model_darcy_small")
    cfg = dict(g2.meta["config"], norm_type="instance")
    for k in ("downscaler_size", "upscaler_size"):
        if cfg.get(k) is not None:
            cfg[k] = tuple(tuple(s) if isinstance(s, list) else s for s in cfg[k])
    md = gt.FourierTransformer2D(**cfg)
    assert md.load_state_dict(g2.sd, strict=True) is not None
    assert not any(isinstance(x, torch.nn.InstanceNorm1d) for x in md.modules())
