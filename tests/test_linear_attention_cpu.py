"""'linear' / 'global' attention, CPU side: the plain-torch restatement (tests/_linear_ref.py) against the fixtures
recorded from the reference (tests/golden/linear/), its float32-vs-float64 envelope, and the host-visible surface of the
feature (exported symbols, accepted attention types).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _linear_ref import LINEAR_GOLDEN, grad_errors, ref_grads, zero_grad_params
from _util import GOLDEN, Golden, rel_l2

REF_TOL = 2e-6      # the bar of test_oracle_golden.py: fp32 round-off between two orderings of the same math
NEW_SYMBOLS = ("gt_feature_softmax_fwd", "gt_feature_softmax_bwd", "gt_token_softmax_ws_bytes", "gt_token_softmax_fwd",
               "gt_token_softmax_bwd")


@pytest.mark.parametrize("name", LINEAR_GOLDEN)
def test_restatement_matches_reference_golden(name):
    g = Golden("linear/" + name)
    out, din, dparam = ref_grads(g, torch.float32)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(v, g.din[k]) for k, v in din.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dparam, g.dparam, g.sd).items()})
    assert errs["out"] < REF_TOL, errs["out"]
    bad = {k: v for k, v in errs.items() if k != "out" and not v < 5 * REF_TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", LINEAR_GOLDEN)
def test_restatement_fp64_envelope(name):
    """float32 restatement vs the float64 one: the numerical envelope the HIP path is judged in (the figures the GPU test's
    docstring quotes come from here)."""
    g = Golden("linear/" + name)
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    errs = {"out": rel_l2(o32, o64)}
    errs.update({"d" + k: rel_l2(v, di64[k]) for k, v in di32.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, g.sd).items()})
    worst = max(errs, key=errs.get)
    over = {k: f"{v:.1e}" for k, v in errs.items() if v > 2e-6}
    print(f"{name}: out {errs['out']:.2e}, worst {worst} {errs[worst]:.2e}, above 2e-6: {over}")
    assert errs["out"] < 1e-6, errs["out"]                 # the bar of test_oracle_fp64_envelope
    # gradients: float32 round-off (6e-8) times the cancellation in the two softmax backwards (dX = Y (dY - <Y, dY>)); the
    # figures are reported above, the bound is a sanity ceiling of 1e3 x eps, not a parity bar
    assert errs[worst] < 6e-5, (worst, errs[worst])


def test_zero_gradient_parameters_are_zero_in_float64():
    """The parameters grad_errors() measures absolutely really have a vanishing gradient: in float64 it is round-off of
    the sibling weight's gradient (the reasoning is in _linear_ref.zero_grad_params)."""
    for name, expect in (("enc_linear_c2", 4), ("enc_global_c5_ln", 1), ("model_burgers_linear_small", None)):
        g = Golden("linear/" + name)
        zero = zero_grad_params(g.sd)
        assert zero and (expect is None or len(zero) == expect), zero
        _, _, dp64 = ref_grads(g, torch.float64)
        for k in zero:
            assert float(dp64[k].norm()) < 1e-12 * float(dp64[k[:-len("bias")] + "weight"].norm()), k


def test_fixtures_hold_arrays_only():
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "linear")) if f.endswith(".npz"))
    assert len(files) == len(LINEAR_GOLDEN) + 1          # + enc_linear_c2_in: the shared weights / inputs of the c2 pair
    for f in files:
        path = os.path.join(GOLDEN, "linear", f)
        assert os.path.getsize(path) < (1 << 20), f
        z = np.load(path, allow_pickle=False)
        for k in z.files:
            assert k == "meta" or k in ("out", "cot") or k.split("/")[0] in ("sd", "in", "din", "dparam", "mask"), (f, k)
            assert z[k].dtype.kind in "fiub", (f, k, z[k].dtype)
        meta = json.loads(bytes(z["meta"]).decode())
        at = meta.get("attention_type") or meta["config"]["attention_type"]
        assert at in ("linear", "global")


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    lib = ctypes.CDLL(_hip.lib_path())
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in _hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert _hip.lib().gt_abi_version() == 21
    # the workspace query is host code: sizes follow the chunking, unsupported head sizes report 0
    q = _hip.lib().gt_token_softmax_ws_bytes
    assert q(4, 1849, 4, 32, 2) == 4 * 15 * 2 * (4 * 36 // 4) * 16
    assert q(1, 1, 1, 16, 0) == 2 * 4 * 16
    assert q(4, 1849, 4, 40, 2) == 0 and q(4, 1849, 4, 32, 3) == 0
    assert _hip.linattn_supported(96, 2) and not _hip.linattn_supported(80, 2)


def test_linear_and_global_are_hip_attention_types():
    import galerkin_transformer as gt
    from galerkin_transformer import layers, model
    for at in ("linear", "global"):
        assert at in layers._HIP_ATTENTION and at in model._ConfiguredModel._hip_attention
        layer = gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type=at, layer_norm=False)
        assert hasattr(layer.attn, "norm_K") and hasattr(layer.attn, "norm_V") and not hasattr(layer.attn, "norm_Q")
        with pytest.raises(RuntimeError, match="no CPU fallback"):        # reaches the HIP operator, not NotImplementedError
            layer(torch.randn(1, 8, 64), torch.rand(1, 8, 2))
        with pytest.raises(RuntimeError, match="casual mask"):
            layer.attn(torch.randn(1, 8, 64), None, None, mask=torch.ones(1, 8, 8))
    for at in ("softmax", "cosine", "causal"):
        assert at not in layers._HIP_ATTENTION


def test_models_construct_and_load_linear_state_dict():
    """The three model classes accept both names; the reference's 'linear' state_dict of the Burgers fixture loads strictly."""
    import galerkin_transformer as gt
    g = Golden("linear/model_burgers_linear_small")
    m = gt.SimpleTransformer(**g.meta["config"])
    res = m.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    lite = dict(dropout=0.0, encoder_dropout=0.0, decoder_dropout=0.0, ffn_dropout=0.0, xavier_init=0.01,
                diagonal_weight=0.01, node_feats=12, pos_dim=2, n_targets=1, n_hidden=32, num_encoder_layers=1, n_head=2, dim_feedforward=64,
                layer_norm=True, attn_norm=False, decoder_type="ifft2", freq_dim=12, num_regressor_layers=1,
                fourier_modes=4, spacial_dim=2, spacial_fc=False, regressor_activation="silu", debug=False)
    for at in ("linear", "global"):
        gt.FourierTransformer2DLite(attention_type=at, **lite)
        gt.SimpleTransformer(**dict(g.meta["config"], attention_type=at))
