"""attention_type='softmax', CPU side: the plain-torch restatement (tests/_softmax_ref.py) against the fixtures recorded
from the reference (tests/golden/softmax/), its float32-vs-float64 envelope, the host-visible surface of the feature
(exported symbols, accepted attention types, state_dict keys) and a lane-accurate model of one forward wave.  No GPU needed."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from _softmax_ref import SOFTMAX_GOLDEN, grad_errors, ref_grads, run_ref, zero_grad_params
from _util import GOLDEN, Golden, rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mfma_sim as S  # noqa: E402

REF_TOL = 2e-6      # the bar of test_oracle_golden.py: fp32 round-off between two orderings of the same math
NEW_SYMBOLS = ("gt_softmax_attn_fwd", "gt_softmax_attn_bwd_q", "gt_softmax_attn_bwd_kv", "gt_row_softmax_fwd",
               "gt_row_softmax_bwd")
LITE = dict(dropout=0.0, encoder_dropout=0.0, decoder_dropout=0.0, ffn_dropout=0.0, xavier_init=0.01, diagonal_weight=0.01,
            node_feats=12, pos_dim=2, n_targets=1, n_hidden=32, num_encoder_layers=1, n_head=2, dim_feedforward=64,
            layer_norm=True, attn_norm=False, decoder_type="ifft2", freq_dim=12, num_regressor_layers=1, fourier_modes=4,
            spacial_dim=2, spacial_fc=False, regressor_activation="silu", debug=False)


@pytest.mark.parametrize("name", SOFTMAX_GOLDEN)
def test_restatement_matches_reference_golden(name):
    g = Golden("softmax/" + name)
    out, din, dparam = ref_grads(g, torch.float32)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(v, g.din[k]) for k, v in din.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dparam, g.dparam, g.sd).items()})
    assert errs["out"] < REF_TOL, errs["out"]
    bad = {k: v for k, v in errs.items() if k != "out" and not v < 5 * REF_TOL}
    assert not bad, bad


def test_restatement_returns_the_recorded_weights():
    g = Golden("softmax/enc_softmax_weights")
    attn = torch.from_numpy(np.load(os.path.join(GOLDEN, "softmax", "enc_softmax_weights.npz"))["attn"])
    _, w = run_ref(g, g.sd, g.inputs, return_attn=True)
    assert w.shape == attn.shape == (2, 4, 70, 70)
    assert rel_l2(w, attn) < REF_TOL
    assert torch.allclose(attn.sum(-1), torch.ones(2, 4, 70), atol=1e-5)


@pytest.mark.parametrize("name", SOFTMAX_GOLDEN)
def test_restatement_fp64_envelope(name):
    """float32 restatement vs the float64 one: the numerical envelope the HIP path is judged in (the figures the GPU test's
    docstring quotes come from here)."""
    g = Golden("softmax/" + name)
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    errs = {"out": rel_l2(o32, o64)}
    errs.update({"d" + k: rel_l2(v, di64[k]) for k, v in di32.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, g.sd).items()})
    worst = max(errs, key=errs.get)
    over = {k: f"{v:.1e}" for k, v in errs.items() if v > 2e-6}
    print(f"{name}: out {errs['out']:.2e}, worst {worst} {errs[worst]:.2e}, above 2e-6: {over}")
    assert errs["out"] < 1e-6, errs["out"]                 # the bar of test_oracle_fp64_envelope
    # gradients: float32 round-off (6e-8) times the cancellation in the softmax backward (dS = P (dP - <P, dP>)); the
    # figures are reported above, the bound is a sanity ceiling of 1e3 x eps, not a parity bar
    assert errs[worst] < 6e-5, (worst, errs[worst])


def test_zero_gradient_parameters_are_zero_in_float64():
    """A constant added to every key shifts each score row uniformly: the bias in front of K' has a vanishing gradient."""
    for name, expect in (("enc_softmax_c2", 4), ("enc_softmax_c4_ln", 1), ("model_burgers_softmax_small", None)):
        g = Golden("softmax/" + name)
        zero = zero_grad_params(g.sd)
        assert zero and (expect is None or len(zero) == expect), zero
        _, _, dp64 = ref_grads(g, torch.float64)
        for k in zero:
            assert float(dp64[k].norm()) < 1e-12 * float(dp64[k[:-len("bias")] + "weight"].norm()), k


def test_fixtures_hold_arrays_only():
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "softmax")) if f.endswith(".npz"))
    assert len(files) == len(SOFTMAX_GOLDEN) + 2           # + the shared weights / inputs of the c2 and c4_ln pairs
    for f in files:
        path = os.path.join(GOLDEN, "softmax", f)
        assert os.path.getsize(path) < (1 << 20), f
        z = np.load(path, allow_pickle=False)
        for k in z.files:
            assert k in ("meta", "out", "cot", "attn") or k.split("/")[0] in ("sd", "in", "din", "dparam", "mask"), (f, k)
            assert z[k].dtype.kind in "fiub", (f, k, z[k].dtype)
        meta = json.loads(bytes(z["meta"]).decode())
        assert (meta.get("attention_type") or meta["config"]["attention_type"]) == "softmax"


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
    assert _hip.SOFTMAX_DP == (20, 36, 52)


def test_softmax_layers_and_models_construct():
    """attention_type='softmax' builds in the layer and in the three model classes, with the reference's parameters."""
    import galerkin_transformer as gt
    from galerkin_transformer import model
    assert "softmax" in model._ConfiguredModel._hip_attention
    layer = gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type="softmax", layer_norm=False)
    assert hasattr(layer.attn, "norm_Q") and hasattr(layer.attn, "norm_K") and not hasattr(layer.attn, "norm_V")
    assert layer.dropout1.p == 0.1                         # forced for 'linear' / 'softmax' (reference model.py:65-66)
    g = Golden("softmax/model_burgers_softmax_small")
    gt.SimpleTransformer(**g.meta["config"])
    gt.FourierTransformer2DLite(attention_type="softmax", **LITE)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    cfg = dict(bench.darcy_config("ex2_darcy141"), attention_type="softmax")
    gt.FourierTransformer2D(**cfg)


@pytest.mark.parametrize("name", ("enc_softmax_c2", "enc_softmax_c4_ln", "model_burgers_softmax_small"))
def test_state_dict_keys_are_the_references(name):
    from test_modules_gpu import build_module
    import galerkin_transformer as gt
    g = Golden("softmax/" + name)
    mod = build_module(gt, g)
    own = mod.state_dict()
    assert set(own) == set(g.sd)
    for k, v in g.sd.items():
        assert own[k].shape == v.shape, k
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    attn = [k for k in own if ".norm_" in k or k.startswith("attn.norm_")]
    assert all("norm_V" not in k for k in attn)
    if (g.meta.get("attn_norm") if g.meta["kind"] == "encoder_layer" else False):
        assert any("norm_Q" in k for k in attn) and any("norm_K" in k for k in attn)


def test_cpu_call_reaches_the_operator():
    import galerkin_transformer as gt
    layer = gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type="softmax", layer_norm=False)
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:        # the HIP operator, not NotImplementedError
        layer(torch.randn(1, 8, 64), torch.rand(1, 8, 2))
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(NotImplementedError):
        layer.attn(torch.randn(1, 8, 64), None, None, mask=torch.ones(1, 8, 8))


def test_coordinate_free_softmax_is_refused_before_any_parameter_is_touched():
    import galerkin_transformer as gt
    layer = gt.SimpleTransformerEncoderLayer(d_model=32, n_head=2, attention_type="softmax")
    with pytest.raises(NotImplementedError, match="without coordinates"):
        layer(torch.randn(1, 8, 32))
    nop = gt.SimpleTransformerEncoderLayer(d_model=32, n_head=2, pos_dim=0, attention_type="softmax")
    with pytest.raises(NotImplementedError, match="without coordinates"):
        nop(torch.randn(1, 8, 32), torch.rand(1, 8, 0))


def test_forward_wave_lane_model():
    """softmax_core_kernel<5, SM_FWD> (gt_softmax.hip), one wave, DP 20, n = 70: two stream tiles, the second partial.  The
    score tile's row / column map, the row reduction (16 in-lane registers, then lanes xor 16 and xor 32), the exclusion of
    the zero-filled rows >= n from the maximum and the sum, and the rescale of the accumulators, against plain softmax
    attention."""
    KS, n = 5, 70
    DP, NF, XC = 4 * KS, (4 * KS - 4) // 16, 4 * KS - 4
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((32, DP))                  # 32 owner rows (queries) of the wave
    K, V = rng.standard_normal((n, DP)) * 2.0, rng.standard_normal((n, DP))
    K[64:] += 3.0                                      # the rows of the partial tile carry the maximum of some queries
    scale = 1.0 / np.sqrt(DP - 2)
    j, kq = S.X, S.KQ
    lanes = np.arange(64)

    def xor(v, o):                                     # __shfl_xor(v, o, 64)
        return v[lanes ^ o]

    f1 = [[scale * Q[16 * nt + j, 4 * s + kq] for s in range(KS)] for nt in range(2)]
    acc1 = [[np.zeros((64, 4)) for _ in range(2)] for _ in range(NF)]
    ax = np.zeros((2, 64, 4))
    run_m, run_l = np.full((2, 64), -np.inf), np.zeros((2, 64))
    for s0 in range(0, n, 64):
        t1 = np.zeros((64, DP)); t2 = np.zeros((64, DP))
        rows = min(64, n - s0)
        t1[:rows], t2[:rows] = K[s0:s0 + rows], V[s0:s0 + rows]
        sa = [[np.zeros((64, 4)) for _ in range(2)] for _ in range(4)]
        for s in range(KS):
            for mt in range(4):
                a1 = t1[16 * mt + j, 4 * s + kq]
                for nt in range(2):
                    sa[mt][nt] = S.mfma(a1, f1[nt][s], sa[mt][nt])
        for mt in range(4):
            for r in range(4):
                dead = s0 + 16 * mt + 4 * kq + r >= n
                for nt in range(2):
                    assert np.all(sa[mt][nt][dead, r] == 0.0)      # zero-filled rows score 0, not -inf ...
                    sa[mt][nt][dead, r] = -np.inf                  # ... and are taken out explicitly
        for nt in range(2):
            mx = np.max(np.stack([sa[mt][nt] for mt in range(4)]), axis=(0, 2))
            mx = np.maximum(mx, xor(mx, 16)); mx = np.maximum(mx, xor(mx, 32))
            mnew = np.maximum(run_m[nt], mx)
            alpha = np.exp(run_m[nt] - mnew)
            run_m[nt] = mnew
            tot = np.zeros(64)
            for mt in range(4):
                sa[mt][nt] = np.exp(sa[mt][nt] - mnew[:, None])
                tot += sa[mt][nt].sum(axis=1)
            tot = tot + xor(tot, 16); tot = tot + xor(tot, 32)
            run_l[nt] = run_l[nt] * alpha + tot
            for dt in range(NF):
                acc1[dt][nt] *= alpha[:, None]
            ax[nt] *= alpha[:, None]
        for mt in range(4):
            for s in range(4):
                row = 16 * mt + 4 * kq + s
                for dt in range(NF):
                    a = t2[row, 16 * dt + j]
                    for nt in range(2):
                        acc1[dt][nt] = S.mfma(a, sa[mt][nt][:, s], acc1[dt][nt])
                x1 = t2[row, XC:XC + 4]
                for nt in range(2):
                    ax[nt] += sa[mt][nt][:, s][:, None] * x1
    O = np.full((32, DP), np.nan)
    L = np.full(32, np.nan)
    for l in range(64):
        for nt in range(2):
            ow = 16 * nt + j[l]
            for dt in range(NF):
                O[ow, 16 * dt + 4 * kq[l]:16 * dt + 4 * kq[l] + 4] = acc1[dt][nt][l] / run_l[nt][l]
            if kq[l] == 0:
                O[ow, XC:XC + 4] = sum(ax[nt][j[l] + 16 * q] for q in range(4)) / run_l[nt][l]
                L[ow] = run_m[nt][l] + np.log(run_l[nt][l])
    Sc = (Q @ K.T) * scale
    P = np.exp(Sc - Sc.max(axis=1, keepdims=True))
    P /= P.sum(axis=1, keepdims=True)
    assert (Sc.argmax(axis=1) >= 64).any() and (Sc.argmax(axis=1) < 64).any()      # both tiles hold some row's maximum
    assert np.allclose(O, P @ V, atol=1e-12)
    assert np.allclose(L, np.log(np.exp(Sc - Sc.max(axis=1, keepdims=True)).sum(axis=1)) + Sc.max(axis=1), atol=1e-12)
