"""The 'conv' scaler modes, CPU side: the plain-torch restatement (tests/_scaler_conv_ref.py) against the fixtures recorded
from the reference (tests/golden/scaler_conv/), its float32-vs-float64 envelope, the module trees DownScaler / UpScaler
build by default, the transposed convolution's size rule and the host-visible surface of the feature (exported symbols,
what keeps raising).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _scaler_conv_ref import SCALER_GOLDEN, all_errors, ref_grads
from _util import GOLDEN, Golden

REF_TOL = 2e-6      # the bar of test_oracle_golden.py: fp32 round-off between two orderings of the same math
NEW_SYMBOLS = ("gt_avgpool2_act_fwd", "gt_avgpool2_act_bwd", "gt_deconv3x3s2_check", "gt_deconv3x3s2_gather_fwd",
               "gt_deconv3x3s2_gather_bwd", "gt_deconv3x3s2_dbias", "gt_deconv3x3s2_dbias_ws_bytes")


@pytest.mark.parametrize("name", SCALER_GOLDEN)
def test_restatement_matches_reference_golden(name):
    g = Golden("scaler_conv/" + name)
    out, dx, dparam = ref_grads(g, torch.float32)
    assert out.shape == g.out.shape and dx.shape == g.din["x"].shape and set(dparam) == set(g.sd)
    errs = all_errors(out, dx, dparam, g.out, g.din["x"], g.dparam)
    bad = {k: v for k, v in errs.items() if not v < REF_TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", SCALER_GOLDEN)
def test_restatement_fp64_envelope(name):
    """float32 restatement vs the float64 one, per quantity: the numerical envelope the HIP path is judged in."""
    g = Golden("scaler_conv/" + name)
    errs = all_errors(*ref_grads(g, torch.float32), *ref_grads(g, torch.float64))
    worst = max(errs, key=errs.get)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"{name}: worst {worst} {errs[worst]:.2e}, above 5e-7: " + str({k: f"{v:.1e}" for k, v in errs.items() if v > 5e-7}))
    assert errs[worst] < 6e-5, (worst, errs[worst])        # a sanity ceiling of 1e3 x eps, not a parity bar


def _fixture_sd(name):
    return Golden("scaler_conv/" + name).sd


def test_default_scalers_construct_with_the_reference_keys():
    """DownScaler(in, out) and UpScaler(in, out) with no further arguments are the 'conv' modes (model.py:645, 697)."""
    import galerkin_transformer as gt
    from galerkin_transformer.layers import Conv2dEncoder, DeConv2dBlock
    down, up = gt.DownScaler(1, 20), gt.UpScaler(16, 16)
    assert [type(m) for m in down.downsample] == [Conv2dEncoder] * 2
    assert [type(m) for m in up.upsample] == [DeConv2dBlock] * 2
    for mod, prefix, fix in ((down, "downsample.", "down_silu_n21"), (up, "upsample.", "up_silu_n5")):
        want = {prefix + k: tuple(v.shape) for k, v in _fixture_sd(fix).items()}
        assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == want
    assert set(down.state_dict()) == {f"downsample.{e}.conv{i}.conv.0.weight" for e in (0, 1) for i in range(4)}
    assert set(up.state_dict()) == {f"upsample.{b}.deconv{i}.{p}" for b in (0, 1) for i in (0, 1) for p in ("weight", "bias")}
    assert tuple(up.upsample[0].deconv0.weight.shape) == (16, 16, 3, 3)
    # paddings: blocks (2, 1) and (4, 2); encoders (1, 1, 1, 1) and (5, 2, 1, 1)
    assert [(b.deconv0.padding[0], b.deconv1.padding[0], b.deconv0.output_padding[0]) for b in up.upsample] == [(2, 1, 0), (4, 2, 0)]
    assert [[getattr(e, f"conv{i}").conv[0].padding[0] for i in range(4)] for e in down.downsample] == [[1, 1, 1, 1], [5, 2, 1, 1]]
    assert [getattr(down.downsample[0], f"conv{i}").conv[0].out_channels for i in range(4)] == [20, 6, 6, 8]
    mod = gt.UpScaler(16, 16)
    mod.load_state_dict({"upsample." + k: v for k, v in _fixture_sd("up_relu_n5").items()})


def test_deconv_mode_is_the_conv_mode():
    import galerkin_transformer as gt
    a, b = gt.UpScaler(16, 16, upsample_mode="conv"), gt.UpScaler(16, 16, upsample_mode="deconv")
    assert str(a) == str(b)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}


def test_unknown_modes_keep_raising():
    import galerkin_transformer as gt
    with pytest.raises(NotImplementedError, match="downsample mode not implemented"):
        gt.DownScaler(1, 20, downsample_mode="nope")
    with pytest.raises(NotImplementedError, match="upsample mode not implemented"):
        gt.UpScaler(16, 16, upsample_mode="nope")


def test_encoder_blocks_ignore_the_activation_type():
    """The reference's quirk (layers.py:309-320): under activation_type='relu' the four blocks stay SiLU with Dropout(0.1);
    only the activation behind the pools follows."""
    from torch import nn

    from galerkin_transformer.layers import Conv2dEncoder
    enc = Conv2dEncoder(4, 20, padding=5, activation_type="relu")
    assert isinstance(enc.activation, nn.ReLU)
    for i in range(4):
        blk = getattr(enc, f"conv{i}")
        assert isinstance(blk.activation, nn.SiLU) and blk.conv[1].p == 0.1 and blk.conv[0].bias is None
        assert not blk.add_res and not blk.basic_block and tuple(blk.conv[0].kernel_size) == (3, 3)
    assert isinstance(enc.pool0, nn.AvgPool2d) and isinstance(enc.pool1, nn.AvgPool2d)
    assert not list(enc.pool0.parameters()) and enc.pool1.kernel_size == 2


def test_deconv_out_size_is_torchs():
    from galerkin_transformer import ops
    seen = refused = 0
    for h in range(1, 13):
        for pad in (0, 1, 2, 4):
            for op in (0, 1):
                w = 13 - h      # another width, to catch swapped axes
                want = [2 * (n - 1) - 2 * pad + 3 + op for n in (h, w)]
                if min(want) < 1:
                    with pytest.raises(ValueError):
                        ops.deconv_out_size(h, w, pad, op)
                    with pytest.raises(RuntimeError):       # torch refuses the call too
                        torch.nn.functional.conv_transpose2d(torch.zeros(1, 1, h, w), torch.zeros(1, 1, 3, 3), stride=2,
                                                             padding=pad, output_padding=op)
                    refused += 1
                    continue
                y = torch.nn.functional.conv_transpose2d(torch.zeros(1, 1, h, w), torch.zeros(1, 1, 3, 3), stride=2,
                                                         padding=pad, output_padding=op)
                assert ops.deconv_out_size(h, w, pad, op) == tuple(y.shape[2:]) == tuple(want)
                seen += 1
    assert seen > 60 and refused > 5
    with pytest.raises(ValueError):
        ops.deconv_out_size(4, 4, 1, 2)         # output_padding must be smaller than the stride
    # the default UpScaler: n_s -> 16 n_s - 45
    for ns, n in ((4, 19), (5, 35), (8, 83)):
        s = ns
        for pad in (2, 1, 4, 2):
            s = ops.deconv_out_size(s, s, pad, 0)[0]
        assert s == n == 16 * ns - 45


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    lib = ctypes.CDLL(_hip.lib_path())
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in _hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    L = _hip.lib()
    assert L.gt_abi_version() == 21 == _hip.ABI_VERSION
    # the shape check touches no device: supported, channels off a multiple of 4, no output, output_padding = 2
    assert L.gt_deconv3x3s2_check(2, 5, 7, 20, 12, 2, 0) == 0
    assert L.gt_deconv3x3s2_check(2, 5, 7, 6, 12, 2, 0) == -4 and L.gt_deconv3x3s2_check(2, 5, 7, 20, 10, 2, 0) == -4
    assert L.gt_deconv3x3s2_check(1, 1, 1, 4, 4, 2, 0) == -1 and L.gt_deconv3x3s2_check(1, 4, 4, 4, 4, 1, 2) == -1
    assert L.gt_deconv3x3s2_check(1, 1, 1, 4, 4, 0, 0) == 0
    assert L.gt_deconv3x3s2_dbias_ws_bytes(2, 5, 7, 12, 2, 0) >= 12 * 4


def test_cpu_tensors_reach_the_operators():
    """A CPU tensor into either scaler is refused by the HIP operators, not by a missing mode."""
    import galerkin_transformer as gt
    from galerkin_transformer import ops
    for mod, x in ((gt.DownScaler(1, 20), torch.randn(2, 21, 21, 1)), (gt.UpScaler(16, 16), torch.randn(2, 5, 5, 16))):
        with pytest.raises(RuntimeError, match="no CPU fallback") as e:
            mod(x)
        assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.avgpool2_act(torch.randn(1, 4, 4, 4), "silu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv_transpose3x3s2(torch.randn(1, 4, 4, 8), torch.randn(8, 8, 3, 3), None, 1, 0, 0.0, "silu", True)


def test_fixtures_hold_arrays_only():
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "scaler_conv")) if f.endswith(".npz"))
    assert files == sorted(n + ".npz" for n in SCALER_GOLDEN)
    for f in files:
        path = os.path.join(GOLDEN, "scaler_conv", f)
        assert os.path.getsize(path) < (1 << 20), f
        z = np.load(path, allow_pickle=False)
        for k in z.files:
            assert k in ("meta", "out", "cot") or k.split("/")[0] in ("sd", "in", "din", "dparam"), (f, k)
            assert z[k].dtype.kind in "fiub", (f, k, z[k].dtype)
        assert json.loads(bytes(z["meta"]).decode())["kind"] == "scaler_conv"
