"""Plain-torch restatement of the 'conv' scaler modes (reference layers.py:284-341, 515-559; model.py:640-749), in any dtype
and on any device, from a state_dict: Conv2dEncoder, DeConv2dBlock, DownScaler('conv'), UpScaler('conv') and the whole
FourierTransformer2D around them (the oracle's encoder layers and regressor).  Pinned against the fixtures of
tests/golden/scaler_conv/ by test_scaler_conv_cpu.py; the GPU tests take their float64 references from here."""
import torch
import torch.nn.functional as F

from _util import rel_l2
from oracle import galerkin_oracle as O

SCALER_GOLDEN = ("down_relu_n21", "down_relu_n16", "down_silu_n21", "down_silu_n16", "up_silu_n5", "up_relu_n5",
                 "deconv_block_op1")
_ACT = {"relu": F.relu, "silu": F.silu, "none": lambda t: t, None: lambda t: t}


def conv2d_encoder(sd, prefix, x, padding, act):
    """x (B, C, H, W).  The four blocks are conv (no bias) -> dropout -> SiLU whatever ``act`` is: the encoder hands its
    activation_type to nobody (layers.py:309-320); eval mode, so their Dropout(0.1) is the identity."""
    pads = (padding, max(padding // 2, 1), max(padding // 4, 1), 1)
    blk = lambda i, t: F.silu(F.conv2d(t, sd[f"{prefix}conv{i}.conv.0.weight"], padding=pads[i]))
    x = _ACT[act](F.avg_pool2d(blk(0, x), 2))
    x1 = blk(1, x)
    x2 = blk(2, x1)
    x3 = blk(3, x2)
    return _ACT[act](F.avg_pool2d(torch.cat([x1, x2, x3], dim=1), 2))


def down_scaler(sd, x, act, padding=5, prefix="downsample."):
    """x (B, n, n, Cin) -> (B, n_s, n_s, Cout): two encoders, the first with padding 1, the second with ``padding``."""
    x = x.permute(0, 3, 1, 2)
    x = conv2d_encoder(sd, prefix + "0.", x, 1, act)
    return conv2d_encoder(sd, prefix + "1.", x, padding, act).permute(0, 2, 3, 1)


def conv_transpose(x, w, b, padding, output_padding, act=None, mask=None):
    """act(mask * conv_transpose2d(x)) on (B, C, H, W); ``mask``: the dropout mask INCLUDING its 1 / (1 - p) scale."""
    y = F.conv_transpose2d(x, w, b, stride=2, padding=padding, output_padding=output_padding)
    return _ACT[act](y if mask is None else y * mask)


def deconv_block(sd, prefix, x, padding, output_padding, act, mask=None):
    """x (B, C, H, W): deconv0 -> dropout (``mask``) -> act -> deconv1 -> act."""
    x = conv_transpose(x, sd[prefix + "deconv0.weight"], sd[prefix + "deconv0.bias"], padding, output_padding, act, mask)
    return conv_transpose(x, sd[prefix + "deconv1.weight"], sd[prefix + "deconv1.bias"], max(padding // 2, 1), output_padding,
                          act)


def up_scaler(sd, x, act, padding=2, output_padding=0, prefix="upsample."):
    """x (B, n_s, n_s, C) -> (B, n, n, C): two blocks with paddings ``padding`` and 2 ``padding``."""
    x = x.permute(0, 3, 1, 2)
    x = deconv_block(sd, prefix + "0.", x, padding, output_padding, act)
    return deconv_block(sd, prefix + "1.", x, 2 * padding, output_padding, act).permute(0, 2, 3, 1)


def run_fixture(meta, sd, x):
    """The module a fixture of tests/golden/scaler_conv/ was recorded from, on its input."""
    if meta["module"] == "DownScaler":
        return down_scaler({"downsample." + k: v for k, v in sd.items()}, x, meta["activation_type"])
    if meta["module"] == "UpScaler":
        return up_scaler({"upsample." + k: v for k, v in sd.items()}, x, meta["activation_type"])
    assert meta["module"] == "DeConv2dBlock"
    return deconv_block(sd, "", x, meta["padding"], meta["output_padding"], meta["activation_type"])


def ref_grads(g, dtype, device="cpu"):
    """(out, dx, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(device, dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    x = g.inputs["x"].to(device, dtype).clone().requires_grad_(True)
    out = run_fixture(g.meta, sd, x)
    names = list(g.dparam)
    grads = torch.autograd.grad(out, [x] + [sd[k] for k in names], g.cot.to(device, dtype))
    return out.detach(), grads[0], dict(zip(names, grads[1:]))


def all_errors(out, dx, dparam, ref_out, ref_dx, ref_dparam):
    errs = {"out": rel_l2(out, ref_out), "dx": rel_l2(dx, ref_dx)}
    errs.update({"dW:" + k: rel_l2(dparam[k], v) for k, v in ref_dparam.items()})
    return errs


def model_forward(sd, cfg, node, pos, grid):
    """FourierTransformer2D.forward (model.py:953-1017) in eval mode with both scalers in their 'conv' mode."""
    B, nh = node.shape[0], cfg["n_hidden"]
    x = down_scaler(O._sub(sd, "downscaler."), node, cfg.get("downscaler_activation") or "silu")
    ns = x.shape[1]
    x = x.reshape(B, -1, nh)
    for li in range(cfg["num_encoder_layers"]):
        x = O.encoder_layer(O._sub(sd, f"encoder_layers.{li}."), x, pos, **O._enc_kwargs(cfg))
    x = up_scaler(O._sub(sd, "upscaler."), x.reshape(B, ns, ns, nh),
                  "silu" if cfg.get("upscaler_activation") == "silu" else "relu")       # (layers.py:548: anything else is ReLU)
    x = O.spectral_regressor(O._sub(sd, "regressor."), x, grid, modes=cfg["fourier_modes"],
                             num_spectral_layers=cfg["num_regressor_layers"], spacial_dim=cfg["spacial_dim"],
                             spacial_fc=cfg["spacial_fc"], activation=cfg.get("regressor_activation"),
                             last_activation=bool(cfg.get("last_activation")))
    if cfg.get("boundary_condition") == "dirichlet":
        x = F.pad(x[:, 1:-1, 1:-1], (0, 0, 1, 1, 1, 1))
    return x
