"""The 'conv' scaler modes on the device (-m gpu): the average-pool and transposed-convolution operators against float64, the
stateless dropout of the transposed convolution, the modules against the fixtures recorded from the reference
(tests/golden/scaler_conv/), the whole FourierTransformer2D around them and graph capture.

Bars.  Operators: KTOL = 2e-6 relative L2 against float64 (the kernel suites' bar for fp32-class products), in the default
arithmetic and under set_precision('f32').  Modules and the whole model: TOL = 1e-5 (_util.TOL).  No bar is widened: the
float32 restatement's own deviation from float64 (test_scaler_conv_cpu.py::test_restatement_fp64_envelope) is largest at
1.1e-6 (up_silu_n5, dW:1.deconv1.bias; 5.4e-7 for up_relu_n5; everything else below 5e-7), and four times that is still
inside the module bar."""
import pytest
import torch
import torch.nn.functional as F

from _scaler_conv_ref import SCALER_GOLDEN, all_errors, conv_transpose, model_forward
from _util import Golden, TOL, rel_l2

pytestmark = pytest.mark.gpu

KTOL = 2e-6


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


@pytest.fixture(params=("default", "f32"))
def precision(request, GT):
    from galerkin_transformer import _hip
    if request.param == "default":
        yield _hip.get_precision()
        return
    old = _hip.set_precision("f32")
    yield "f32"
    _hip.set_precision(old)


# ------------------------------------------------------------------------------------------ average pool + activation
_ACT64 = {"none": lambda t: t, "relu": F.relu, "silu": F.silu}


# (2, 20, 13, 9) and (1, 4, 2, 2): both pools drop a line / the smallest map.  (2, 3, 7, 8): W % 4 == 0 takes the two-cell
# channels-first kernel, C = 3 the scalar channels-last one.
@pytest.mark.parametrize("shape", ((2, 20, 13, 9), (1, 4, 2, 2), (2, 3, 7, 8)))
@pytest.mark.parametrize("act", ("none", "relu", "silu"))
def test_avgpool_act_vs_float64(GT, gpu_device, shape, act):
    from galerkin_transformer import ops
    B, C, Hh, Ww = shape
    gen = torch.Generator().manual_seed(sum(shape) + len(act))
    x = torch.randn(shape, generator=gen)
    cot = torch.randn(B, C, Hh // 2, Ww // 2, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = _ACT64[act](F.avg_pool2d(x64, 2))
    (dx64,) = torch.autograd.grad(y64, x64, cot.double())
    if Hh % 2:
        assert not dx64[:, :, -1].any()
    for in_nhwc in (False, True):
        for out_nhwc in (False, True):
            xd = (x.permute(0, 2, 3, 1) if in_nhwc else x).contiguous().to(gpu_device).requires_grad_(True)
            cd = (cot.permute(0, 2, 3, 1) if out_nhwc else cot).contiguous().to(gpu_device)
            y = ops.avgpool2_act(xd, act, in_nhwc=in_nhwc, out_nhwc=out_nhwc)
            (dx,) = torch.autograd.grad(y, xd, cd)
            torch.cuda.synchronize()
            y, dx = y.detach().cpu(), dx.cpu()
            y = y.permute(0, 3, 1, 2) if out_nhwc else y
            dx = dx.permute(0, 3, 1, 2) if in_nhwc else dx
            assert y.shape == y64.shape and dx.shape == x.shape
            errs = {"y": rel_l2(y, y64), "dx": rel_l2(dx, dx64)}
            print(shape, act, in_nhwc, out_nhwc, {k: f"{v:.1e}" for k, v in errs.items()})
            assert max(errs.values()) < KTOL, (in_nhwc, out_nhwc, errs)
            if Hh % 2:
                assert torch.equal(dx[:, :, -1], torch.zeros(B, C, Ww)), "dropped row"
            if Ww % 2:
                assert torch.equal(dx[:, :, :, -1], torch.zeros(B, C, Hh)), "dropped column"


def test_avgpool_refuses_an_empty_map(GT, gpu_device):
    from galerkin_transformer import _hip, ops
    with _hip.Profile() as prof:
        with pytest.raises(ValueError):
            ops.avgpool2_act(torch.zeros(1, 4, 1, 6, device=gpu_device), "silu")
        with pytest.raises(NotImplementedError):
            ops.avgpool2_act(torch.zeros(1, 4, 4, 6, device=gpu_device), "gelu")
    assert not prof.records


# ------------------------------------------------------------------------------------------ transposed convolution
def _deconv_case(shape, pad, op, seed, bias=True):
    B, Hh, Ww, Cin, Cout = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hh, Ww, Cin, generator=gen)
    w = torch.randn(Cin, Cout, 3, 3, generator=gen) / (Cin * 2.25) ** 0.5
    b = 0.3 * torch.randn(Cout, generator=gen) if bias else None
    ho, wo = (2 * (n - 1) - 2 * pad + 3 + op for n in (Hh, Ww))
    cot = torch.randn(B, ho, wo, Cout, generator=gen)
    return x, w, b, cot


def _deconv_f64(x, w, b, cot, pad, op, act, mask=None):
    """float64 on the CPU, channels-last in and out: (y, dx, dW, db); ``mask`` (B, Ho, Wo, C) includes the 1 / (1 - p)."""
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    m = None if mask is None else mask.double().permute(0, 3, 1, 2)
    y = conv_transpose(x64.permute(0, 3, 1, 2), w64, b64, pad, op, act, m).permute(0, 2, 3, 1)
    g = torch.autograd.grad(y, [x64, w64] + ([] if b is None else [b64]), cot.double())
    return y.detach(), g[0], g[1], (None if b is None else g[2])


def _deconv_dev(dev, x, w, b, cot, pad, op, act, p_drop=0.0, training=True):
    from galerkin_transformer import ops
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bd = None if b is None else b.to(dev).requires_grad_(True)
    y = ops.conv_transpose3x3s2(xd, wd, bd, pad, op, p_drop, act, training)
    g = torch.autograd.grad(y, [xd, wd] + ([] if b is None else [bd]), cot.to(dev))
    torch.cuda.synchronize()
    return y.detach().cpu(), g[0].cpu(), g[1].cpu(), (None if b is None else g[2].cpu())


def _deconv_errs(got, ref):
    return {k: rel_l2(a, r) for k, a, r in zip(("y", "dx", "dW", "db"), got, ref) if r is not None}


@pytest.mark.parametrize("op", (0, 1))
@pytest.mark.parametrize("pad", (1, 2, 4))
def test_conv_transpose_vs_float64(GT, gpu_device, precision, pad, op):
    """(B, H, W, Cin, Cout) = (2, 5, 7, 20, 12): not square, so swapped axes show."""
    from galerkin_transformer import ops
    shape = (2, 5, 7, 20, 12)
    for act in ("silu", "relu", None):
        x, w, b, cot = _deconv_case(shape, pad, op, 100 * pad + 10 * op + len(str(act)))
        ref = _deconv_f64(x, w, b, cot, pad, op, act)
        got = _deconv_dev(gpu_device, x, w, b, cot, pad, op, act)
        assert tuple(got[0].shape[1:3]) == ops.deconv_out_size(5, 7, pad, op) == tuple(ref[0].shape[1:3])
        errs = _deconv_errs(got, ref)
        print(precision, pad, op, act, {k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < KTOL, (act, errs)
        again = _deconv_dev(gpu_device, x, w, b, cot, pad, op, act)
        assert all(torch.equal(a, c) for a, c in zip(got, again)), "second call differs"


def test_conv_transpose_production_widths(GT, gpu_device, precision):
    """(1, 12, 12, 128, 128), padding 2: more than one tile of every product, the up-scaler's widths."""
    x, w, b, cot = _deconv_case((1, 12, 12, 128, 128), 2, 0, 7)
    errs = _deconv_errs(_deconv_dev(gpu_device, x, w, b, cot, 2, 0, "silu"), _deconv_f64(x, w, b, cot, 2, 0, "silu"))
    print(precision, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < KTOL, errs


def test_conv_transpose_smallest_image(GT, gpu_device, precision):
    """H = W = 1, padding 0: one pixel becomes 3 x 3 (4 x 4 with output_padding 1, whose last line holds the bias alone)."""
    for op in (0, 1):
        x, w, b, cot = _deconv_case((1, 1, 1, 4, 8), 0, op, 11 + op)
        got, ref = _deconv_dev(gpu_device, x, w, b, cot, 0, op, "silu"), _deconv_f64(x, w, b, cot, 0, op, "silu")
        assert got[0].shape == (1, 3 + op, 3 + op, 8)
        errs = _deconv_errs(got, ref)
        assert max(errs.values()) < KTOL, (op, errs)
    x, w, _, cot = _deconv_case((2, 3, 2, 8, 4), 1, 0, 13, bias=False)          # no bias
    errs = _deconv_errs(_deconv_dev(gpu_device, x, w, None, cot, 1, 0, "relu"), _deconv_f64(x, w, None, cot, 1, 0, "relu"))
    assert max(errs.values()) < KTOL, errs


def test_conv_transpose_refusals_launch_nothing(GT, gpu_device):
    from galerkin_transformer import _hip, ops
    dev = gpu_device
    with _hip.Profile() as prof:
        with pytest.raises(NotImplementedError):                 # C_in = 6
            ops.conv_transpose3x3s2(torch.zeros(2, 5, 7, 6, device=dev), torch.zeros(6, 12, 3, 3, device=dev), None, 2, 0)
        with pytest.raises(NotImplementedError):                 # C_out = 10
            ops.conv_transpose3x3s2(torch.zeros(2, 5, 7, 8, device=dev), torch.zeros(8, 10, 3, 3, device=dev), None, 2, 0)
        with pytest.raises(ValueError):                          # no output left
            ops.conv_transpose3x3s2(torch.zeros(1, 1, 1, 8, device=dev), torch.zeros(8, 8, 3, 3, device=dev), None, 2, 0)
        with pytest.raises(ValueError):                          # output_padding = stride
            ops.conv_transpose3x3s2(torch.zeros(1, 4, 4, 8, device=dev), torch.zeros(8, 8, 3, 3, device=dev), None, 1, 2)
        with pytest.raises(ValueError):                          # the weight of another convolution
            ops.conv_transpose3x3s2(torch.zeros(1, 4, 4, 8, device=dev), torch.zeros(4, 8, 3, 3, device=dev), None, 1, 0)
    assert not prof.records
    with _hip.Profile() as prof:                                 # (and a supported call does record its launches)
        ops.conv_transpose3x3s2(torch.zeros(1, 4, 4, 8, device=dev), torch.zeros(8, 8, 3, 3, device=dev), None, 1, 0)
    torch.cuda.synchronize()
    assert any("gt_deconv3x3s2_gather_fwd" in r[0] for r in prof.records)


# ------------------------------------------------------------------------------------------ dropout
def _dropped_run(dev, case, pad, op, p, seed):
    """One training call with p_drop = p under SiLU; the mask (with its scale) is read off the output: silu(0) = 0."""
    from galerkin_transformer import _hip
    x, w, b, cot = case
    _hip.set_seed(seed, dev)
    got = _deconv_dev(dev, x, w, b, cot, pad, op, "silu", p_drop=p, training=True)
    mask = (got[0] != 0).float() / (1.0 - p)
    return got, mask


def test_conv_transpose_dropout_mask_is_recomputed(GT, gpu_device, precision):
    p = 0.3
    case = _deconv_case((2, 5, 7, 20, 12), 2, 0, 21)
    got, mask = _dropped_run(gpu_device, case, 2, 0, p, 1234)
    ref = _deconv_f64(*case, 2, 0, "silu", mask)
    # (an exact zero at a kept position would be read as dropped and show as an error below; none is expected -- if one
    # turns up the remedy is another seed, not a wider bar)
    errs = _deconv_errs(got, ref)
    print(precision, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < KTOL, errs
    frac = float((mask == 0).float().mean())
    assert 0.15 < frac < 0.45, frac           # (1 848 values: a sanity band; the share itself is checked on the large case)


def test_conv_transpose_dropout_share_and_fresh_masks(GT, gpu_device):
    from galerkin_transformer import _hip, ops
    p, dev = 0.3, gpu_device
    case = _deconv_case((1, 12, 12, 128, 128), 2, 0, 22)
    got, mask = _dropped_run(dev, case, 2, 0, p, 99)
    assert mask.numel() >= 10 ** 4
    frac = float((mask == 0).float().mean())
    print("dropped share", frac, "of", mask.numel())
    assert abs(frac - p) < 0.02, frac         # > 10 standard deviations of the binomial at the 56 448 values here
    errs = _deconv_errs(got, _deconv_f64(*case, 2, 0, "silu", mask))
    assert max(errs.values()) < KTOL, errs
    # two calls of one step draw different masks; eval mode draws none
    x, w, b, _ = (t.to(dev) for t in case)
    _hip.set_seed(5, dev)
    y1 = ops.conv_transpose3x3s2(x, w, b, 2, 0, p, "silu", True)
    y2 = ops.conv_transpose3x3s2(x, w, b, 2, 0, p, "silu", True)
    y3 = ops.conv_transpose3x3s2(x, w, b, 2, 0, p, "silu", False)
    torch.cuda.synchronize()
    differ = float(((y1 == 0) != (y2 == 0)).float().mean())
    assert 0.3 < differ < 0.55, differ        # 2 p (1 - p) = 0.42 for independent masks
    assert int((y3 == 0).sum()) == 0


# ------------------------------------------------------------------------------------------ modules against the fixtures
def _fixture_module(GT, g, dev):
    from galerkin_transformer.layers import DeConv2dBlock
    m = g.meta
    torch.manual_seed(0)
    if m["module"] == "DownScaler":
        mod, prefix = GT.DownScaler(m["in_dim"], m["out_dim"], activation_type=m["activation_type"]), "downsample."
    elif m["module"] == "UpScaler":
        mod, prefix = GT.UpScaler(m["in_dim"], m["out_dim"], activation_type=m["activation_type"]), "upsample."
    else:
        mod, prefix = DeConv2dBlock(m["in_dim"], m["hidden_dim"], m["out_dim"], padding=m["padding"],
                                    output_padding=m["output_padding"], activation_type=m["activation_type"]), ""
    res = mod.load_state_dict({prefix + k: v for k, v in g.sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return mod.to(dev).eval(), prefix


@pytest.mark.parametrize("name", SCALER_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("scaler_conv/" + name)
    mod, prefix = _fixture_module(GT, g, gpu_device)
    x = g.inputs["x"].to(gpu_device).requires_grad_(True)
    out = mod(x)
    out.backward(g.cot.to(gpu_device))
    torch.cuda.synchronize()
    assert out.shape == g.out.shape and x.grad.shape == g.din["x"].shape
    grads = {k[len(prefix):]: p.grad for k, p in mod.named_parameters()}
    assert set(grads) == set(g.dparam) and all(v is not None for v in grads.values())
    errs = all_errors(out, x.grad, grads, g.out, g.din["x"], g.dparam)
    print(name, "worst", max(errs, key=errs.get), {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


# ------------------------------------------------------------------------------------------ whole model
def _model_cfg():
    # n = 35 and n_s = 5 go together: 35 -> 5 through the two encoders, 16 * 5 - 45 = 35 back
    return dict(node_feats=1, pos_dim=2, n_targets=1, n_hidden=32, num_feat_layers=0, num_encoder_layers=1, n_head=2,
                dim_feedforward=64, attention_type="galerkin", layer_norm=False, attn_norm=True, norm_eps=1e-7,
                xavier_init=0.01, diagonal_weight=0.01, symmetric_init=False, batch_norm=False, return_attn_weight=False,
                return_latent=False, decoder_type="ifft2", freq_dim=16, num_regressor_layers=2, fourier_modes=4,
                spacial_dim=2, spacial_fc=True, regressor_activation="silu", last_activation=True,
                downsample_mode="conv", upsample_mode="conv", downscaler_size=(5, 5), upscaler_size=(35, 35),
                downscaler_activation="relu", upscaler_activation="silu", downscaler_dropout=0.05, upscaler_dropout=0.1,
                dropout=0.0, encoder_dropout=0.05, ffn_dropout=0.05, decoder_dropout=0.0, boundary_condition="dirichlet",
                debug=False)


def _model_batch(dev):
    gen = torch.Generator().manual_seed(3)
    B, n, ns = 2, 35, 5
    node = torch.randn(B, n, n, 1, generator=gen)
    lin = lambda k: torch.linspace(0, 1, k)
    pos = torch.stack(torch.meshgrid(lin(ns), lin(ns), indexing="ij"), -1).reshape(1, ns * ns, 2).repeat(B, 1, 1)
    grid = torch.stack(torch.meshgrid(lin(n), lin(n), indexing="ij"), -1)[None].repeat(B, 1, 1, 1)
    target = torch.randn(B, n, n, 1, generator=gen)
    return tuple(t.to(dev) for t in (node, pos, grid, target))


def test_whole_model_with_conv_scalers(GT, gpu_device):
    from galerkin_transformer.layers import Conv2dEncoder, DeConv2dBlock
    dev, cfg = gpu_device, _model_cfg()
    torch.manual_seed(4)
    model = GT.FourierTransformer2D(**cfg).to(dev)
    assert isinstance(model.downscaler.downsample[1], Conv2dEncoder) and isinstance(model.upscaler.upsample[1], DeConv2dBlock)
    node, pos, grid, target = _model_batch(dev)
    # one training step: forward, loss, backward
    model.train()
    preds = model(node, None, pos, grid)["preds"]
    assert preds.shape == target.shape
    loss = ((preds - target) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for k, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), k
    assert all(float(prm.grad.abs().max()) > 0 for k, prm in model.named_parameters() if "scaler" in k)
    # eval forward against float64
    model.eval()
    with torch.no_grad():
        out = model(node, None, pos, grid)["preds"]
    torch.cuda.synchronize()
    sd64 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    ref = model_forward(sd64, cfg, node.double().cpu(), pos.double().cpu(), grid.double().cpu())
    err = rel_l2(out, ref)
    print("whole model, eval forward vs float64:", f"{err:.2e}")
    assert out.shape == ref.shape and err < TOL, err


# ------------------------------------------------------------------------------------------ graph capture
def test_graph_capture_replays_eager(GT, gpu_device):
    g = Golden("scaler_conv/up_silu_n5")
    dev = gpu_device
    mod, _ = _fixture_module(GT, g, dev)
    x = g.inputs["x"].to(dev).requires_grad_(True)
    cot = g.cot.to(dev)
    params = list(mod.parameters())

    def step():
        return torch.autograd.grad(mod(x), [x] + params, cot)
    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
