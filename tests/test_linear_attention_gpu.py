"""'linear' / 'global' attention on the device (-m gpu): the softmax kernels through the C ABI, the modules against the
fixtures recorded from the reference (tests/golden/linear/), one full-size layer against the float64 restatement, and
the behaviour around them (dropout modes, graph capture, nothing leaking into the Galerkin path).

Bars.  Kernels: KTOL = 2e-6 (test_kernels_gpu.py).  Modules: TOL = 1e-5 relative L2 for the output, dx and every parameter
gradient, except where the float32 restatement itself sits further than TOL / 12 from the float64 one: there the bound is
max(TOL, 12 x that deviation), the rule of test_fullsize_models_gpu._gate, computed in the test from the CPU restatement --
never from the device run.  Deviations of the float32 restatement from float64 measured on the CPU
(test_linear_attention_cpu.py::test_restatement_fp64_envelope), largest per fixture:
    enc_linear_c2 1.0e-06, _replay 7.8e-07, enc_linear_c1 1.4e-06, enc_linear_c4 9.3e-07, enc_linear_nopos 1.0e-06,
    enc_global_c5_ln 1.4e-05 (linears.0.bias; linears.0.weight 1.1e-05, linears.1.bias 2.5e-06), _replay 1.8e-06,
    model_burgers_linear_small 9.7e-06 (encoder_layers.1.attn.linears.1.bias; ten tensors between 2e-6 and 1e-5).
Gradients that vanish in exact arithmetic (the bias in front of the token softmax: _linear_ref.zero_grad_params) are
measured absolutely, against the size of the sibling weight's gradient (_linear_ref.grad_errors), at the same bars."""
import ctypes as C
import os
import sys

import pytest
import torch

from _linear_ref import LINEAR_GOLDEN, encoder_layer, grad_errors, ref_grads
from _util import Golden, TOL, rel_l2
from test_modules_gpu import build_module, run_module

pytestmark = pytest.mark.gpu

KTOL = 2e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = [(dk, p) for dk in (16, 32, 48, 64, 96) for p in (0, 1, 2)]          # every DP the Galerkin path takes
NS = (1, 63, 64, 65, 1000, 1849, 8192)
# (B, h, n) the token softmax runs once more at (dk, p) = (96, 2): C4 = 12 * 100 / 4 = 300 column groups, i.e. a single row
# lane (RL = 1) and two column blocks, the second with 44 live lanes of 256.  Every other shape has one column block, RL >= 2.
WIDE = (2, 12, 150)


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


def _tiles(B, n, h, dk, p, dev, seed, big=False):
    """Head tiles [B*n, h, DP] with zero pad columns (as gt_headnorm_fwd leaves them); big: entries near +-80."""
    from galerkin_transformer import _hip
    Dr, DP = dk + p, _hip.round4(dk + p)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * n, h, DP, generator=g)
    if big:
        x = x + 80.0 * torch.sign(torch.randn(B * n, h, DP, generator=g))
    x[..., Dr:] = 0
    return x.to(dev), Dr, DP


@pytest.mark.parametrize("dk,p", HEADS)
def test_feature_softmax_kernels(GT, gpu_device, dk, p):
    from galerkin_transformer import _hip
    B, h = 2, 3
    for n in NS:
        x, Dr, DP = _tiles(B, n, h, dk, p, gpu_device, 1000 * dk + 10 * p + n, big=(n == 65))
        dy = torch.randn_like(x)
        y = _hip.feature_softmax_fwd(x, B * n * h, dk, p)
        dx = _hip.feature_softmax_bwd(y, dy, B * n * h, dk, p)
        x64 = x[..., :Dr].double().requires_grad_(True)
        y64 = torch.softmax(x64, dim=-1)
        (dx64,) = torch.autograd.grad(y64, x64, dy[..., :Dr].double())
        assert torch.isfinite(y).all() and torch.isfinite(dx).all()
        assert (y[..., Dr:] == 0).all() and (dx[..., Dr:] == 0).all()
        assert rel_l2(y[..., :Dr], y64) < KTOL, (n, rel_l2(y[..., :Dr], y64))
        assert rel_l2(dx[..., :Dr], dx64) < KTOL, (n, rel_l2(dx[..., :Dr], dx64))
        assert torch.equal(y, _hip.feature_softmax_fwd(x, B * n * h, dk, p))
        assert torch.equal(dx, _hip.feature_softmax_bwd(y, dy, B * n * h, dk, p))
        xi, gi = x.clone(), dy.clone()                      # in place, as the operator uses them
        assert torch.equal(_hip.feature_softmax_fwd(xi, B * n * h, dk, p, out=xi), y)
        assert torch.equal(_hip.feature_softmax_bwd(y, gi, B * n * h, dk, p, out=gi), dx)


@pytest.mark.parametrize("dk,p", HEADS)
def test_token_softmax_kernels(GT, gpu_device, dk, p):
    from galerkin_transformer import _hip
    for B, h, n in [(2, 3, n) for n in NS] + ([WIDE] if (dk, p) == (96, 2) else []):
        x, Dr, DP = _tiles(B, n, h, dk, p, gpu_device, 2000 * dk + 10 * p + n, big=(n == 65))
        dy = torch.randn_like(x)
        y = _hip.token_softmax_fwd(x, B, n, h, dk, p)
        dx = _hip.token_softmax_bwd(y, dy, B, n, h, dk, p)
        x64 = x.reshape(B, n, h, DP)[..., :Dr].double().requires_grad_(True)
        y64 = torch.softmax(x64, dim=1)
        (dx64,) = torch.autograd.grad(y64, x64, dy.reshape(B, n, h, DP)[..., :Dr].double())
        yv, dxv = y.reshape(B, n, h, DP), dx.reshape(B, n, h, DP)
        assert torch.isfinite(y).all() and torch.isfinite(dx).all()
        assert (yv[..., Dr:] == 0).all() and (dxv[..., Dr:] == 0).all()
        assert rel_l2(yv[..., :Dr], y64) < KTOL, ((B, h, n), rel_l2(yv[..., :Dr], y64))
        assert rel_l2(dxv[..., :Dr], dx64) < KTOL, ((B, h, n), rel_l2(dxv[..., :Dr], dx64))
        assert torch.equal(y, _hip.token_softmax_fwd(x, B, n, h, dk, p))
        assert torch.equal(dx, _hip.token_softmax_bwd(y, dy, B, n, h, dk, p))
        xi, gi = x.clone(), dy.clone()
        assert torch.equal(_hip.token_softmax_fwd(xi, B, n, h, dk, p, out=xi), y)
        assert torch.equal(_hip.token_softmax_bwd(y, gi, B, n, h, dk, p, out=gi), dx)


def test_softmax_kernels_refuse_other_shapes(GT, gpu_device):
    from galerkin_transformer import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    x = torch.zeros(64, 1, 44, device=gpu_device)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=gpu_device)
    for dk, p in ((40, 2), (32, 3), (128, 0)):
        assert lib.gt_feature_softmax_fwd(x.data_ptr(), x.data_ptr(), 64, dk, p, st) == -4
        assert lib.gt_token_softmax_fwd(x.data_ptr(), x.data_ptr(), 1, 64, 1, dk, p, ws.data_ptr(), ws.numel(), st) == -4
    assert lib.gt_token_softmax_fwd(x.data_ptr(), x.data_ptr(), 1, 64, 1, 32, 2, ws.data_ptr(), 16, st) == -3   # GT_EWS


def _no_dropout(mod):
    """The encoder layer forces dropout = 0.1 for 'linear' whatever its argument says (reference model.py:65-66, mirrored):
    switch every nn.Dropout off, as the fixture generator does on the reference."""
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def _run_fixture(GT, dev, g):
    torch.manual_seed(0)
    mod = build_module(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = _no_dropout(mod).to(dev).train()
    if g.masks:
        GT.set_attention_dropout("replay")
        GT.push_attention_masks([m.to(dev) for m in g.masks])
    else:
        GT.set_attention_dropout("off")
    try:
        ins = {k: v.to(dev) for k, v in g.inputs.items()}
        for k in g.din:
            ins[k].requires_grad_(True)
        out = run_module(mod, g, ins)
        out.backward(g.cot.to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    grads = {k: p.grad for k, p in mod.named_parameters()}
    return out.detach(), {k: ins[k].grad for k in g.din}, grads


def _gate(name, errs, noise):
    print(name, "worst", max(errs.values()), {k: (f"{v:.1e}", f"{noise.get(k, 0.0):.1e}") for k, v in errs.items()
                                              if v > 0.5 * TOL})
    bad = {k: (v, max(TOL, 12.0 * noise.get(k, 0.0))) for k, v in errs.items()
           if k != "out" and not v < max(TOL, 12.0 * noise.get(k, 0.0))}
    assert errs["out"] < TOL, errs["out"]
    assert not bad, bad


@pytest.mark.parametrize("name", LINEAR_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("linear/" + name)
    out, din, grads = _run_fixture(GT, gpu_device, g)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(din[k], g.din[k]) for k in g.din})
    for k in g.dparam:
        assert grads[k] is not None, k
    errs.update({"dW:" + k: v for k, v in grad_errors(grads, g.dparam, g.sd).items()})
    # the float32 restatement's own distance from float64, per tensor (CPU): what 1e-5 can and cannot ask of a gradient
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    noise = {"d" + k: rel_l2(di32[k], di64[k]) for k in di32}
    noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, g.sd).items()})
    _gate(name, errs, noise)


def test_full_size_darcy_layer_vs_float64(GT, gpu_device):
    """The ex2_darcy141 encoder shape (1 849 tokens, d 128, 4 heads x (32 + 2), B = 4), attention_type='linear', mask
    replayed, against the float64 restatement; the float32 restatement on the CPU gives the per-tensor noise of the gate."""
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.darcy_config("ex2_darcy141")
    d, h, f = cfg["n_hidden"], cfg["n_head"], cfg["dim_feedforward"]
    B, n, p = 4, 43 * 43, 2
    kw = dict(d_model=d, pos_dim=p, n_head=h, dim_feedforward=f, attention_type="linear", layer_norm=False,
              attn_norm=True, norm_eps=1e-7)
    torch.manual_seed(77)
    layer = GT.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, **kw)
    with torch.no_grad():
        for prm in layer.parameters():
            prm.add_(0.02 * torch.randn_like(prm))
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    x, pos, cot = torch.randn(B, n, d), torch.rand(B, n, p), torch.randn(B, n, d)
    mask = (torch.rand(B, h, d // h + p, d // h + p) >= 0.5).float() * 2.0
    dev = gpu_device
    layer = _no_dropout(layer).to(dev).train()
    GT.set_attention_dropout("replay")
    GT.push_attention_masks([mask.to(dev)])
    try:
        xg = x.to(dev).requires_grad_(True)
        y = layer(xg, pos.to(dev))
        y.backward(cot.to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")

    def ref(dtype):
        s = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        xx = x.to(dtype).requires_grad_(True)
        out = encoder_layer(s, xx, pos.to(dtype), n_head=h, attention_type="linear", layer_norm=False, attn_norm=True,
                            norm_eps=1e-7, attn_drop=mask.to(dtype))
        gs = torch.autograd.grad(out, [xx] + list(s.values()), cot.to(dtype))
        return out.detach(), gs[0], dict(zip(s, gs[1:]))

    o64, dx64, dp64 = ref(torch.float64)
    o32, dx32, dp32 = ref(torch.float32)
    grads = {k: prm.grad for k, prm in layer.named_parameters()}
    errs = {"out": rel_l2(y, o64), "dx": rel_l2(xg.grad, dx64)}
    errs.update({"dW:" + k: v for k, v in grad_errors(grads, dp64, sd).items()})
    noise = {"dx": rel_l2(dx32, dx64)}
    noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, sd).items()})
    _gate("darcy141 linear layer", errs, noise)


def test_global_is_linear(GT, gpu_device):
    g = Golden("linear/enc_linear_c2")
    outs = []
    for at in ("linear", "global"):
        g.meta["attention_type"] = at
        outs.append(_run_fixture(GT, gpu_device, g))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1]["x"], outs[1][1]["x"])
    for k, v in outs[0][2].items():
        assert torch.equal(v, outs[1][2][k]), k


def test_reference_dropout_mode_statistics(GT, gpu_device):
    g = Golden("linear/enc_linear_c2")
    mod = build_module(GT, g)
    mod.load_state_dict(g.sd)
    mod = mod.to(gpu_device).eval()
    mod.attn_weight = True
    x, pos = g.inputs["x"].to(gpu_device), g.inputs["pos"].to(gpu_device)
    GT.set_attention_dropout("off")
    _, w0 = mod(x, pos)
    GT.set_attention_dropout("reference")
    y1, w1 = mod(x, pos)
    y2, w2 = mod(x, pos)
    torch.cuda.synchronize()
    assert w0.shape == (2, 4, 34, 34)
    kept = (w1 != 0)
    assert abs(kept.float().mean().item() - 0.5) < 0.05
    assert torch.allclose(w1[kept], 2 * w0[kept], rtol=1e-5, atol=1e-9)
    assert not torch.equal(w1, w2) and rel_l2(y1, y2) > 1e-6


def test_graph_capture_replays_eager(GT, gpu_device):
    g = Golden("linear/enc_linear_c2")
    dev = gpu_device
    mod = build_module(GT, g)
    mod.load_state_dict(g.sd)
    mod = _no_dropout(mod).to(dev).train()
    x = g.inputs["x"].to(dev).requires_grad_(True)
    pos, cot = g.inputs["pos"].to(dev), g.cot.to(dev)
    params = list(mod.parameters())
    GT.set_attention_dropout("off")
    try:
        def step():
            return torch.autograd.grad(mod(x, pos), [x] + params, cot)
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
    finally:
        GT.set_attention_dropout("reference")
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def test_nothing_leaks_between_kinds(GT, gpu_device):
    gal, lin = Golden("enc_galerkin_c2"), Golden("linear/enc_linear_c2")
    before = _run_fixture(GT, gpu_device, gal)
    _run_fixture(GT, gpu_device, lin)
    after = _run_fixture(GT, gpu_device, gal)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
    for k, v in before[2].items():
        assert torch.equal(v, after[2][k]), k


def test_models_train_with_linear_and_global(GT, gpu_device):
    g = Golden("linear/model_burgers_linear_small")
    dev = gpu_device
    for at in ("linear", "global"):
        m = GT.SimpleTransformer(**dict(g.meta["config"], attention_type=at))
        m.load_state_dict(g.sd, strict=True)
        m = m.to(dev).train()
        out = m(g.inputs["node"].to(dev), None, g.inputs["pos"].to(dev))["preds"]
        out.square().mean().backward()
        torch.cuda.synchronize()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    lite = dict(dropout=0.0, encoder_dropout=0.0, decoder_dropout=0.0, ffn_dropout=0.0, xavier_init=0.01,
                diagonal_weight=0.01, node_feats=12, pos_dim=2, n_targets=1, n_hidden=32, num_encoder_layers=1, n_head=2,
                dim_feedforward=64, layer_norm=True, attn_norm=False, decoder_type="ifft2", freq_dim=12,
                num_regressor_layers=1, fourier_modes=4, spacial_dim=2, spacial_fc=False, regressor_activation="silu",
                debug=False, attention_type="linear")
    m = GT.FourierTransformer2DLite(**lite).to(dev).train()
    ng = 16
    out = m(torch.randn(2, ng, ng, 10, device=dev), None, torch.rand(2, ng * ng, 2, device=dev),
            torch.rand(2, ng, ng, 2, device=dev))["preds"]
    out.square().mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_unsupported_arguments_still_raise(GT, gpu_device):
    layer = GT.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type="linear",
                                             layer_norm=False).to(gpu_device)
    x, pos = torch.randn(1, 8, 64, device=gpu_device), torch.rand(1, 8, 2, device=gpu_device)
    with pytest.raises(RuntimeError, match="casual mask"):
        layer.attn(x, x, x, pos=pos, mask=torch.ones(1, 8, 8, device=gpu_device))
    with pytest.raises(NotImplementedError):
        layer.attn(x, x, x, pos=pos, weight=torch.ones(1, 8, 1, device=gpu_device))
    with pytest.raises(NotImplementedError):
        layer(x, pos, weight=torch.ones(1, 8, 1, device=gpu_device))
