"""norm_type='instance' on the device (-m gpu): the token-norm kernels through the C ABI, the modules against the fixtures
recorded from the reference (tests/golden/instance/), one full-size layer against the float64 restatement, and the behaviour
around them (eval = train, graph capture, nothing leaking into the LayerNorm paths, refusals).

Bars.  Kernels: KTOL = 2e-6 (test_linear_attention_gpu.py holds the softmax kernels to it).  Offset column (|mean| / std =
1e3): 4 x the float32 evaluation of torch.nn.functional.instance_norm on the same data against float64, measured in the
test.  Modules: TOL = 1e-5 relative L2 for the output, dx and every parameter gradient, except where the float32 restatement
itself sits further than TOL / 12 from the float64 one: there max(TOL, 12 x that deviation), computed in the test from the
CPU restatement -- never from the device run.  Deviations of the float32 restatement from float64 measured on the CPU
(test_instance_norm_cpu.py::test_restatement_fp64_envelope), largest per fixture:
    enc_galerkin_inst_c2 5.8e-07, _replay 5.9e-07, enc_galerkin_inst_c1 7.2e-07, enc_galerkin_inst_c4 5.0e-07,
    enc_galerkin_inst_nopos 1.6e-06, enc_linear_inst_c2 2.9e-06 (linears.2.bias), enc_global_inst_c5 2.4e-06
    (linears.2.bias), model_burgers_galerkin_inst_small 2.8e-06: the 1e-5 bar binds everywhere.
Gradients that vanish in exact arithmetic (the K and V projection biases behind the token mean; norm_K.*.bias too behind
the token softmax: _instance_ref.zero_grad_params) are measured absolutely, against the size of the sibling weight's
gradient (_instance_ref.grad_errors), at the same bars."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from _instance_ref import INSTANCE_GOLDEN, attention_type_of, encoder_layer, grad_errors, ref_grads
from _util import Golden, TOL, rel_l2
from test_modules_gpu import build_module, run_module

pytestmark = pytest.mark.gpu

KTOL = 2e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ((16, 1), (32, 2), (48, 2), (64, 0), (96, 2))
# 33, 150, 1849: no multiple of any chunk length.  (Not n = 2: there xh = +-1 whatever the data, so dX vanishes in exact
# arithmetic up to eps and a relative error of it measures nothing; the operator test below runs n = 8.)
NS = (33, 150, 1849)
# (B, h, n) run once more at (dk, p) = (96, 2): C4 = 12 * 100 / 4 = 300 column groups, i.e. a single row lane (RL = 1) and two
# column blocks, the second with 44 live lanes of 256.  Every other shape here has one column block and RL >= 2.
WIDE = (2, 12, 150)


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


def _tiles(B, n, h, dk, p, dev, seed, offset=0.0):
    """Head tiles [B*n, h, DP]: coordinates in [0, p), values (+ offset) behind them, zero pad columns."""
    from galerkin_transformer import _hip
    Dr, DP = dk + p, _hip.round4(dk + p)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * n, h, DP, generator=g)
    x[..., p:Dr] += offset
    x[..., :p] = torch.rand(B * n, h, p, generator=g)
    x[..., Dr:] = 0
    return x.to(dev), Dr, DP


def _ref64(x, dy, gamma, beta, eps, B, n, h, dk, p):
    """float64 torch on the value columns: (y, dx, dgamma, dbeta, mean, rstd), tensors [B, n, h, dk] / [h, dk] / [B, h, dk]."""
    DP = x.shape[-1]
    xv = x.reshape(B, n, h, DP)[..., p:p + dk].double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu = xv.mean(dim=1, keepdim=True)
    var = ((xv - mu) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xv - mu) * rstd * g64 + b64
    dx, dg, db = torch.autograd.grad(y, [xv, g64, b64], dy.reshape(B, n, h, DP)[..., p:p + dk].double())
    return y.detach(), dx, dg, db, mu.detach()[:, 0], rstd.detach()[:, 0]


@pytest.mark.parametrize("dk,p", HEADS)
def test_token_norm_kernels(GT, gpu_device, dk, p):
    from galerkin_transformer import _hip
    eps = 1e-5
    for B, h, n in [(3, 3, n) for n in NS] + ([WIDE] if (dk, p) == (96, 2) else []):
        x, Dr, DP = _tiles(B, n, h, dk, p, gpu_device, 3000 * dk + 10 * p + n)
        dy = torch.randn_like(x)
        gamma = 1.0 + 0.5 * torch.randn(h, dk, device=gpu_device)
        beta = torch.randn(h, dk, device=gpu_device)
        y, stats = _hip.token_norm_fwd(x, gamma, beta, eps, B, n, h, dk, p)
        dx, dg, db = _hip.token_norm_bwd(x, dy, gamma, stats, B, n, h, dk, p)
        y64, dx64, dg64, db64, mu64, rstd64 = _ref64(x, dy, gamma, beta, eps, B, n, h, dk, p)
        yv, dxv = y.reshape(B, n, h, DP), dx.reshape(B, n, h, DP)
        xv, dyv = x.reshape(B, n, h, DP), dy.reshape(B, n, h, DP)
        assert torch.isfinite(y).all() and torch.isfinite(dx).all()
        errs = dict(y=rel_l2(yv[..., p:Dr], y64), dx=rel_l2(dxv[..., p:Dr], dx64), dgamma=rel_l2(dg, dg64),
                    dbeta=rel_l2(db, db64), rstd=rel_l2(stats[..., 1], rstd64),
                    # the mean in units of the column's standard deviation, which is how it enters y (the mean of n unit
                    # normals is ~ n^-1/2: an error relative to itself would measure the data's cancellation)
                    mean=float(((stats[..., 0].double() - mu64) * rstd64).norm() / rstd64.numel() ** 0.5))
        print(dk, p, (B, h, n), {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < KTOL for v in errs.values()), ((B, h, n), errs)
        # coordinates pass through untouched, pad columns are exact zeros
        assert torch.equal(yv[..., :p], xv[..., :p]) and torch.equal(dxv[..., :p], dyv[..., :p])
        assert (yv[..., Dr:] == 0).all() and (dxv[..., Dr:] == 0).all()
        # two runs: the same bits; in place: the same bits
        y2, stats2 = _hip.token_norm_fwd(x, gamma, beta, eps, B, n, h, dk, p)
        dx2, dg2, db2 = _hip.token_norm_bwd(x, dy, gamma, stats, B, n, h, dk, p)
        assert torch.equal(y, y2) and torch.equal(stats, stats2)
        assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
        xi, gi = x.clone(), dy.clone()
        yi, si = _hip.token_norm_fwd(xi, gamma, beta, eps, B, n, h, dk, p, out=xi)
        assert yi is xi and torch.equal(yi, y) and torch.equal(si, stats)
        dxi, dgi, dbi = _hip.token_norm_bwd(x, gi, gamma, stats, B, n, h, dk, p, out=gi)
        assert dxi is gi and torch.equal(dxi, dx) and torch.equal(dgi, dg) and torch.equal(dbi, db)


def test_token_norm_refuses_other_shapes(GT, gpu_device):
    from galerkin_transformer import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    x = torch.zeros(64, 1, 44, device=gpu_device)
    gb = torch.ones(1, 128, device=gpu_device)
    stats = torch.zeros(1, 1, 128, 2, device=gpu_device)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=gpu_device)
    for dk, p in ((40, 2), (32, 3), (128, 0)):
        assert lib.gt_token_norm_ws_bytes(1, 64, 1, dk, p) == 0
        assert lib.gt_token_norm_fwd(x.data_ptr(), gb.data_ptr(), gb.data_ptr(), 1e-5, x.data_ptr(), stats.data_ptr(), 1, 64,
                                     1, dk, p, ws.data_ptr(), ws.numel(), st) == -4          # GT_ENOTSUP
        assert lib.gt_token_norm_bwd(x.data_ptr(), x.data_ptr(), gb.data_ptr(), stats.data_ptr(), x.data_ptr(), gb.data_ptr(),
                                     gb.data_ptr(), 1, 64, 1, dk, p, ws.data_ptr(), ws.numel(), st) == -4
    need = lib.gt_token_norm_ws_bytes(1, 64, 1, 32, 2)
    assert need > 16
    assert lib.gt_token_norm_fwd(x.data_ptr(), gb.data_ptr(), gb.data_ptr(), 1e-5, x.data_ptr(), stats.data_ptr(), 1, 64, 1,
                                 32, 2, ws.data_ptr(), need - 16, st) == -3                  # GT_EWS
    assert lib.gt_token_norm_bwd(x.data_ptr(), x.data_ptr(), gb.data_ptr(), stats.data_ptr(), x.data_ptr(), gb.data_ptr(),
                                 gb.data_ptr(), 1, 64, 1, 32, 2, ws.data_ptr(), need - 16, st) == -3
    torch.cuda.synchronize()


def test_offset_column_keeps_its_digits(GT, gpu_device):
    """Every value column is 1e3 + N(0, 1): |mean| / std = 1e3.  Forward and dX against float64; the allowance is what
    float32 torch.nn.functional.instance_norm loses on the same data (CPU, against float64), times 4.  A variance formed as
    E[x^2] - mean^2 is off by ~5e-2 here."""
    from galerkin_transformer import _hip
    B, n, h, dk, p, eps = 2, 1849, 3, 32, 2, 1e-5
    x, Dr, DP = _tiles(B, n, h, dk, p, gpu_device, 4242, offset=1e3)
    dy = torch.randn_like(x)
    gamma = 1.0 + 0.5 * torch.randn(h, dk, device=gpu_device)
    beta = torch.randn(h, dk, device=gpu_device)
    y, stats = _hip.token_norm_fwd(x, gamma, beta, eps, B, n, h, dk, p)
    dx, dg, db = _hip.token_norm_bwd(x, dy, gamma, stats, B, n, h, dk, p)
    y64, dx64, dg64, db64, _, _ = _ref64(x, dy, gamma, beta, eps, B, n, h, dk, p)
    # the yardstick: torch's own float32 operator, [B, h * dk, n] with the per-head affine flattened to channels
    xc = x.reshape(B, n, h, DP)[..., p:Dr].permute(0, 2, 3, 1).reshape(B, h * dk, n).cpu().requires_grad_(True)
    gc = dy.reshape(B, n, h, DP)[..., p:Dr].permute(0, 2, 3, 1).reshape(B, h * dk, n).cpu()
    yt = F.instance_norm(xc, weight=gamma.reshape(-1).cpu(), bias=beta.reshape(-1).cpu(), eps=eps)
    (dxt,) = torch.autograd.grad(yt, xc, gc)
    back = lambda t: t.detach().reshape(B, h, dk, n).permute(0, 3, 1, 2)
    allow_y, allow_dx = 4 * rel_l2(back(yt), y64.cpu()), 4 * rel_l2(back(dxt), dx64.cpu())
    err_y = rel_l2(y.reshape(B, n, h, DP)[..., p:Dr], y64)
    err_dx = rel_l2(dx.reshape(B, n, h, DP)[..., p:Dr], dx64)
    print(f"offset column: y {err_y:.2e} (allowance {allow_y:.2e}), dx {err_dx:.2e} (allowance {allow_dx:.2e}), "
          f"dgamma {rel_l2(dg, dg64):.2e}, dbeta {rel_l2(db, db64):.2e}")
    assert err_y < allow_y, (err_y, allow_y)
    assert err_dx < allow_dx, (err_dx, allow_dx)


def test_zero_weights(GT, gpu_device):
    """gamma with zeros: dX is exactly zero there and dgamma is still right (xh comes from the raw input, not from Y / gamma)."""
    from galerkin_transformer import _hip
    B, n, h, dk, p, eps = 2, 150, 4, 32, 2, 1e-5
    x, Dr, DP = _tiles(B, n, h, dk, p, gpu_device, 99)
    dy = torch.randn_like(x)
    gamma = 1.0 + 0.5 * torch.randn(h, dk, device=gpu_device)
    gamma[:, ::3] = 0
    gamma[1] = 0
    beta = torch.randn(h, dk, device=gpu_device)
    y, stats = _hip.token_norm_fwd(x, gamma, beta, eps, B, n, h, dk, p)
    dx, dg, db = _hip.token_norm_bwd(x, dy, gamma, stats, B, n, h, dk, p)
    y64, dx64, dg64, db64, _, _ = _ref64(x, dy, gamma, beta, eps, B, n, h, dk, p)
    dxv = dx.reshape(B, n, h, DP)[..., p:Dr]
    assert (dxv[..., gamma == 0] == 0).all()
    assert torch.isfinite(dg).all() and float(dg[gamma == 0].abs().min()) > 0
    assert rel_l2(dg, dg64) < KTOL and rel_l2(db, db64) < KTOL and rel_l2(dxv, dx64) < KTOL
    assert rel_l2(y.reshape(B, n, h, DP)[..., p:Dr], y64) < KTOL


def _no_dropout(mod):
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def _run_fixture(GT, dev, g, train=True):
    torch.manual_seed(0)
    mod = build_module(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = _no_dropout(mod).to(dev)
    mod = mod.train() if train else mod.eval()
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
    worst = max(errs, key=errs.get)
    ratios = {k: v / max(TOL, 12.0 * noise.get(k, 0.0)) for k, v in errs.items()}
    wr = max(ratios, key=ratios.get)
    print(f"{name}: worst {worst} {errs[worst]:.2e}; worst error / bound {wr} {ratios[wr]:.2f}",
          {k: (f"{v:.1e}", f"{noise.get(k, 0.0):.1e}") for k, v in errs.items() if v > 0.5 * TOL})
    bad = {k: (v, max(TOL, 12.0 * noise.get(k, 0.0))) for k, v in errs.items()
           if k != "out" and not v < max(TOL, 12.0 * noise.get(k, 0.0))}
    assert errs["out"] < TOL, errs["out"]
    assert not bad, bad


@pytest.mark.parametrize("name", INSTANCE_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("instance/" + name)
    at = attention_type_of(g)
    out, din, grads = _run_fixture(GT, gpu_device, g)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(din[k], g.din[k]) for k in g.din})
    for k in g.dparam:
        assert grads[k] is not None, k
    errs.update({"dW:" + k: v for k, v in grad_errors(grads, g.dparam, g.sd, at).items()})
    # the float32 restatement's own distance from float64, per tensor (CPU): what 1e-5 can and cannot ask of a gradient
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    noise = {"d" + k: rel_l2(di32[k], di64[k]) for k in di32}
    noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, g.sd, at).items()})
    _gate(name, errs, noise)


def _darcy_layer(GT, at="galerkin"):
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.darcy_config("ex2_darcy141")
    d, h, f = cfg["n_hidden"], cfg["n_head"], cfg["dim_feedforward"]
    kw = dict(d_model=d, pos_dim=2, n_head=h, dim_feedforward=f, attention_type=at, layer_norm=False, attn_norm=True,
              norm_eps=1e-7)
    torch.manual_seed(78)
    layer = GT.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, norm_type="instance", **kw)
    with torch.no_grad():
        for prm in layer.parameters():
            prm.add_(0.02 * torch.randn_like(prm))
    return layer, d, h


@pytest.mark.parametrize("at", ("galerkin", "linear"))
def test_full_size_darcy_layer_vs_float64(GT, gpu_device, at):
    """The ex2_darcy141 encoder shape (1 849 tokens, d 128, 4 heads x (32 + 2), B = 4) with norm_type='instance', attention
    dropout off, against the float64 restatement; the float32 restatement on the CPU gives the per-tensor noise of the gate."""
    layer, d, h = _darcy_layer(GT, at)
    B, n, p = 4, 43 * 43, 2
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    x, pos, cot = torch.randn(B, n, d), torch.rand(B, n, p), torch.randn(B, n, d)
    dev = gpu_device
    layer = _no_dropout(layer).to(dev).train()
    GT.set_attention_dropout("off")
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
        out = encoder_layer(s, xx, pos.to(dtype), n_head=h, attention_type=at, layer_norm=False, attn_norm=True,
                            norm_eps=1e-7)
        gs = torch.autograd.grad(out, [xx] + list(s.values()), cot.to(dtype))
        return out.detach(), gs[0], dict(zip(s, gs[1:]))

    o64, dx64, dp64 = ref(torch.float64)
    o32, dx32, dp32 = ref(torch.float32)
    grads = {k: prm.grad for k, prm in layer.named_parameters()}
    errs = {"out": rel_l2(y, o64), "dx": rel_l2(xg.grad, dx64)}
    errs.update({"dW:" + k: v for k, v in grad_errors(grads, dp64, sd, at).items()})
    noise = {"dx": rel_l2(dx32, dx64)}
    noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, sd, at).items()})
    _gate(f"darcy141 {at} instance layer", errs, noise)


def test_full_size_darcy_layer_reference_dropout(GT, gpu_device):
    """The same layer with the attention dropout in 'reference' mode: finite results, about half of the matrix kept and the
    kept entries doubled."""
    layer, d, h = _darcy_layer(GT)
    B, n, p = 4, 43 * 43, 2
    dev = gpu_device
    layer = _no_dropout(layer).to(dev).train()
    layer.attn_weight = True
    x, pos = torch.randn(B, n, d, device=dev), torch.rand(B, n, p, device=dev)
    GT.set_attention_dropout("off")
    try:
        _, w0 = layer(x, pos)
        GT.set_attention_dropout("reference")
        xg = x.clone().requires_grad_(True)
        y1, w1 = layer(xg, pos)
        y1.square().mean().backward()
        y2, w2 = layer(x, pos)
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    assert w0.shape == (B, h, d // h + p, d // h + p)
    assert torch.isfinite(y1).all() and torch.isfinite(xg.grad).all()
    assert all(prm.grad is not None and torch.isfinite(prm.grad).all() for prm in layer.parameters())
    kept = (w1 != 0)
    assert abs(kept.float().mean().item() - 0.5) < 0.05
    assert torch.allclose(w1[kept], 2 * w0[kept], rtol=1e-5, atol=1e-9)
    assert not torch.equal(w1, w2) and rel_l2(y1, y2) > 1e-6


@pytest.mark.parametrize("name", ("enc_galerkin_inst_c2", "enc_linear_inst_c2"))
def test_eval_equals_train(GT, gpu_device, name):
    """No running statistics: the statistics are per instance in eval() too."""
    g = Golden("instance/" + name)
    a = _run_fixture(GT, gpu_device, g, train=True)
    b = _run_fixture(GT, gpu_device, g, train=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1]["x"], b[1]["x"])
    for k, v in a[2].items():
        assert torch.equal(v, b[2][k]), k


@pytest.mark.parametrize("name", ("enc_galerkin_inst_c2", "enc_linear_inst_c2"))
def test_graph_capture_replays_eager(GT, gpu_device, name):
    g = Golden("instance/" + name)
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
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


_ISOLATION = r"""
import sys, torch
root, out, first = sys.argv[1], sys.argv[2], sys.argv[3] == "1"
for p in (root, root + "/galerkin-transformer_amd", root + "/tests"):
    sys.path.insert(0, p)
import galerkin_transformer as GT
from _util import Golden
from test_instance_norm_gpu import _run_fixture
dev = torch.device("cuda:0")
if first:
    for name in ("enc_galerkin_inst_c2", "enc_linear_inst_c2"):
        _run_fixture(GT, dev, Golden("instance/" + name))
res = {}
for name in ("enc_galerkin_c2", "linear/enc_linear_c2"):
    o, di, gr = _run_fixture(GT, dev, Golden(name))
    res[name] = [o.cpu(), di["x"].cpu()] + [gr[k].cpu() for k in sorted(gr)]
torch.save(res, out)
"""


def test_layernorm_paths_are_untouched(GT, gpu_device):
    """With instance-norm layers built and run first in the same process, the LayerNorm 'galerkin' and 'linear' fixtures give
    the bits a fresh process gives."""
    with tempfile.TemporaryDirectory() as tmp:
        outs = []
        for first in ("0", "1"):
            path = os.path.join(tmp, f"iso{first}.pt")
            r = subprocess.run([sys.executable, "-c", _ISOLATION, ROOT, path, first], capture_output=True, text=True,
                               timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append(torch.load(path))
    for name, ts in outs[0].items():
        assert len(ts) == len(outs[1][name])
        for a, b in zip(ts, outs[1][name]):
            assert torch.equal(a, b), name


def test_one_token_raises(GT, gpu_device):
    layer = GT.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type="galerkin", layer_norm=False,
                                             norm_type="instance").to(gpu_device)
    with pytest.raises(ValueError, match="more than 1"):
        layer(torch.randn(2, 1, 64, device=gpu_device), torch.rand(2, 1, 2, device=gpu_device))
    y = layer(torch.randn(2, 8, 64, device=gpu_device), torch.rand(2, 8, 2, device=gpu_device))
    assert torch.isfinite(y).all()


def test_models_train_with_instance_norm(GT, gpu_device):
    g = Golden("instance/model_burgers_galerkin_inst_small")
    dev = gpu_device
    for at in ("galerkin", "linear", "global"):
        m = GT.SimpleTransformer(**dict(g.meta["config"], attention_type=at))
        m.load_state_dict(g.sd, strict=True)
        m = m.to(dev).train()
        out = m(g.inputs["node"].to(dev), None, g.inputs["pos"].to(dev))["preds"]
        out.square().mean().backward()
        torch.cuda.synchronize()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    lite = dict(dropout=0.0, encoder_dropout=0.0, decoder_dropout=0.0, ffn_dropout=0.0, xavier_init=0.01,
                diagonal_weight=0.01, node_feats=12, pos_dim=2, n_targets=1, n_hidden=32, num_encoder_layers=1, n_head=2,
                dim_feedforward=64, layer_norm=False, attn_norm=True, decoder_type="ifft2", freq_dim=12,
                num_regressor_layers=1, fourier_modes=4, spacial_dim=2, spacial_fc=False, regressor_activation="silu",
                debug=False, attention_type="galerkin", norm_type="instance")
    m = GT.FourierTransformer2DLite(**lite).to(dev).train()
    assert any(isinstance(x, torch.nn.InstanceNorm1d) for x in m.modules())
    ng = 16
    out = m(torch.randn(2, ng, ng, 10, device=dev), None, torch.rand(2, ng * ng, 2, device=dev),
            torch.rand(2, ng, ng, 2, device=dev))["preds"]
    out.square().mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
