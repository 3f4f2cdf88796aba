"""Spectral mode mixing at any channel width (-m gpu): the tiled kernels behind gt_modemix_fwd / gt_modemix_bwd against the
float64 complex einsum, the wide spectral modules against fixtures recorded from the reference
(tests/golden/spectral_wide/), and one training step + graph capture of a 1-D model whose first decoder layer is 128 -> 64.
Before the tiled route every case here raised GtNotSupported."""
import os

import pytest
import torch

from _spectral_wide_ref import WIDE_GOLDEN, wide_golden
from _util import TOL, rel_l2
from test_modules_gpu import build_module, run_module

pytestmark = pytest.mark.gpu

KTOL = 2e-6          # tests/test_kernels_gpu.py: fp32 accumulation-order noise; Y at KTOL, dX and dW at 5 * KTOL
RESIDENT, TILED = 0, 1
SENTINEL = -777.25


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


# (B, Cin, Cout, Q, q_total, q_off), (forward route, backward route, batch slices of the backward).
# The float32 einsum of torch on the CPU is 1.6e-7 .. 4.1e-7 (Y), 2.7e-8 .. 2.2e-7 (dX), 3.1e-8 .. 8.0e-8 (dW) off the
# float64 one on these inputs, 4.1e-7 on Y for the 6144-term sum: four times that stays under KTOL, so every case is held to
# the bounds of test_kernels_gpu.py::test_modemix as they are.
CASES = [
    ((3, 96, 80, 4, 8, 4), (RESIDENT, TILED, 1)),         # backward tiled, forward resident; non-zero q_off
    ((9, 80, 96, 3, 3, 0), (RESIDENT, TILED, 2)),         # the batch crosses one 8-sample pass; the transposed aspect
    ((5, 100, 70, 2, 2, 0), (RESIDENT, TILED, 1)),        # no multiple of 16 or of 4: tile tails on both channel axes
    ((17, 96, 72, 2, 4, 2), (RESIDENT, TILED, 3)),        # three batch slices, slab reduction
    ((2, 160, 136, 2, 4, 2), (TILED, TILED, 1)),          # forward tiled as well
    ((1, 6144, 1, 1, 1, 0), (TILED, TILED, 1)),           # degenerate aspects: a 6144-term contraction in the forward ...
    ((1, 1, 6144, 1, 1, 0), (RESIDENT, TILED, 1)),        # ... and in the data gradient
]


@pytest.mark.parametrize("shape,plan", CASES, ids=["x".join(map(str, s)) for s, _ in CASES])
def test_tiled_kernels_vs_float64(H, gpu_device, shape, plan):
    B, Cin, Cout, Q, qtot, qoff = shape
    dev = gpu_device
    assert H.modemix_plan(B, Q, Cin, Cout) == plan
    Xc, Wc, cotc = rnd(B, 2, qtot, Cin, seed=35), rnd(Cin, Cout, Q, 2, seed=36, scale=0.3), rnd(B, 2, qtot, Cout, seed=37)
    x64, w64 = Xc.double().requires_grad_(True), Wc.double().requires_grad_(True)
    xc = torch.complex(x64[:, 0, qoff:qoff + Q], x64[:, 1, qoff:qoff + Q])       # [B,Q,Cin]
    wc = torch.complex(w64[..., 0], w64[..., 1])                                  # [Cin,Cout,Q]
    yc = torch.einsum("bqi,ioq->bqo", xc, wc)
    ref = torch.stack([yc.real, yc.imag], 1)
    gx, gw = torch.autograd.grad(ref, [x64, w64], cotc.double()[:, :, qoff:qoff + Q])

    X, W, cot = Xc.to(dev), Wc.to(dev), cotc.to(dev)
    outside = torch.ones(qtot, dtype=torch.bool)
    outside[qoff:qoff + Q] = False
    Y = torch.full((B, 2, qtot, Cout), SENTINEL, device=dev)
    H.modemix_fwd(X, W, Y, B, Q, Cin, Cout, qtot, qoff)

    def backward():
        dX = torch.full((B, 2, qtot, Cin), SENTINEL, device=dev)
        dW = torch.full((Cin, Cout, Q, 2), SENTINEL, device=dev)
        H.modemix_bwd(X, W, cot, dX, dW, B, Q, Cin, Cout, qtot, qoff)
        return dX, dW

    dX, dW = backward()
    dX2, dW2 = backward()
    torch.cuda.synchronize()
    errs = dict(Y=rel_l2(Y[:, :, qoff:qoff + Q], ref.detach()), dX=rel_l2(dX[:, :, qoff:qoff + Q], gx[:, :, qoff:qoff + Q]),
                dW=rel_l2(dW, gw))
    print(shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["Y"] < KTOL, errs
    assert errs["dX"] < 5 * KTOL and errs["dW"] < 5 * KTOL, errs
    # nothing outside [q_off, q_off + Q) is written
    assert (Y[:, :, outside.to(dev)] == SENTINEL).all() and (dX[:, :, outside.to(dev)] == SENTINEL).all()
    assert not gx[:, :, outside].any()
    # the sum over the batch is complete whichever way it is cut (dW above), and the same on a second call
    assert torch.equal(dX, dX2) and torch.equal(dW, dW2)


@pytest.mark.parametrize("name", WIDE_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    """tests/test_modules_gpu.py's check on the wide fixtures: strict load of the reference's state_dict, then output, input
    gradient and every parameter gradient at the project's parity bar."""
    g = wide_golden(name)
    dev = gpu_device
    torch.manual_seed(0)
    mod = build_module(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = mod.to(dev).train()
    ins = {k: v.to(dev) for k, v in g.inputs.items()}
    for k in g.din:
        ins[k].requires_grad_(True)
    out = run_module(mod, g, ins)
    assert out.shape == g.out.shape
    out.backward(g.cot.to(dev))
    torch.cuda.synchronize()
    errs = {"out": rel_l2(out, g.out)}
    for k in g.din:
        errs["d" + k] = rel_l2(ins[k].grad, g.din[k])
    params = dict(mod.named_parameters())
    assert set(g.dparam) == set(params)
    for k, ref in g.dparam.items():
        assert params[k].grad is not None, k
        errs["dW:" + k] = rel_l2(params[k].grad, ref)
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"{name}: {bad}  (worst {max(errs.values()):.2e})"


def test_wide_burgers_model_trains_a_step_and_captures(GT, gpu_device):
    """SimpleTransformer(config.yml: ex1_burgers) at n_hidden 128 / freq_dim 64 (first spectral layer 128 -> 64, 8192 weight
    pairs): forward + WeightedL2Loss + backward captured into one graph replays bit-identically to eager, twice; then one
    FlatClipAdam step runs, with a finite gradient on every parameter and a non-zero one on the wide layer's Fourier weight."""
    import yaml
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "galerkin-transformer_amd", "config.yml")) as f:
        cfg = dict(yaml.full_load(f)["ex1_burgers"], n_hidden=128, n_head=4, attention_type="galerkin", dim_feedforward=256,
                   num_encoder_layers=1, freq_dim=64, fourier_modes=4)
    dev, N, n = gpu_device, 2, 32
    torch.manual_seed(5)
    model = GT.SimpleTransformer(**cfg).to(dev).train()
    wide = "regressor.spectral_conv.0.fourier_weight"
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    wide_keys = [k for k, _ in named if k.startswith(wide)]
    assert wide_keys and all(tuple(dict(named)[k].shape[:2]) == (128, 64) for k in wide_keys)
    assert _hip.modemix_plan(N, 4, 128, 64)[:2] == (RESIDENT, TILED)
    params = [p for _, p in named]
    opt = GT.FlatClipAdam(params, lr=1e-3, max_norm=0.99, model=model)
    lf = GT.WeightedL2Loss(regularizer=True, h=1 / n, gamma=0.5)
    g = torch.Generator().manual_seed(11)
    node = torch.randn(N, n, 1, generator=g).to(dev)
    pos = torch.linspace(0, 1, n)[None, :, None].repeat(N, 1, 1).to(dev)
    u, up = torch.randn(N, n, generator=g).to(dev), (torch.randn(N, n, generator=g) * n).to(dev)

    def total_loss():
        out = model(node, None, pos)["preds"]
        loss, reg, _ = lf.terms(out[..., 0], u, targets_prime=up)
        return lf.reduce(loss) + lf.reduce(reg)

    def step():
        return torch.autograd.grad(total_loss(), params)

    GT.set_attention_dropout("off")
    try:
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
        replays = []
        for _ in range(2):
            graph.replay()
            replays.append([t.clone() for t in captured])
        torch.cuda.synchronize()
        for (k, _), e, r0, r1 in zip(named, eager, *replays):
            assert torch.equal(r0, r1), k
            assert torch.equal(e, r0), k
        del graph, captured

        # one training step
        before = [p.detach().clone() for p in params]
        for p in params:
            p.grad = None
        total = total_loss()
        total.backward()
        opt.gather_grads()
        _hip.weight_packs.invalidate()
        opt.apply()
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    assert torch.isfinite(total)
    for (k, p), e in zip(named, eager):
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        assert torch.equal(p.grad, e), k               # the same inputs and weights as the eager step above
    for k in wide_keys:
        assert dict(named)[k].grad.abs().max() > 0, k
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, params))
