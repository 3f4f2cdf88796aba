"""WeightedL2Loss (1-D) on the HIP operator, on the device (-m gpu): gt_h1loss1d_fwd / _final / _bwd through
ft.WeightedL2Loss against ``_terms_torch`` evaluated in float64 on the CPU from the same inputs -- the code under test is
never its own oracle.

Bars.  loss, reg, L2, H1: relative 1e-5 per sample (VTOL of test_loss_hip_gpu.py).  dP: relative L2 below _util.TOL = 1e-5.
Shapes (N, L, d): (2, 3, 2) one interior point * (2, 5, 2) * (3, 9, 4) * (3, 64, 2) the fixture of
tests/golden/host_losses.npz * (2, 2048, 2) two blocks per sample * (3, 4099, 2) odd length, three blocks per sample, a
sample boundary off the 16-byte grid."""
import json
import os

import numpy as np
import pytest
import torch

from _loss1d_ref import inputs, oracle64
from _util import GOLDEN, TOL, Golden, rel_l2

pytestmark = pytest.mark.gpu

VTOL = 1e-5
SHAPES = ((2, 3, 2), (2, 5, 2), (3, 9, 4), (3, 64, 2), (2, 2048, 2), (3, 4099, 2))
FWD, FINAL, BWD = "gt_h1loss1d_fwd", "gt_h1loss1d_final", "gt_h1loss1d_bwd"


@pytest.fixture(scope="module")
def FT(gpu_device):
    from galerkin_transformer import _hip, ft
    _hip.lib()
    return ft


def _run(lf, P, T, G, gl, gr, fn=None):
    """terms (or fn) on the given device tensors and the gradient of (loss gl).sum() + (reg gr).sum() w.r.t. P."""
    p = P.detach().requires_grad_(True)
    loss, reg, norms = (fn or lf.terms)(p, T, targets_prime=G)
    total = (loss * gl).sum()
    if reg is not None:
        total = total + (reg * gr).sum()
    (dP,) = torch.autograd.grad(total, p)
    return dict(loss=loss.detach(), reg=None if reg is None else reg.detach(), L2=norms["L2"], H1=norms["H1"], dP=dP)


def _check(got, ref, what):
    errs = {}
    for k in ("loss", "reg", "L2", "H1"):
        a, b = got[k], ref[k]
        assert (a is None) == (b is None) and torch.is_tensor(a) == torch.is_tensor(b), (what, k)
        if a is None or not torch.is_tensor(a):
            assert a == b, (what, k)
            continue
        assert a.dtype == torch.float32 and a.shape == b.shape, (what, k)
        errs[k] = float(((a.double().cpu() - b) / b).abs().max())
    errs["dP"] = rel_l2(got["dP"], ref["dP"])
    print(what, {k: f"{v:.1e}" for k, v in errs.items()})
    assert got["dP"].shape == ref["dP"].shape and got["dP"].is_contiguous()
    for k, v in errs.items():
        assert v < (TOL if k == "dP" else VTOL), (what, k, v)
    return errs


def _on(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _keys(prof):
    return [r[0] for r in prof.records if "h1loss1d" in r[0]]


@pytest.mark.parametrize("N,L,d", SHAPES)
def test_terms_match_float64_oracle(FT, gpu_device, N, L, d):
    P, T, G, gl, gr = inputs(N, L)
    lf = FT.WeightedL2Loss(regularizer=True, dilation=d, h=1 / L, beta=0.7, gamma=0.3)
    ref = oracle64(lf, P, T, G, gl, gr)
    assert ref["reg"] is not None
    _check(_run(lf, *_on(gpu_device, P, T, G, gl, gr)), ref, f"reg N{N} L{L} d{d}")


@pytest.mark.parametrize("N,L,d", ((2, 5, 2), (3, 64, 2), (3, 4099, 2)))
def test_variants_match_float64_oracle(FT, gpu_device, N, L, d):
    """Validation call (no G, regularizer=False), the norms without the regulariser (G given, regularizer=False), gamma = 0,
    and P as channel 0 of an [N, L, 2] and of an [N, L, 1] tensor (element pitch 2 and 1)."""
    dev = gpu_device
    P, T, G, gl, gr = inputs(N, L)
    plain = FT.WeightedL2Loss(regularizer=False, dilation=d, h=1 / L)
    ref = oracle64(plain, P, T, gl=gl)
    assert ref["reg"] is None and ref["H1"] == 1
    _check(_run(plain, *_on(dev, P, T, None, gl, gr)), ref, f"noG L{L}")
    ref = oracle64(plain, P, T, G, gl)
    assert ref["reg"] is None and torch.is_tensor(ref["H1"])
    _check(_run(plain, *_on(dev, P, T, G, gl, gr)), ref, f"norms-only L{L}")
    nogamma = FT.WeightedL2Loss(regularizer=True, dilation=d, h=1 / L, gamma=0.0)
    ref = oracle64(nogamma, P, T, G, gl)
    assert ref["reg"] is None
    _check(_run(nogamma, *_on(dev, P, T, G, gl, gr)), ref, f"gamma0 L{L}")
    lf = FT.WeightedL2Loss(regularizer=True, dilation=d, h=1 / L, gamma=0.5)
    ref = oracle64(lf, P, T, G, gl, gr)
    Pd, Td, Gd, gld, grd = _on(dev, P, T, G, gl, gr)
    for c in (2, 1):
        out = torch.randn(N, L, c, device=dev)
        out[..., 0] = Pd
        p = out.requires_grad_(True)
        loss, reg, norms = lf.terms(p[..., 0], Td, targets_prime=Gd)
        (dout,) = torch.autograd.grad((loss * gld).sum() + (reg * grd).sum(), p)
        assert not dout[..., 1:].any()
        _check(dict(loss=loss.detach(), reg=reg.detach(), L2=norms["L2"], H1=norms["H1"], dP=dout[..., 0].contiguous()), ref,
               f"pitch{c} L{L}")


@pytest.fixture(scope="module")
def host():
    z = np.load(os.path.join(GOLDEN, "host_losses.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def test_forward_matches_reference_golden(FT, gpu_device, host):
    """forward() on the device against the values recorded from the reference (N, L, d = 3, 64, 2; the seven cases include
    return_norm=False, the three metrics, the orthogonaliser, and one with alpha, which stays on the torch route)."""
    from galerkin_transformer import _hip
    dev = gpu_device
    z, idx = host
    t = lambda k: torch.from_numpy(np.array(z[k]))
    assert len(idx["loss1d"]) == 7
    for i, c in enumerate(idx["loss1d"]):
        kw = {}
        if "tprime" in c["use"]:
            kw["targets_prime"] = t("l1/tprime").to(dev)
        if "pprime" in c["use"]:
            kw["preds_prime"] = t("l1/pprime").to(dev)
        if "K" in c["use"]:
            kw["K"] = t("l1/K").to(dev)
        lat = [t("l1/lat0").to(dev), t("l1/lat1").to(dev)] if "lat" in c["use"] else None
        if lat is not None:
            kw["preds_latent"] = lat
        lf = FT.WeightedL2Loss(**c["kw"])
        p = t("l1/preds").to(dev).requires_grad_(True)
        with _hip.Profile() as prof:
            loss, reg, ortho, metric = lf(p, t("l1/targets").to(dev), **kw)
            (gp,) = torch.autograd.grad((loss + reg + ortho).sum(), p)
        keys = [r[0] for r in prof.records]
        assert keys == ([] if c["kw"].get("alpha") else [FWD, FINAL, BWD]), (i, keys)
        got = torch.stack([loss.detach().reshape(()).cpu(), reg.detach().reshape(()).cpu(), ortho.detach().reshape(()).cpu(),
                           torch.tensor(float(metric))])
        want = t(f"l1/{i}/out")
        print(i, c, got.tolist(), want.tolist(), rel_l2(gp, t(f"l1/{i}/dpreds")))
        assert torch.equal(got[want == 0], want[want == 0]), (i, c, got, want)          # the [0.0] placeholders
        assert torch.allclose(got, want, rtol=VTOL, atol=0), (i, c, got, want)
        assert rel_l2(gp, t(f"l1/{i}/dpreds")) < TOL, (i, c)
        if lat is not None:
            assert torch.equal(ortho, lf._orthogonalizer(lat)), (i, c)


def test_route_is_the_hip_operator(FT, gpu_device):
    from galerkin_transformer import _hip
    P, T, G, gl, gr = _on(gpu_device, *inputs(3, 64))
    lf = FT.WeightedL2Loss(regularizer=True, h=1 / 64, gamma=0.5)
    assert lf._hip_terms_ok(P, T, targets_prime=G)
    with _hip.Profile() as prof:
        _run(lf, P, T, G, gl, gr)
    assert _keys(prof) == [FWD, FINAL, BWD]
    with _hip.Profile() as prof, torch.no_grad():
        loss, reg, norms = lf.terms(P, T, targets_prime=G)
    assert _keys(prof) == [FWD, FINAL] and not loss.requires_grad and not reg.requires_grad
    with _hip.Profile() as prof:                 # a prediction without a gradient: nothing to run backwards
        loss, reg, _ = lf.terms(P, T, targets_prime=G)
    assert _keys(prof) == [FWD, FINAL] and not loss.requires_grad and not reg.requires_grad


def test_reruns_are_bit_identical(FT, gpu_device):
    P, T, G, gl, gr = _on(gpu_device, *inputs(3, 4099))
    lf = FT.WeightedL2Loss(regularizer=True, h=1 / 4099, gamma=0.5)
    a, b = _run(lf, P, T, G, gl, gr), _run(lf, P, T, G, gl, gr)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n_targets", (1, 2))
def test_call_forms_of_train_batch_burgers(FT, gpu_device, n_targets):
    """The loss calls of train_batch_burgers on the output of a tiny SimpleTransformer (one forward, shared by both routes):
    loss + reg and every parameter gradient of the HIP route against the torch route.  With two targets the call passes the
    second channel as preds_prime (alpha = 0): the HIP route, and that channel gets no gradient."""
    from galerkin_transformer import _hip
    import galerkin_transformer as GT
    dev = gpu_device
    N, n = 2, 64
    cfg = dict(Golden("model_burgers_small").meta["config"], n_hidden=32, n_head=2, num_encoder_layers=1, n_targets=n_targets,
               dropout=0.0, encoder_dropout=0.0, ffn_dropout=0.0, decoder_dropout=0.0)
    torch.manual_seed(7)
    m = GT.SimpleTransformer(**cfg).to(dev).train()
    g = torch.Generator().manual_seed(11)
    node = torch.randn(N, n, 1, generator=g).to(dev)
    pos = torch.linspace(0, 1, n)[None, :, None].repeat(N, 1, 1).to(dev)
    u, up = torch.randn(N, n, generator=g).to(dev), (torch.randn(N, n, generator=g) * n).to(dev)
    lf = FT.WeightedL2Loss(regularizer=True, h=1 / n, gamma=0.5)
    params = [p for p in m.parameters() if p.requires_grad]
    out = m(node, None, pos)["preds"]
    assert out.shape == (N, n, n_targets)

    def call(terms):
        if n_targets == 2:
            loss, reg, _ = terms(out[..., 0], u, out[..., 1], up)
        else:
            loss, reg, _ = terms(out[..., 0], u, targets_prime=up)
        total = lf.reduce(loss) + lf.reduce(reg)
        return total.detach(), torch.autograd.grad(total, [out] + params, retain_graph=True, allow_unused=True)

    with _hip.Profile() as prof:
        hip = call(lf.terms)
    assert _keys(prof) == [FWD, FINAL, BWD]
    ref = call(lf._terms_torch)
    assert abs(float(hip[0]) - float(ref[0])) < VTOL * abs(float(ref[0]))
    if n_targets == 2:
        assert not hip[1][0][..., 1].any()
    for a, b, name in zip(hip[1], ref[1], ["out"] + [k for k, p in m.named_parameters() if p.requires_grad]):
        assert (a is None) == (b is None), name
        if a is not None:
            assert rel_l2(a, b) < TOL, (name, rel_l2(a, b))


def test_graph_capture_replays_with_new_predictions(FT, gpu_device):
    """terms + reduce + backward captured once; two replays with other predictions give what eager calls give, bit for bit."""
    dev = gpu_device
    N, L = 3, 4099
    P, T, G, _, _ = _on(dev, *inputs(N, L))
    lf = FT.WeightedL2Loss(regularizer=True, h=1 / L, gamma=0.5)
    static = torch.zeros(N, L, 1, device=dev, requires_grad=True)

    def step():
        loss, reg, _ = lf.terms(static[..., 0], T, targets_prime=G)
        total = lf.reduce(loss) + lf.reduce(reg)
        # detached: a kept reference to an eager step's autograd graph keeps the leaf's AccumulateGrad node of the default
        # stream alive, and the engine would then synchronise that stream with the capturing one in the middle of the capture
        return total.detach(), torch.autograd.grad(total, static)[0]

    def load(p):
        with torch.no_grad():
            static[..., 0].copy_(p)

    preds = [P, P + 0.1 * torch.randn_like(P), T + 0.01 * torch.randn_like(P)]
    eager = []
    for p in preds:
        load(p)
        eager.append([t.clone() for t in step()])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for p, want in zip(preds[1:], eager[1:]):
        load(p)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured[0], want[0]) and torch.equal(captured[1], want[1])
    ref = oracle64(lf, preds[2], T, G)      # and the replayed values are the right ones
    want = ref["loss"].sqrt().mean() + ref["reg"].sqrt().mean()
    assert abs(float(captured[0]) - float(want)) < VTOL * float(want)
    assert rel_l2(captured[1][..., 0], _reduced_grad64(lf, preds[2], T, G)) < TOL


def _reduced_grad64(lf, P, T, G):
    """d(reduce(loss) + reduce(reg)) / dP of the torch route in float64 on the CPU."""
    f64 = lambda t: t.detach().double().cpu()
    p = f64(P).requires_grad_(True)
    loss, reg, _ = lf._terms_torch(p, f64(T), targets_prime=f64(G))
    return torch.autograd.grad(lf.reduce(loss) + lf.reduce(reg), p)[0]
