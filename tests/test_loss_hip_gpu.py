"""WeightedL2Loss2d on the HIP operator, on the device (-m gpu): gt_h1loss2d_fwd / _final / _bwd through ft.WeightedL2Loss2d
against ``_terms_torch`` evaluated in float64 on the CPU from the same inputs -- the code under test is never its own oracle.

Bars.  loss, reg, L2, H1: relative 1e-5 per sample (the bar test_modules_gpu.py holds this loss to).  dP: relative L2 below
_util.TOL = 1e-5.  Shapes (N, n, d): (2, 3, 2) one interior point * (2, 5, 2) * (3, 9, 4) * (2, 17, 2) the fixture of
tests/golden/host_losses.npz * (3, 64, 2) three blocks per sample * (2, 141, 2) odd size, ten blocks per sample, a sample
boundary off the 16-byte grid."""
import json
import os

import numpy as np
import pytest
import torch

from _loss_ref import inputs, oracle64
from _util import GOLDEN, TOL, rel_l2

pytestmark = pytest.mark.gpu

VTOL = 1e-5
SHAPES = ((2, 3, 2), (2, 5, 2), (3, 9, 4), (2, 17, 2), (3, 64, 2), (2, 141, 2))
FWD, FINAL, BWD = "gt_h1loss2d_fwd", "gt_h1loss2d_final", "gt_h1loss2d_bwd"


@pytest.fixture(scope="module")
def FT(gpu_device):
    from galerkin_transformer import _hip, ft
    _hip.lib()
    return ft


def _run(lf, P, T, G, K, gl, gr, fn=None):
    """terms (or fn) on the given device tensors and the gradient of (loss gl).sum() + (reg gr).sum() w.r.t. P."""
    p = P.detach().requires_grad_(True)
    loss, reg, norms = (fn or lf.terms)(p, T, targets_prime=G, K=K)
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


@pytest.mark.parametrize("N,n,d", SHAPES)
@pytest.mark.parametrize("use_k", (True, False), ids=("K", "noK"))
def test_terms_match_float64_oracle(FT, gpu_device, N, n, d, use_k):
    P, T, G, K, gl, gr = inputs(N, n)
    K = K if use_k else None
    lf = FT.WeightedL2Loss2d(regularizer=True, dilation=d, h=1 / n, beta=0.7, gamma=0.3)
    ref = oracle64(lf, P, T, G, K, gl, gr)
    _check(_run(lf, *_on(gpu_device, P, T, G, K, gl, gr)), ref, f"reg N{N} n{n} d{d}")


@pytest.mark.parametrize("N,n,d", ((2, 5, 2), (3, 64, 2), (2, 141, 2)))
def test_variants_match_float64_oracle(FT, gpu_device, N, n, d):
    """Validation call (no G, regularizer=False), the norms without the regulariser (G given, regularizer=False), K as
    [N, n, n], and P as channel 0 of an [N, n, n, 2] and of an [N, n, n, 1] tensor (pixel pitch 2 and 1)."""
    dev = gpu_device
    P, T, G, K, gl, gr = inputs(N, n)
    plain = FT.WeightedL2Loss2d(regularizer=False, dilation=d, h=1 / n)
    ref = oracle64(plain, P, T, gl=gl)
    assert ref["reg"] is None and ref["H1"] == 1
    _check(_run(plain, *_on(dev, P, T, None, None, gl, gr)), ref, f"noG n{n}")
    _check(_run(plain, *_on(dev, P, T, G, K, gl, gr)), oracle64(plain, P, T, G, K, gl), f"norms-only n{n}")
    lf = FT.WeightedL2Loss2d(regularizer=True, dilation=d, h=1 / n, gamma=0.5)
    ref = oracle64(lf, P, T, G, K, gl, gr)
    Pd, Td, Gd, Kd, gld, grd = _on(dev, P, T, G, K, gl, gr)
    _check(_run(lf, Pd, Td, Gd, Kd[..., 0].contiguous(), gld, grd), ref, f"K[N,n,n] n{n}")
    for c in (2, 1):
        out = torch.randn(N, n, n, c, device=dev)
        out[..., 0] = Pd
        p = out.requires_grad_(True)
        loss, reg, norms = lf.terms(p[..., 0], Td, targets_prime=Gd, K=Kd)
        (dout,) = torch.autograd.grad((loss * gld).sum() + (reg * grd).sum(), p)
        assert not dout[..., 1:].any()
        _check(dict(loss=loss.detach(), reg=reg.detach(), L2=norms["L2"], H1=norms["H1"], dP=dout[..., 0].contiguous()), ref,
               f"pitch{c} n{n}")


@pytest.fixture(scope="module")
def host():
    z = np.load(os.path.join(GOLDEN, "host_losses.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def test_forward_matches_reference_golden(FT, gpu_device, host):
    """forward() on the device against the values recorded from the reference (N, n, d = 2, 17, 2; the five cases include
    return_norm=False, K, and one with alpha, which stays on the torch route), and against the float64 oracle."""
    from galerkin_transformer import _hip
    z, idx = host
    t = lambda k: torch.from_numpy(np.array(z[k]))
    for i, c in enumerate(idx["loss2d"]):
        kw = {}
        if "tprime" in c["use"]:
            kw["targets_prime"] = t("l2/tprime")
        if "pprime" in c["use"]:
            kw["preds_prime"] = t("l2/pprime")
        if "K" in c["use"]:
            kw["K"] = t("l2/K")
        lf = FT.WeightedL2Loss2d(**c["kw"])
        p = t("l2/preds").to(gpu_device).requires_grad_(True)
        with _hip.Profile() as prof:
            loss, reg, metric, norms = lf(p, t("l2/targets").to(gpu_device), **{k: v.to(gpu_device) for k, v in kw.items()})
            (gp,) = torch.autograd.grad((loss + reg).sum(), p)
        keys = [r[0] for r in prof.records]
        assert keys == ([] if c["kw"].get("alpha") else [FWD, FINAL, BWD]), (i, keys)
        got = torch.stack([loss.detach().reshape(()).cpu(), reg.detach().reshape(()).cpu(), torch.tensor(float(metric))])
        want = t(f"l2/{i}/out")
        print(i, c, ((got - want) / want.clamp_min(1e-30)).abs().tolist(), rel_l2(gp, t(f"l2/{i}/dpreds")))
        assert torch.allclose(got, want, rtol=VTOL, atol=1e-9), (i, c, got, want)
        assert torch.allclose(norms["L2"].detach().cpu(), t(f"l2/{i}/L2"), rtol=VTOL, atol=0), (i, c)
        assert rel_l2(gp, t(f"l2/{i}/dpreds")) < TOL, (i, c)
        # the same call against float64
        p64 = t("l2/preds").double().requires_grad_(True)
        l64, r64, _, n64 = lf(p64, t("l2/targets").double(), **{k: v.double() for k, v in kw.items()})
        (g64,) = torch.autograd.grad((l64 + r64).sum(), p64)
        assert abs(loss.item() - l64.item()) < VTOL * l64.item() and abs(reg.item() - r64.item()) <= VTOL * r64.item()
        assert rel_l2(gp, g64) < TOL, (i, c)


def _keys(prof):
    return [r[0] for r in prof.records if "h1loss2d" in r[0]]


def test_route_is_the_hip_operator(FT, gpu_device):
    from galerkin_transformer import _hip
    P, T, G, K, gl, gr = _on(gpu_device, *inputs(3, 64))
    lf = FT.WeightedL2Loss2d(regularizer=True, h=1 / 64, gamma=0.5)
    with _hip.Profile() as prof:
        _run(lf, P, T, G, K, gl, gr)
    assert _keys(prof) == [FWD, FINAL, BWD]
    with _hip.Profile() as prof, torch.no_grad():
        loss, reg, norms = lf.terms(P, T, targets_prime=G, K=K)
    assert _keys(prof) == [FWD, FINAL] and not loss.requires_grad
    with _hip.Profile() as prof:                 # a prediction without a gradient: nothing to run backwards
        loss, reg, _ = lf.terms(P, T, targets_prime=G, K=K)
    assert _keys(prof) == [FWD, FINAL] and not loss.requires_grad and not reg.requires_grad


def test_reruns_are_bit_identical(FT, gpu_device):
    P, T, G, K, gl, gr = _on(gpu_device, *inputs(2, 141))
    lf = FT.WeightedL2Loss2d(regularizer=True, h=1 / 141, gamma=0.5)
    a, b = _run(lf, P, T, G, K, gl, gr), _run(lf, P, T, G, K, gl, gr)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_weights_fall_back_to_torch(FT, gpu_device):
    from galerkin_transformer import _hip
    N, n = 2, 17
    P, T, G, K, gl, gr = _on(gpu_device, *inputs(N, n))
    w = torch.rand(N, device=gpu_device) + 0.5
    lf = FT.WeightedL2Loss2d(regularizer=True, h=1 / n, gamma=0.5)
    with _hip.Profile() as prof:
        got = _run(lf, P, T, G, K, gl, gr, fn=lambda *a, **kw: lf.terms(*a, weights=w, **kw))
    assert _keys(prof) == []
    want = _run(lf, P, T, G, K, gl, gr, fn=lambda *a, **kw: lf._terms_torch(*a, weights=w, **kw))
    for k in got:
        assert torch.equal(got[k], want[k]), k
    ref = oracle64(lf, P, T, G, K, gl, gr, weights=w)
    _check(got, ref, "weights")


def test_graph_capture_replays_with_new_predictions(FT, gpu_device):
    """terms + reduce + backward captured once; two replays with other predictions give what eager calls give, bit for bit."""
    dev = gpu_device
    N, n = 3, 64
    P, T, G, K, _, _ = _on(dev, *inputs(N, n))
    lf = FT.WeightedL2Loss2d(regularizer=True, h=1 / n, gamma=0.5)
    static = torch.zeros(N, n, n, 1, device=dev, requires_grad=True)

    def step():
        loss, reg, _ = lf.terms(static[..., 0], T, targets_prime=G, K=K)
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
    ref = oracle64(lf, preds[2], T, G, K)      # and the replayed values are the right ones
    want = ref["loss"].sqrt().mean() + ref["reg"].sqrt().mean()
    assert abs(float(captured[0]) - float(want)) < VTOL * float(want)
