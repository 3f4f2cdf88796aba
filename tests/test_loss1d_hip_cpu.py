"""WeightedL2Loss (1-D) on the HIP operator, CPU side: the host-visible surface (exported symbols, workspace query), the
route predicate, terms() and forward() of CPU tensors unchanged, and the backward gather formula of the kernel (restated in
numpy, tests/_loss1d_ref.py) against autograd of the torch route in float64.  No GPU needed."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from _loss1d_ref import dpreds_np, inputs, oracle64, terms_np
from _util import GOLDEN, rel_l2

NEW_SYMBOLS = {"gt_h1loss1d_ws_bytes": 2, "gt_h1loss1d_fwd": 12, "gt_h1loss1d_final": 14, "gt_h1loss1d_bwd": 16}
SHAPES = ((2, 3, 2), (2, 5, 2), (3, 9, 4), (2, 12, 6))


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = ctypes.CDLL(_hip.lib_path())
    for s, nargs in NEW_SYMBOLS.items():
        (params,) = re.findall(r"\b" + s + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(params.split(",")) == nargs, (s, params)
        assert s in _hip.EXPORTED_SYMBOLS and len(_hip._PROTOS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    assert _hip.lib().gt_abi_version() == 21 and _hip.ABI_VERSION == 21
    assert "#define GT_ABI_VERSION 21" in hdr


def test_workspace_query():
    """Host code: four floats per block, a block per 512 groups of four elements, two groups of slack for the row's ends."""
    from galerkin_transformer import _hip
    q = _hip.lib().gt_h1loss1d_ws_bytes
    assert q(0, 8) == 0 and q(2, 0) == 0 and q(-1, 8) == 0 and q(2, -8) == 0
    blocks = lambda L: -(-(L // 4 + 2) // 512)
    assert blocks(3) == 1 and blocks(64) == 1 and blocks(2048) == 2 and blocks(4099) == 3 and blocks(8192) == 5
    for N, L in ((2, 3), (3, 64), (2, 2048), (3, 4099), (32, 8192)):
        assert q(N, L) == N * blocks(L) * 16, (N, L)


def _dev(shape, requires_grad=False, is_cuda=True, dtype=torch.float32):
    """What the predicate reads of a tensor, without a device."""
    return types.SimpleNamespace(shape=torch.Size(shape), ndim=len(shape), is_cuda=is_cuda, dtype=dtype,
                                 requires_grad=requires_grad)


def test_route_predicate():
    from galerkin_transformer.ft import WeightedL2Loss
    N, L = 4, 64
    lf = WeightedL2Loss(regularizer=True, h=1 / L, gamma=0.5)
    P, T, G = _dev((N, L), True), _dev((N, L)), _dev((N, L))
    # train_batch_burgers with a one-channel and with a two-channel output (alpha is 0), validate_epoch_burgers, no G
    assert lf._hip_terms_ok(P, T, targets_prime=G)
    assert lf._hip_terms_ok(P, T, _dev((N, L), True), G)
    assert lf._hip_terms_ok(_dev((N, L)), T, targets_prime=G)
    assert lf._hip_terms_ok(P, T)
    # one fallback condition each
    assert not lf._hip_terms_ok(_dev((N, L), True, is_cuda=False), T, targets_prime=G)
    assert not lf._hip_terms_ok(_dev((N, L), True, dtype=torch.float64), T, targets_prime=G)
    assert not lf._hip_terms_ok(_dev((N, L, 1), True), T, targets_prime=G)
    assert not lf._hip_terms_ok(_dev((N, 2), True), _dev((N, 2)))                                # L <= dilation
    assert not WeightedL2Loss(regularizer=True, h=1 / L, alpha=0.2)._hip_terms_ok(P, T, _dev((N, L), True), G, K=_dev((N, L)))
    assert not lf._hip_terms_ok(P, _dev((N, L), True), targets_prime=G)
    assert not lf._hip_terms_ok(P, T, targets_prime=_dev((N, L), True))
    assert not lf._hip_terms_ok(P, _dev((N, L + 1)), targets_prime=G)
    assert not lf._hip_terms_ok(P, T, targets_prime=_dev((N, L, 1)))
    assert not lf._hip_terms_ok(P, _dev((N, L), is_cuda=False), targets_prime=G)
    assert not lf._hip_terms_ok(P, T, targets_prime=_dev((N, L), dtype=torch.float64))


@pytest.fixture(scope="module")
def host():
    z = np.load(os.path.join(GOLDEN, "host_losses.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def case_kwargs(z, c):
    """(preds, targets, keyword tensors of terms(), latents or None) of a recorded 1-D case."""
    t = lambda k: torch.from_numpy(np.array(z[k]))
    kw = {}
    if "tprime" in c["use"]:
        kw["targets_prime"] = t("l1/tprime")
    if "pprime" in c["use"]:
        kw["preds_prime"] = t("l1/pprime")
    if "K" in c["use"]:
        kw["K"] = t("l1/K")
    lat = [t("l1/lat0"), t("l1/lat1")] if "lat" in c["use"] else None
    return t("l1/preds"), t("l1/targets"), kw, lat


def test_cpu_tensors_take_the_torch_route_unchanged(host):
    """terms() is _terms_torch() bit for bit, and forward() gives the recorded reference values (the bar of
    test_host_golden_cpu.py: rtol 1e-6, dpreds relative L2 1e-6)."""
    from galerkin_transformer.ft import WeightedL2Loss
    z, idx = host
    assert len(idx["loss1d"]) == 7
    for i, c in enumerate(idx["loss1d"]):
        preds, targets, kw, lat = case_kwargs(z, c)
        lf = WeightedL2Loss(**c["kw"])
        assert not lf._hip_terms_ok(preds, targets, **kw)
        got, want = [], []
        for fn, out in ((lf.terms, got), (lf._terms_torch, want)):
            p = preds.clone().requires_grad_(True)
            loss, reg, norms = fn(p, targets, **kw)
            (gp,) = torch.autograd.grad(loss.sum() + (0 if reg is None else reg.sum()), p)
            out += [loss.detach(), reg if reg is None else reg.detach(), norms["L2"], norms["H1"], gp]
        for a, b in zip(got, want):
            assert type(a) is type(b)
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b, c
        p = preds.clone().requires_grad_(True)
        loss, reg, ortho, metric = lf(p, targets, **kw, **({} if lat is None else dict(preds_latent=lat)))
        (gp,) = torch.autograd.grad((loss + reg + ortho).sum(), p)
        out = torch.stack([loss.detach().reshape(()), reg.detach().reshape(()), ortho.detach().reshape(()),
                           torch.tensor(float(metric))])
        ref = torch.from_numpy(np.array(z[f"l1/{i}/out"]))
        assert torch.allclose(out, ref, rtol=1e-6, atol=1e-9), (i, c, out, ref)
        assert rel_l2(gp, torch.from_numpy(np.array(z[f"l1/{i}/dpreds"]))) < 1e-6, (i, c)


@pytest.mark.parametrize("N,L,d", SHAPES)
def test_gather_formula_matches_autograd_float64(N, L, d):
    """The numpy restatement of what the kernels compute -- values and the backward gather -- against autograd of
    _terms_torch, both in float64: rounding only (1e-12; the two differ by the order of a few sums)."""
    from galerkin_transformer.ft import WeightedL2Loss
    P, T, G, gl, gr = inputs(N, L)
    h, beta, gamma = 1 / L, 0.7, 0.3
    lf = WeightedL2Loss(regularizer=True, dilation=d, h=h, beta=beta, gamma=gamma)
    cfg = dict(d=d, h=h, beta=beta, gamma_h=lf.gamma)
    assert lf.gamma == gamma * h
    ref = oracle64(lf, P, T, G, gl, gr)
    np64 = lambda t: None if t is None else t.double().numpy()
    loss, reg, L2, H1 = terms_np(np64(P), np64(T), np64(G), **cfg)
    for name, v in (("loss", loss), ("reg", reg), ("L2", L2), ("H1", H1)):
        assert np.allclose(v, ref[name].numpy(), rtol=1e-12, atol=0), name
    dP = dpreds_np(np64(P), np64(T), np64(G), L2, H1, np64(gl), np64(gr), **cfg)
    err = np.abs(dP - ref["dP"].numpy()).max() / np.abs(ref["dP"].numpy()).max()
    assert err < 1e-12, err
    # without G: no regulariser, H1 = 1, the gradient is the first term alone
    ref0 = oracle64(WeightedL2Loss(regularizer=False, dilation=d, h=h, beta=beta, gamma=gamma), P, T, gl=gl)
    loss0, reg0, L20, H10 = terms_np(np64(P), np64(T), **cfg)
    assert reg0 is None and ref0["reg"] is None and ref0["H1"] == 1 and np.all(H10 == 1)
    assert np.allclose(loss0, ref0["loss"].numpy(), rtol=1e-12, atol=0)
    dP0 = dpreds_np(np64(P), np64(T), None, L20, H10, np64(gl), None, **cfg)
    assert np.abs(dP0 - ref0["dP"].numpy()).max() < 1e-12 * np.abs(ref0["dP"].numpy()).max()
