"""WeightedL2Loss2d on the HIP operator, CPU side: the host-visible surface (exported symbols, workspace query), the route
predicate, terms() of CPU tensors unchanged bit for bit, and the backward gather formula of the kernel (restated in numpy,
tests/_loss_ref.py) against autograd of the torch route in float64.  No GPU needed."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from _loss_ref import dpreds_np, inputs, oracle64, terms_np
from _util import GOLDEN

NEW_SYMBOLS = {"gt_h1loss2d_ws_bytes": 2, "gt_h1loss2d_fwd": 13, "gt_h1loss2d_final": 15, "gt_h1loss2d_bwd": 17}
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
    """Host code: four floats per block, a block per 512 groups of four pixels, two groups of slack for the sample's ends."""
    from galerkin_transformer import _hip
    q = _hip.lib().gt_h1loss2d_ws_bytes
    assert q(0, 8) == 0 and q(2, 0) == 0 and q(-1, 8) == 0
    blocks = lambda n: -(-(n * n // 4 + 2) // 512)
    assert blocks(3) == 1 and blocks(64) == 3 and blocks(141) == 10
    for N, n in ((2, 3), (3, 64), (2, 141), (128, 141)):
        assert q(N, n) == N * blocks(n) * 16, (N, n)


@pytest.fixture(scope="module")
def host():
    z = np.load(os.path.join(GOLDEN, "host_losses.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _case_kwargs(z, c):
    t = lambda k: torch.from_numpy(np.array(z[k]))
    kw = {}
    if "tprime" in c["use"]:
        kw["targets_prime"] = t("l2/tprime")
    if "pprime" in c["use"]:
        kw["preds_prime"] = t("l2/pprime")
    if "K" in c["use"]:
        kw["K"] = t("l2/K")
    return t("l2/preds"), t("l2/targets"), kw


def test_terms_on_cpu_tensors_is_the_torch_route_bit_for_bit(host):
    from galerkin_transformer.ft import WeightedL2Loss2d
    z, idx = host
    assert len(idx["loss2d"]) == 5
    for c in idx["loss2d"]:
        preds, targets, kw = _case_kwargs(z, c)
        lf = WeightedL2Loss2d(**c["kw"])
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


def _dev(shape, requires_grad=False, is_cuda=True, dtype=torch.float32):
    """What the predicate reads of a tensor, without a device."""
    return types.SimpleNamespace(shape=torch.Size(shape), ndim=len(shape), is_cuda=is_cuda, dtype=dtype,
                                 requires_grad=requires_grad)


def test_route_predicate():
    from galerkin_transformer.ft import WeightedL2Loss2d
    N, n = 4, 17
    lf = WeightedL2Loss2d(regularizer=True, h=1 / n, gamma=0.5)
    P, T, G, K = _dev((N, n, n), True), _dev((N, n, n)), _dev((N, n, n, 2)), _dev((N, n, n, 1))
    # the call forms of train_batch_darcy (with and without a predicted gradient; alpha is 0), validation, ns_lite, bench
    assert lf._hip_terms_ok(P, T, targets_prime=G, K=K)
    assert lf._hip_terms_ok(P, T, _dev((N, n, n, 2), True), G, K=K)
    assert lf._hip_terms_ok(_dev((N, n, n)), T)
    assert lf._hip_terms_ok(P, T, targets_prime=G)
    assert lf._hip_terms_ok(P, T, targets_prime=G, K=_dev((N, n, n)))
    # one fallback condition each
    assert not lf._hip_terms_ok(_dev((N, n, n), True, is_cuda=False), T, targets_prime=G, K=K)
    assert not lf._hip_terms_ok(_dev((N, n, n), True, dtype=torch.float64), T, targets_prime=G, K=K)
    assert not lf._hip_terms_ok(_dev((N, n, n, 1), True), T, targets_prime=G, K=K)
    assert not lf._hip_terms_ok(_dev((N, 2, 2), True), _dev((N, 2, 2)))                       # n <= dilation
    assert not lf._hip_terms_ok(P, T, targets_prime=G, K=K, weights=_dev((N, 1, 1)))
    assert not WeightedL2Loss2d(regularizer=True, h=1 / n, alpha=0.2)._hip_terms_ok(P, T, _dev((N, n, n, 2), True), G, K=K)
    assert not lf._hip_terms_ok(P, _dev((N, n, n), True), targets_prime=G, K=K)
    assert not lf._hip_terms_ok(P, T, targets_prime=_dev((N, n, n, 2), True), K=K)
    assert not lf._hip_terms_ok(P, T, targets_prime=G, K=_dev((N, n, n, 1), True))
    assert not lf._hip_terms_ok(P, T, targets_prime=G, K=_dev((N, 1, 1, 1)))
    assert not lf._hip_terms_ok(P, T, targets_prime=G, K=_dev((N, n, n, 2)))
    assert not WeightedL2Loss2d(dim=3, h=1 / n)._hip_terms_ok(P, T, targets_prime=G, K=K)


@pytest.mark.parametrize("N,n,d", SHAPES)
@pytest.mark.parametrize("use_k", (True, False), ids=("K", "noK"))
def test_gather_formula_matches_autograd_float64(N, n, d, use_k):
    """The numpy restatement of what the kernels compute -- values and the backward gather -- against autograd of
    _terms_torch, both in float64: rounding only (1e-12; the two differ by the order of a few sums)."""
    from galerkin_transformer.ft import WeightedL2Loss2d
    P, T, G, K, gl, gr = inputs(N, n)
    K = K if use_k else None
    cfg = dict(h=1 / n, beta=0.7, gamma=0.3)
    lf = WeightedL2Loss2d(regularizer=True, dilation=d, eps=1e-10, **cfg)
    ref = oracle64(lf, P, T, G, K, gl, gr)
    np64 = lambda t: None if t is None else t.double().numpy()
    loss, reg, L2, H1 = terms_np(np64(P), np64(T), np64(G), np64(K), d=d, eps=1e-10, **cfg)
    for name, v in (("loss", loss), ("reg", reg), ("L2", L2), ("H1", H1)):
        assert np.allclose(v, ref[name].numpy(), rtol=1e-12, atol=0), name
    dP = dpreds_np(np64(P), np64(T), np64(G), np64(K), L2, H1, np64(gl), np64(gr), d=d, **cfg)
    err = np.abs(dP - ref["dP"].numpy()).max() / np.abs(ref["dP"].numpy()).max()
    assert err < 1e-12, err
    # without G: no regulariser, H1 = 1, the gradient is the first term alone
    ref0 = oracle64(WeightedL2Loss2d(regularizer=False, dilation=d, **cfg), P, T, gl=gl)
    loss0, reg0, L20, H10 = terms_np(np64(P), np64(T), d=d, **cfg)
    assert reg0 is None and ref0["reg"] is None and ref0["H1"] == 1 and np.all(H10 == 1)
    assert np.allclose(loss0, ref0["loss"].numpy(), rtol=1e-12, atol=0)
    dP0 = dpreds_np(np64(P), np64(T), None, None, L20, H10, np64(gl), None, d=d, **cfg)
    assert np.abs(dP0 - ref0["dP"].numpy()).max() < 1e-12 * np.abs(ref0["dP"].numpy()).max()
