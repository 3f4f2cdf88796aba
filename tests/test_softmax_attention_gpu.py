"""attention_type='softmax' on the device (-m gpu): the fused and the row-softmax kernels through the C ABI against float64,
the two routes against each other, the modules against the fixtures recorded from the reference (tests/golden/softmax/), and
the behaviour around them (unsupported widths, nothing leaking into the Galerkin path, graph capture).

Bars.  Kernels: KTOL = 2e-6 relative L2 (the kernel suites' bar) for O, L, dQ', dK', dV', D.  At n = 1 the softmax is the
constant 1, dS = P (m dPm - D) cancels exactly and the float64 dQ', dK' are zero: there the absolute error is taken relative
to the size of the same product without the cancellation, (P .* m .* dPm) K' * scale and its transpose product, at the same
bar.  Large-range case: max(KTOL, 12 x the float32 CPU restatement's own deviation from float64 on those inputs), computed in
the test on the CPU.  Routes: 1e-5.  Modules: TOL = 1e-5 for the output, dx and every parameter gradient, or
max(TOL, 12 x the float32 restatement's deviation from float64) per tensor (the rule of test_fullsize_models_gpu._gate,
computed on the CPU, never from the device run).  Deviations of the float32 restatement from float64 measured on the CPU
(test_softmax_attention_cpu.py::test_restatement_fp64_envelope), largest per fixture:
    enc_softmax_c2 1.2e-06 (attn.linears.1.bias), _replay 9.6e-07, enc_softmax_c1 7.6e-07, enc_softmax_c4_ln 4.0e-07,
    _replay 4.2e-07, enc_softmax_weights 9.7e-07, model_burgers_softmax_small 4.8e-06 (encoder_layers.0.attn.norm_Q.0.bias;
    nine tensors between 2e-6 and 5e-6).
Gradients that vanish in exact arithmetic (the bias in front of K': _softmax_ref.zero_grad_params) are measured absolutely,
against the size of the sibling weight's gradient (_linear_ref.grad_errors), at the same bars."""
import math
import os

import numpy as np
import pytest
import torch

from _softmax_ref import SOFTMAX_GOLDEN, core, grad_errors, ref_grads
from _util import GOLDEN, Golden, TOL, rel_l2
from test_modules_gpu import build_module, run_module

pytestmark = pytest.mark.gpu

KTOL = 2e-6
NS = (1, 63, 64, 65, 129, 257)
B_, H_ = 2, 2


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


def _tiles(n, DP, seed, big=False):
    """Head tiles [B*n, h, DP], unit normal, with two zero pad columns; big: entries shifted by +-80."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B_ * n, H_, DP, generator=g)
    if big:
        x = x + 80.0 * torch.sign(torch.randn(B_ * n, H_, DP, generator=g))
    x[..., DP - 2:] = 0
    return x


def _heads(t, n):
    return t.reshape(B_, n, H_, t.shape[-1]).permute(0, 2, 1, 3)


def _formula(Q, K, V, dO, n, scale, m, dtype):
    """The issue's formulas in ``dtype`` on the CPU: dict of O, L, dQ, dK, dV, D (+ the uncancelled dQ / dK products)."""
    q, k, v = (_heads(t.cpu(), n).to(dtype).requires_grad_(True) for t in (Q, K, V))
    do = _heads(dO.cpu(), n).to(dtype)
    mm = None if m is None else m.cpu().to(dtype)
    o, pm, L = core(q, k, v, scale, mm)
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], do)
    raw = pm.detach() * (do @ v.detach().transpose(-1, -2)) * (1.0 if mm is None else mm)
    return dict(O=o.detach(), L=L.detach(), dQ=dq, dK=dk, dV=dv, D=(do * o.detach()).sum(-1), Pm=pm.detach(),
                dQ_raw=raw @ k.detach() * scale, dK_raw=raw.transpose(-1, -2) @ q.detach() * scale)


def _device_run(_hip, dev, Q, K, V, dO, n, DP, scale, mask, drop):
    Qd, Kd, Vd, dOd = (t.to(dev) for t in (Q, K, V, dO))
    md = None if mask is None else mask.to(dev).contiguous()
    O, L = _hip.softmax_attn_fwd(Qd, Kd, Vd, B_, n, H_, DP, scale, md, drop)
    dQ, dK, dV, D = _hip.softmax_attn_bwd(dOd, O, Qd, Kd, Vd, L, B_, n, H_, DP, scale, md, drop)
    O2, L2 = _hip.softmax_attn_fwd(Qd, Kd, Vd, B_, n, H_, DP, scale, md, drop)
    dQ2, dK2, dV2, D2 = _hip.softmax_attn_bwd(dOd, O2, Qd, Kd, Vd, L2, B_, n, H_, DP, scale, md, drop)
    torch.cuda.synchronize()
    got = dict(O=O, L=L[0], dQ=dQ, dK=dK, dV=dV, D=D)         # (L[1]: the rounding residual of L[0], gt_hip.h)
    for k, t in dict(O=O2, L=L2[0], dQ=dQ2, dK=dK2, dV=dV2, D=D2).items():
        assert torch.equal(got[k], t), ("second call differs", k)
    for k in ("O", "dQ", "dK", "dV"):
        assert (got[k][..., DP - 2:] == 0).all(), ("pad columns", k)
        assert torch.isfinite(got[k]).all(), k
    assert torch.isfinite(L).all() and torch.isfinite(D).all() and torch.equal(L, L2)
    return {k: (_heads(t, n) if t.dim() == 3 and t.shape[-1] == DP else t).cpu() for k, t in got.items()}


def _draw_mask(_hip, dev, n, drop):
    """The mask the kernels draw for ``drop``: gt_dropout_apply over ones [B, h, n, n] (same element index)."""
    return _hip.dropout_apply(torch.ones(B_, H_, n, n, device=dev), drop)


@pytest.mark.parametrize("mode", ("plain", "dropout", "mask"))
@pytest.mark.parametrize("DP", (20, 36, 52))
def test_fused_kernels_vs_float64(GT, gpu_device, DP, mode):
    from galerkin_transformer import _hip
    dev = gpu_device
    scale = 1.0 / math.sqrt(DP - 2)
    _hip.set_seed(20261018)
    for n in NS:
        Q, K, V, dO = (_tiles(n, DP, 100 * DP + 10 * n + i) for i in range(4))
        mask = drop = m = None
        if mode == "dropout":
            drop = _hip.dropout_desc(0.5, 77 + n, dev)
            m = _draw_mask(_hip, dev, n, drop)
            assert set(m.unique().tolist()) <= {0.0, 2.0}
        elif mode == "mask":
            mask = m = (torch.rand(B_, H_, n, n, generator=torch.Generator().manual_seed(n)) >= 0.5).float() * 2.0
        got = _device_run(_hip, dev, Q, K, V, dO, n, DP, scale, mask, drop)
        ref = _formula(Q, K, V, dO, n, scale, m, torch.float64)
        for k in ("O", "L", "dQ", "dK", "dV", "D"):
            den = ref[k]
            if n == 1 and k in ("dQ", "dK"):            # exact cancellation (module docstring): the uncancelled product
                assert float(ref[k].norm()) < 1e-12 * float(ref[k + "_raw"].norm()) or float(ref[k + "_raw"].norm()) == 0
                den = ref[k + "_raw"]
            e = float((got[k].double() - ref[k]).norm()) / (float(den.norm()) or 1.0)
            print(f"DP {DP} {mode} n {n} {k}: {e:.2e}")
            assert e < KTOL, (DP, mode, n, k, e)


@pytest.mark.parametrize("DP", (20, 36, 52))
def test_large_range(GT, gpu_device, DP):
    """Tile entries shifted by +-80: the scores overflow exp() without the running maximum."""
    from galerkin_transformer import _hip
    n, scale = 65, 1.0 / math.sqrt(DP - 2)
    Q, K, V, dO = (_tiles(n, DP, 7000 + 10 * DP + i, big=True) for i in range(4))
    ref = _formula(Q, K, V, dO, n, scale, None, torch.float64)
    r32 = _formula(Q, K, V, dO, n, scale, None, torch.float32)
    assert float(ref["L"].abs().max()) > 100.0                 # exp(L) is not a float32
    got = _device_run(_hip, gpu_device, Q, K, V, dO, n, DP, scale, None, None)
    for k in ("O", "L", "dQ", "dK", "dV", "D"):
        bound = max(KTOL, 12.0 * rel_l2(r32[k], ref[k]))
        e = rel_l2(got[k], ref[k])
        print(f"DP {DP} big {k}: {e:.2e} (bound {bound:.2e})")
        assert e < bound, (DP, k, e, bound)


def test_other_widths_are_refused(GT, gpu_device):
    from galerkin_transformer import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    x = torch.zeros(64, 1, 68, device=gpu_device)
    s = torch.zeros(128, device=gpu_device)
    for DP in (16, 44, 68):
        assert lib.gt_softmax_attn_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), s.data_ptr(), 1, 64, 1, DP,
                                       1.0, None, None, st) == -4


@pytest.mark.parametrize("n", (1, 65, 257))
def test_row_softmax_kernels(GT, gpu_device, n):
    from galerkin_transformer import _hip
    dev = gpu_device
    g = torch.Generator().manual_seed(n)
    S = (3.0 * torch.randn(B_, H_, n, n, generator=g)).to(dev)
    dPm = torch.randn(B_, H_, n, n, generator=g).to(dev)
    _hip.set_seed(5)
    drop = _hip.dropout_desc(0.5, 9, dev)
    for m, mask, d in ((None, None, None), (_draw_mask(_hip, dev, n, drop), None, drop),
                       ((torch.rand(B_, H_, n, n, generator=g) >= 0.5).float().to(dev) * 2.0,) * 2 + (None,)):
        P, Pm = _hip.row_softmax_fwd(S, B_ * H_ * n, n, mask, d)
        dS = _hip.row_softmax_bwd(P, dPm, B_ * H_ * n, n, mask, d)
        s64 = S.double().requires_grad_(True)
        p64 = s64.softmax(-1)
        pm64 = p64 if m is None else p64 * m.double()
        (ds64,) = torch.autograd.grad(pm64, s64, dPm.double())
        assert rel_l2(P, p64) < KTOL and rel_l2(Pm, pm64) < KTOL
        den = float(ds64.norm()) if n > 1 else float((pm64.detach() * dPm.double()).norm())
        assert float((dS.double() - ds64).norm()) / (den or 1.0) < KTOL
        assert torch.equal(_hip.row_softmax_fwd(S.clone(), B_ * H_ * n, n, mask, d)[0], P)
        assert torch.equal(_hip.row_softmax_bwd(P, dPm.clone(), B_ * H_ * n, n, mask, d), dS)


def _no_dropout(mod):
    """The encoder layer forces dropout = 0.1 for 'softmax' whatever its argument says (reference model.py:65-66, mirrored):
    switch every nn.Dropout off, as the fixture generator does on the reference."""
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def _run_fixture(GT, dev, g, mode=None, seed=None):
    from galerkin_transformer import _hip
    torch.manual_seed(0)
    mod = build_module(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = _no_dropout(mod).to(dev).train()
    if mode is not None:
        GT.set_attention_dropout(mode)
        _hip.set_seed(seed)
    elif g.masks:
        GT.set_attention_dropout("replay")
        GT.push_attention_masks([m.to(dev) for m in g.masks])
    else:
        GT.set_attention_dropout("off")
    try:
        ins = {k: v.to(dev) for k, v in g.inputs.items()}
        for k in g.din:
            ins[k].requires_grad_(True)
        out = run_module(mod, g, ins)
        w = None
        if isinstance(out, tuple):
            out, w = out
        out.backward(g.cot.to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    grads = {k: p.grad for k, p in mod.named_parameters()}
    return out.detach(), {k: ins[k].grad for k in g.din}, grads, w


def _gate(name, errs, noise):
    print(name, "worst", max(errs.values()), {k: (f"{v:.1e}", f"{noise.get(k, 0.0):.1e}") for k, v in errs.items()
                                              if v > 0.5 * TOL})
    bad = {k: (v, max(TOL, 12.0 * noise.get(k, 0.0))) for k, v in errs.items()
           if k != "out" and not v < max(TOL, 12.0 * noise.get(k, 0.0))}
    assert errs["out"] < TOL, errs["out"]
    assert not bad, bad


@pytest.mark.parametrize("name", SOFTMAX_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("softmax/" + name)
    out, din, grads, w = _run_fixture(GT, gpu_device, g)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(din[k], g.din[k]) for k in g.din})
    for k in g.dparam:
        assert grads[k] is not None, k
    errs.update({"dW:" + k: v for k, v in grad_errors(grads, g.dparam, g.sd).items()})
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    noise = {"d" + k: rel_l2(di32[k], di64[k]) for k in di32}
    noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64, g.sd).items()})
    _gate(name, errs, noise)
    if name == "enc_softmax_weights":       # the materialised route returns softmax(S) .* mask, as the reference does
        attn = torch.from_numpy(np.load(os.path.join(GOLDEN, "softmax", name + ".npz"))["attn"])
        assert w is not None and w.shape == attn.shape
        assert rel_l2(w, attn) < TOL
    else:
        assert w is None


def test_routes_agree_and_draw_one_mask(GT, gpu_device):
    """The fused and the materialised route on the same inputs under the same 'reference'-mode descriptor: forward and all
    gradients at 1e-5; the returned weight is P .* m against float64 with m drawn by gt_dropout_apply."""
    from galerkin_transformer import _hip
    g = Golden("softmax/enc_softmax_weights")
    runs = {}
    for need_w in (True, False):
        g.meta["attn_weight"] = need_w
        runs[need_w] = _run_fixture(GT, gpu_device, g, mode="reference", seed=4242)
    g.meta["attn_weight"] = True
    (o1, di1, gr1, w), (o0, di0, gr0, w0) = runs[True], runs[False]
    assert w0 is None and w is not None
    assert rel_l2(o0, o1) < 1e-5 and rel_l2(di0["x"], di1["x"]) < 1e-5
    errs = grad_errors(gr0, gr1, g.sd)
    assert max(errs.values()) < 1e-5, errs
    plain = _run_fixture(GT, gpu_device, g)
    assert not torch.equal(o1, plain[0]) and rel_l2(w, plain[3]) > 0.5       # the mask was drawn at all
    # salts: set_seed rewinds the call-site counter to 1, the attention call takes the first salt
    _hip.set_seed(4242)
    m = _draw_mask_shape(_hip, gpu_device, w.shape, _hip.dropout_desc(0.5, 1, gpu_device))
    kept = m != 0
    assert abs(kept.float().mean().item() - 0.5) < 0.02
    assert torch.equal(w != 0, kept) or ((w != 0) ^ kept).float().mean().item() < 1e-6      # (P may underflow nowhere here)
    assert rel_l2(w, plain[3].double() * m.double()) < KTOL


def _draw_mask_shape(_hip, dev, shape, drop):
    return _hip.dropout_apply(torch.ones(*shape, device=dev), drop)


def test_unsupported_width_raises_before_any_launch(GT, gpu_device):
    from galerkin_transformer import _hip
    layer = GT.SimpleTransformerEncoderLayer(d_model=80, n_head=2, pos_dim=2, attention_type="softmax",
                                             layer_norm=False).to(gpu_device)          # DP = round4(40 + 2) = 44
    x, pos = torch.randn(1, 8, 80, device=gpu_device), torch.rand(1, 8, 2, device=gpu_device)
    with _hip.Profile() as prof:
        with pytest.raises(NotImplementedError, match="no kernel"):
            layer(x, pos)
    assert not prof.records
    with pytest.raises(NotImplementedError):
        layer.attn(x, x, x, pos=pos, mask=torch.ones(1, 8, 8, device=gpu_device))
    with pytest.raises(NotImplementedError):
        layer.attn(x, x, x, pos=pos, weight=torch.ones(1, 8, 1, device=gpu_device))


def test_nothing_leaks_between_kinds(GT, gpu_device):
    gal, sm = Golden("enc_galerkin_c2"), Golden("softmax/enc_softmax_c2")
    before = _run_fixture(GT, gpu_device, gal)
    _run_fixture(GT, gpu_device, sm)
    after = _run_fixture(GT, gpu_device, gal)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
    for k, v in before[2].items():
        assert torch.equal(v, after[2][k]), k


def test_graph_capture_replays_eager(GT, gpu_device):
    g = Golden("softmax/enc_softmax_c2")
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


def test_models_train_with_softmax(GT, gpu_device):
    from test_softmax_attention_cpu import LITE
    dev = gpu_device
    m = GT.FourierTransformer2DLite(attention_type="softmax", **LITE).to(dev).train()
    ng = 16
    out = m(torch.randn(2, ng, ng, 10, device=dev), None, torch.rand(2, ng * ng, 2, device=dev),
            torch.rand(2, ng, ng, 2, device=dev))["preds"]
    out.square().mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
