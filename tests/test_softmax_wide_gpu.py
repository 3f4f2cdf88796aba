"""attention_type='softmax' at the 64- and 96-wide heads (head tiles DP = 68, 100; gt_softmax_attn_wide_*) on the device
(-m gpu), with the helpers and the bars of test_softmax_attention_gpu.py: the fused kernels through the C ABI against float64,
the modules against the fixtures recorded from the reference (tests/golden/softmax_wide/), the two routes against each other,
graph capture, the shipped ex1 configuration, and the behaviour around them (widths the entry points refuse, nothing leaking
into the Galerkin path).

Bars.  Kernels: KTOL = 2e-6 relative L2 for O, L, dQ', dK', dV', D; at n = 1 the cancellation rule of
test_softmax_attention_gpu.py.  Large-range case: max(KTOL, 12 x the float32 CPU restatement's own deviation from float64 on
those inputs), computed in the test on the CPU.  Routes: 1e-5.  Modules: TOL = 1e-5 for the output, and
max(TOL, 12 x the float32 restatement's deviation from float64) per gradient (computed on the CPU, never from the device
run); gradients that vanish in exact arithmetic are measured absolutely (_linear_ref.grad_errors).  Deviations of the float32
restatement from float64 measured on the CPU (test_softmax_wide_cpu.py::test_restatement_fp64_envelope), output and largest
gradient per fixture:
    enc_softmax_w100 8.0e-08, 1.5e-06 (attn.linears.1.bias); _replay 7.9e-08, 1.3e-06; enc_softmax_w68 9.0e-08, 1.1e-06
    (attn.linears.1.bias); _replay 9.1e-08, 1.1e-06; enc_softmax_w68_weights 9.0e-08, 1.1e-06; model_burgers_softmax_ex1
    1.1e-06, 3.1e-06 (encoder_layers.1.attn.norm_Q.0.bias, the only tensor above 2e-6)."""
import math
import os

import numpy as np
import pytest
import torch

from _softmax_ref import grad_errors, ref_grads
from _softmax_wide_ref import SUB, WIDE_GOLDEN, wide_golden
from _util import GOLDEN, Golden, TOL, rel_l2
from test_modules_gpu import build_module
from test_softmax_attention_gpu import (GT, KTOL, NS, B_, H_, _device_run, _draw_mask, _formula, _gate,  # noqa: F401
                                        _no_dropout, _run_fixture, _tiles)

pytestmark = pytest.mark.gpu

WIDE_DP = (68, 100)


@pytest.mark.parametrize("mode", ("plain", "dropout", "mask"))
@pytest.mark.parametrize("DP", WIDE_DP)
def test_fused_kernels_vs_float64(GT, gpu_device, DP, mode):
    """n = 1, 63, 64, 65, 129, 257: one partial stream tile, exactly one, the tile boundary, a partial 128-owner block, more
    than one block.  _device_run also asserts that a second call is bit-identical and the pad columns are exactly zero."""
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
            if n == 1 and k in ("dQ", "dK"):            # exact cancellation: the uncancelled product
                assert float(ref[k].norm()) < 1e-12 * float(ref[k + "_raw"].norm()) or float(ref[k + "_raw"].norm()) == 0
                den = ref[k + "_raw"]
            e = float((got[k].double() - ref[k]).norm()) / (float(den.norm()) or 1.0)
            print(f"DP {DP} {mode} n {n} {k}: {e:.2e}")
            assert e < KTOL, (DP, mode, n, k, e)


@pytest.mark.parametrize("DP", WIDE_DP)
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


def test_entry_points_split_the_widths(GT, gpu_device):
    """The wide entry points answer GT_ENOTSUP (-4) for the narrow widths and for 84 / 116; the narrow forward still does for 68."""
    from galerkin_transformer import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    x = torch.zeros(64, 1, 116, device=gpu_device)
    s = torch.zeros(128, device=gpu_device)
    p = x.data_ptr()
    for DP in (20, 52, 84, 116):
        assert lib.gt_softmax_attn_wide_fwd(p, p, p, p, s.data_ptr(), 1, 64, 1, DP, 1.0, None, None, st) == -4
        assert lib.gt_softmax_attn_wide_bwd_q(p, p, p, p, p, s.data_ptr(), s.data_ptr(), p, 1, 64, 1, DP, 1.0, None, None,
                                              st) == -4
        assert lib.gt_softmax_attn_wide_bwd_kv(p, p, p, p, s.data_ptr(), s.data_ptr(), p, p, 1, 64, 1, DP, 1.0, None, None,
                                               st) == -4
    assert lib.gt_softmax_attn_fwd(p, p, p, p, s.data_ptr(), 1, 64, 1, 68, 1.0, None, None, st) == -4
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", WIDE_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = wide_golden(name)
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
    if name == "enc_softmax_w68_weights":   # need_weights=True: gt_gemm + gt_row_softmax_*, returns softmax(S) .* mask
        attn = torch.from_numpy(np.load(os.path.join(GOLDEN, SUB + name + ".npz"))["attn"])
        assert w is not None and w.shape == attn.shape
        assert rel_l2(w, attn) < TOL
    else:
        assert w is None


def test_weights_route_runs_at_100(GT, gpu_device):
    """need_weights=True at DP = 100: the materialised route on the w100 fixture's layer gives the fixture's output and
    gradients at the module bar, and a row-stochastic weight."""
    g = wide_golden("enc_softmax_w100")
    g.meta["attn_weight"] = True
    out, din, grads, w = _run_fixture(GT, gpu_device, g)
    assert w is not None and w.shape == (2, 1, 65, 65)
    assert torch.allclose(w.sum(-1), torch.ones(2, 1, 65, device=w.device), atol=1e-5)
    assert rel_l2(out, g.out) < TOL and rel_l2(din["x"], g.din["x"]) < TOL


def test_routes_agree_under_one_dropout_descriptor(GT, gpu_device):
    """The fused (gt_softmax_attn_wide_*) and the materialised route on the same inputs under the same 'reference'-mode
    descriptor: forward and all gradients at 1e-5."""
    g = wide_golden("enc_softmax_w68_weights")
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


def test_graph_capture_replays_eager(GT, gpu_device):
    """One DP = 100 layer step (forward + all gradients) captured and replayed: bit-identical to eager."""
    g = wide_golden("enc_softmax_w100")
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


def test_shipped_ex1_trains_a_step_on_the_fused_route(GT, gpu_device):
    """SimpleTransformer(**config.yml: ex1_burgers) with attention_type='softmax', n = 128: forward + MSE + backward; every
    gradient is there and finite; the wide fused kernels ran in every layer and no n x n product or row softmax did."""
    import yaml
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "galerkin-transformer_amd", "config.yml")) as f:
        cfg = dict(yaml.full_load(f)["ex1_burgers"], attention_type="softmax")
    dev, n = gpu_device, 128
    torch.manual_seed(3)
    m = GT.SimpleTransformer(**cfg).to(dev).train()
    node = torch.randn(2, n, 1, device=dev)
    pos = torch.linspace(0, 1, n, device=dev)[None, :, None].repeat(2, 1, 1)
    target = torch.randn(2, n, 1, device=dev)
    with _hip.Profile() as prof:
        out = m(node, None, pos)["preds"]
        (out - target).square().mean().backward()
        torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    keys = [r[0] for r in prof.records]
    layers = cfg["num_encoder_layers"]
    for sym in ("gt_softmax_attn_wide_fwd", "gt_softmax_attn_wide_bwd_q", "gt_softmax_attn_wide_bwd_kv"):
        assert keys.count(sym) == layers, (sym, keys.count(sym))
    assert not [k for k in keys if k.startswith("gt_row_softmax") or k.startswith("gt_softmax_attn_") and "_wide_" not in k]
    nn_products = [r for r in prof.records if r[6] is not None and len(r[6]) >= 2 and r[6][0] == n and r[6][1] == n]
    assert not nn_products, [(r[0], r[6]) for r in nn_products]


def test_unsupported_width_still_raises_before_any_launch(GT, gpu_device):
    from galerkin_transformer import _hip
    layer = GT.SimpleTransformerEncoderLayer(d_model=80, n_head=2, pos_dim=2, attention_type="softmax",
                                             layer_norm=False).to(gpu_device)          # DP = round4(40 + 2) = 44
    x, pos = torch.randn(1, 8, 80, device=gpu_device), torch.rand(1, 8, 2, device=gpu_device)
    with _hip.Profile() as prof:
        with pytest.raises(NotImplementedError, match="no kernel") as e:
            layer(x, pos)
    assert not prof.records
    assert str(_hip.SOFTMAX_DP) in str(e.value) and str(_hip.SOFTMAX_DP_WIDE) in str(e.value)


def test_nothing_leaks_between_kinds(GT, gpu_device):
    gal = Golden("enc_galerkin_c2")
    before = _run_fixture(GT, gpu_device, gal)
    _run_fixture(GT, gpu_device, wide_golden("enc_softmax_w100"))
    _run_fixture(GT, gpu_device, wide_golden("enc_softmax_w68"))
    after = _run_fixture(GT, gpu_device, gal)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
    for k, v in before[2].items():
        assert torch.equal(v, after[2][k]), k
