"""attention_type='official' on the device (-m gpu): the tail-free fused softmax kernels (gt_softmax_attn_nopos_*) through
the C ABI against float64, ops.multihead_attention's two routes against each other, _TransformerEncoderLayer,
TransformerEncoderWrapper and SimpleTransformer(attention_type='official') against the fixtures recorded from the reference
(tests/golden/official/), the layer's own attention dropout, and the behaviour around them (refused widths, nothing
leaking into the other kinds, graph capture, a training step).

Bars: the project's own, from test_softmax_attention_gpu.py.  Kernels: KTOL = 2e-6 relative L2 for O, L, dQ', dK', dV', D,
for the whole tile and again for its last 16-column fragment alone (where a leftover tail path would show); at n = 1 the
float64 dQ', dK' vanish and the uncancelled product is the denominator, as there.  Large range: max(KTOL, 12 x the float32
CPU restatement's own deviation from float64).  Routes: 1e-5.  Modules: TOL = 1e-5 for the output; dx and every parameter
gradient max(TOL, 12 x the float32 restatement's deviation from float64) per tensor (_gate's rule), the deviations computed
on the CPU in the test (test_official_cpu.py quotes them: none above 5e-7, so every bar is 1e-5)."""
import math
import os

import numpy as np
import pytest
import torch

from _official_ref import OFFICIAL_GOLDEN, SUB, build_module, ref_grads, run_module, run_ref
from _util import GOLDEN, Golden, TOL, rel_l2
from test_softmax_attention_gpu import B_, H_, KTOL, NS, _draw_mask, _draw_mask_shape, _formula, _gate, _heads
from test_softmax_attention_gpu import _run_fixture as _run_simple_fixture

pytestmark = pytest.mark.gpu

DPS = (16, 32, 48, 64, 96)


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


def _tiles(n, DP, seed, big=False):
    """Head tiles [B*n, h, DP], unit normal in EVERY column (no coordinate, no pad columns); big: entries shifted by +-80."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B_ * n, H_, DP, generator=g)
    if big:
        x = x + 80.0 * torch.sign(torch.randn(B_ * n, H_, DP, generator=g))
    return x


def _device_run(_hip, dev, Q, K, V, dO, n, DP, scale, mask, drop):
    assert _hip._softmax_entry(DP, "fwd") == "gt_softmax_attn_nopos_fwd"
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
        assert torch.isfinite(t).all(), k
    assert torch.isfinite(L).all() and torch.equal(L, L2)     # the tail-free forward writes L and its residual
    return {k: (_heads(t, n) if k in ("O", "dQ", "dK", "dV") else t).cpu() for k, t in got.items()}      # L, D: [B, h, n]


@pytest.mark.parametrize("mode", ("plain", "dropout", "mask"))
@pytest.mark.parametrize("DP", DPS)
def test_nopos_kernels_vs_float64(GT, gpu_device, DP, mode):
    from galerkin_transformer import _hip
    dev = gpu_device
    scale = 1.0 / math.sqrt(DP)
    _hip.set_seed(20261020)
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
            if n == 1 and k in ("dQ", "dK"):            # exact cancellation: the uncancelled product is the yardstick
                assert float(ref[k].norm()) < 1e-12 * float(ref[k + "_raw"].norm()) or float(ref[k + "_raw"].norm()) == 0
                den = ref[k + "_raw"]
            e = float((got[k].double() - ref[k]).norm()) / (float(den.norm()) or 1.0)
            print(f"DP {DP} {mode} n {n} {k}: {e:.2e}")
            assert e < KTOL, (DP, mode, n, k, e)
            if k in ("O", "dQ", "dK", "dV"):            # the last 16-column fragment on its own
                e = float((got[k][..., DP - 16:].double() - ref[k][..., DP - 16:]).norm()) / \
                    (float(den[..., DP - 16:].norm()) or 1.0)
                print(f"DP {DP} {mode} n {n} {k}[last 16]: {e:.2e}")
                assert e < KTOL, (DP, mode, n, k, "last fragment", e)


@pytest.mark.parametrize("DP", DPS)
def test_large_range(GT, gpu_device, DP):
    """Tile entries shifted by +-80: the scores overflow exp() without the running maximum."""
    from galerkin_transformer import _hip
    n, scale = 65, 1.0 / math.sqrt(DP)
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
    x = torch.zeros(64, 1, 112, device=gpu_device).data_ptr()
    s = torch.zeros(128, device=gpu_device).data_ptr()
    for DP in (20, 24, 80, 112):
        assert lib.gt_softmax_attn_nopos_fwd(x, x, x, x, s, 1, 64, 1, DP, 1.0, None, None, st) == -4
        assert lib.gt_softmax_attn_nopos_bwd_q(x, x, x, x, x, s, s, x, 1, 64, 1, DP, 1.0, None, None, st) == -4
        assert lib.gt_softmax_attn_nopos_bwd_kv(x, x, x, x, s, s, x, x, 1, 64, 1, DP, 1.0, None, None, st) == -4
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- modules
def _load(GT, dev, g, dropout=0.0):
    torch.manual_seed(0)
    mod = build_module(GT, g, dropout=dropout)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return mod.to(dev)


def _run(mod, dev, g):
    """Forward + backward of one fixture on the device: (out, {input: grad}, {param: grad}, w)."""
    ins = {k: v.to(dev) for k, v in g.inputs.items()}
    for k in g.din:
        ins[k].requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out, w = run_module(mod, g, ins)
    out.backward(g.cot.to(dev))
    torch.cuda.synchronize()
    return out.detach(), {k: ins[k].grad for k in g.din}, {k: p.grad for k, p in mod.named_parameters()}, w


def _noise(g, m=None):
    """Deviation of the float32 restatement from float64 per tensor, on the CPU."""
    _, di32, dp32 = ref_grads(g, torch.float32, m=m)
    _, di64, dp64 = ref_grads(g, torch.float64, m=m)
    noise = {"d" + k: rel_l2(di32[k], di64[k]) for k in di32}
    noise.update({"dW:" + k: rel_l2(dp32[k], dp64[k]) for k in dp32})
    return noise


def _errs(run, out, din, dparam):
    o, di, gr, _ = run
    errs = {"out": rel_l2(o, out)}
    errs.update({"d" + k: rel_l2(di[k], din[k]) for k in din})
    for k in dparam:
        assert gr[k] is not None, k
    errs.update({"dW:" + k: rel_l2(gr[k], dparam[k]) for k in dparam})
    return errs


@pytest.mark.parametrize("name", OFFICIAL_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden(SUB + name)
    run = _run(_load(GT, gpu_device, g).train(), gpu_device, g)        # (built with every dropout 0: training mode is exact)
    assert run[0].shape == g.out.shape
    _gate(name, _errs(run, g.out, g.din, g.dparam), _noise(g))
    w = run[3]
    if name == "enc_official_weights":       # the materialised route returns the head mean of P, as the reference does
        attn = torch.from_numpy(np.load(os.path.join(GOLDEN, "official", name + ".npz"))["attn"])
        assert w is not None and w.shape == attn.shape and not w.requires_grad
        assert rel_l2(w, attn) < TOL
    else:
        assert w is None


def _attention_dropout_only(mod, p):
    """The layer's dropout on P at rate p, every other dropout of the layer off."""
    mod.self_attn.dropout = p
    for m in (mod.dropout, mod.dropout1, mod.dropout2):
        m.p = 0.0
    return mod.train()


def test_routes_agree_under_one_descriptor(GT, gpu_device):
    """need_weights True (materialised) and False (fused) on the same inputs, the same dropout descriptor (p 0.3)."""
    from galerkin_transformer import _hip
    g = Golden(SUB + "enc_official_weights")
    runs = {}
    for need_w in (True, False):
        mod = _attention_dropout_only(_load(GT, gpu_device, g), 0.3)
        mod.attn_weight = need_w
        _hip.set_seed(4242)
        runs[need_w] = _run(mod, gpu_device, g)
    (o1, di1, gr1, w), (o0, di0, gr0, w0) = runs[True], runs[False]
    assert w0 is None and w is not None and w.shape == (2, 70, 70)
    assert rel_l2(o0, o1) < 1e-5 and rel_l2(di0["x"], di1["x"]) < 1e-5
    errs = {k: rel_l2(gr0[k], gr1[k]) for k in g.dparam}
    assert max(errs.values()) < 1e-5, errs
    assert rel_l2(o1, g.out) > 1e-3                           # the mask was drawn at all


def test_module_dropout(GT, gpu_device):
    """Training with p = 0.3 on P: output and dx against the float64 restatement with m drawn by gt_dropout_apply for the
    operator's salt; the keep rate; the set_attention_dropout switch does not act on this layer; eval reproduces the golden."""
    from galerkin_transformer import _hip
    dev = gpu_device
    g = Golden(SUB + "enc_official_weights")
    mod = _attention_dropout_only(_load(GT, dev, g), 0.3)
    results = {}
    try:
        for mode in ("off", "reference"):
            GT.set_attention_dropout(mode)
            _hip.set_seed(99)
            results[mode] = _run(mod, dev, g)
    finally:
        GT.set_attention_dropout("reference")
    a, b = results["off"], results["reference"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1]["x"], b[1]["x"]) and torch.equal(a[3], b[3])
    for k in g.dparam:
        assert torch.equal(a[2][k], b[2][k]), k
    # salts: set_seed rewinds the call-site counter to 1, the attention call takes the first salt
    _hip.set_seed(99)
    m = _draw_mask_shape(_hip, dev, (2, 4, 70, 70), _hip.dropout_desc(0.3, 1, dev)).cpu()
    vals = m.unique().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1.0 / 0.7) < 1e-6, vals
    keep, N = float((m != 0).float().mean()), m.numel()
    assert N == 39200 and abs(keep - 0.7) < 5.0 * math.sqrt(0.7 * 0.3 / N), keep
    o64, di64, dp64 = ref_grads(g, torch.float64, m=m)
    noise = _noise(g, m=m)
    _gate("enc_official_weights p 0.3", _errs(a, o64, di64, dp64), noise)
    mod.attn_weight = False                                   # ... and the fused route under the same descriptor
    _hip.set_seed(99)
    fused = _run(mod, dev, g)
    mod.attn_weight = True
    assert fused[3] is None
    _gate("enc_official_weights p 0.3 fused", _errs(fused, o64, di64, dp64), noise)
    sd64 = {k: v.double() for k, v in g.sd.items()}
    _, w64 = run_ref(g, sd64, {k: v.double() for k, v in g.inputs.items()}, return_attn=True, m=m)
    assert rel_l2(a[3], w64) < TOL                            # the returned weight is the head mean of Pm
    # eval: no dropout anywhere
    ev = _run(mod.eval(), dev, g)
    assert rel_l2(ev[0], g.out) < TOL and rel_l2(ev[1]["x"], g.din["x"]) < TOL


def test_unsupported_width_raises_before_any_launch(GT, gpu_device):
    from galerkin_transformer import _hip
    layer = GT._TransformerEncoderLayer(80, 2, dim_feedforward=64).to(gpu_device)          # d_k = 40
    x = torch.randn(1, 8, 80, device=gpu_device)
    with _hip.Profile() as prof:
        with pytest.raises(NotImplementedError, match="no kernel"):
            layer(x)
        with pytest.raises(AssertionError, match="was expecting embedding dimension"):
            layer(x, torch.rand(1, 8, 2, device=gpu_device))
    assert not prof.records


def test_nothing_leaks_between_kinds(GT, gpu_device):
    off = Golden(SUB + "enc_official_d64h4")
    for other in ("enc_galerkin_c2", "softmax/enc_softmax_c2"):
        g = Golden(other)
        before = _run_simple_fixture(GT, gpu_device, g)
        _run(_load(GT, gpu_device, off).train(), gpu_device, off)
        after = _run_simple_fixture(GT, gpu_device, g)
        assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
        for k, v in before[2].items():
            assert torch.equal(v, after[2][k]), (other, k)


def test_graph_capture_replays_eager(GT, gpu_device):
    g = Golden(SUB + "enc_official_d64h4")
    dev = gpu_device
    mod = _load(GT, dev, g).train()
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


def test_model_trains_one_step(GT, gpu_device):
    from galerkin_transformer import _hip
    dev = gpu_device
    g = Golden(SUB + "model_burgers_official_small")
    cfg = dict(g.meta["config"], encoder_dropout=0.1, ffn_dropout=0.1, dropout=0.05, layer_norm=True)
    torch.manual_seed(3)
    model = GT.SimpleTransformer(**cfg).to(dev).train()
    params = list(model.parameters())
    opt = GT.FlatClipAdam(params, lr=1e-3, max_norm=0.99, model=model)
    _hip.set_seed(7)
    before = [p.detach().clone() for p in params]
    out = model(torch.randn(2, 256, 1, device=dev), None, None)["preds"]
    assert out.shape == (2, 256, 1)
    out.square().mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in params)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, params))
