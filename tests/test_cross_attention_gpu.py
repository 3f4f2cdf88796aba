"""Cross-attention on the device (-m gpu): the single-stream head-tile kernels through the C ABI against float64, the modules
against the fixtures recorded from the reference (tests/golden/cross/), the cross route against the self-attention route,
aliased inputs, and the behaviour around them (nothing leaking into the self-attention path, graph capture).

Bars.  Kernels: KTOL = 2e-6 relative L2 (the kernel suites' bar) for the tiles, the statistics, dX, dgamma and dbeta; the
coordinate and pad columns and everything of dX outside the value columns are exact.  Modules: TOL = 1e-5 for the output, or
max(TOL, 12 x the float32 restatement's deviation from float64) per tensor for the returned weight, each input gradient and
every parameter gradient (the rule of test_fullsize_models_gpu._gate, computed on the CPU, never from the device run).
Deviations of the float32 restatement from float64 measured on the CPU
(test_cross_attention_cpu.py::test_restatement_fp64_envelope), largest per fixture:
    x_galerkin_nopos 3.8e-07 (norm_V.2.bias), _replay 6.5e-07, x_galerkin_nopos_wide 6.6e-07, x_linear_nopos 7.2e-07,
    x_galerkin_inst_nopos 1.7e-06 (norm_K.3.bias), x_galerkin_pos 4.3e-07, x_linear_pos 7.3e-07 (linears.1.bias),
    x_fourier_pos 5.0e-07, _replay 4.5e-07, x_softmax_pos 1.0e-06 (linears.1.bias), x_galerkin_nonorm 4.0e-07 (dmem);
    none above 2e-6.
Gradients that vanish in exact arithmetic (the bias in front of K' under a token or key softmax, the K and V projection biases
under the token-axis norm: _cross_ref.param_errors) are measured absolutely, against the size of the sibling weight's
gradient, at the same bars.  Routes and aliasing: 1e-5."""
import pytest
import torch

from _cross_ref import CROSS_GOLDEN, all_errors, golden_weight, param_errors, ref_grads
from _util import Golden, TOL, rel_l2

pytestmark = pytest.mark.gpu

KTOL = 2e-6
TS = (1, 15, 16, 17, 140)
SHAPES = ((4, 16, 2), (2, 48, 1), (1, 96, 1), (3, 20, 0))


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


# ------------------------------------------------------------------------------------------ kernels
def _headtile_f64(X, pos, gamma, beta, d_out, h, dk, p, eps):
    """float64 on the CPU: (tiles, stats, dX, dgamma, dbeta) of out = [pos | LN(x) gamma + beta | 0] per head."""
    T = X.shape[0]
    x = X.double().reshape(T, h, dk).requires_grad_(True)
    DP = (dk + p + 3) & ~3
    y, stats = x, None
    gm = bt = None
    if gamma is not None:
        gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        mu = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
        y = (x - mu) * rstd * gm[None] + bt[None]
        stats = torch.cat([mu, rstd], -1).detach()
    pp = torch.zeros(T, h, 0, dtype=torch.float64) if p == 0 else pos.double()[:, None].expand(T, h, p)
    out = torch.cat([pp, y, torch.zeros(T, h, DP - dk - p, dtype=torch.float64)], -1)
    grads = torch.autograd.grad(out, [x] + ([gm, bt] if gamma is not None else []), d_out.double())
    return out.detach(), stats, grads[0].reshape(T, h * dk), (grads[1] if gamma is not None else None), \
        (grads[2] if gamma is not None else None)


@pytest.mark.parametrize("normed", (True, False))
@pytest.mark.parametrize("h,dk,p", SHAPES)
def test_headtile_kernels_vs_float64(GT, gpu_device, h, dk, p, normed):
    from galerkin_transformer import _hip
    dev, hd, DP, eps = gpu_device, h * dk, (dk + p + 3) & ~3, 1e-5
    gen = torch.Generator().manual_seed(1000 * h + 10 * dk + p)
    # (leading dimension, first column): dense; the second column block of a packed [T, 2 h dk] product; an odd row pitch
    for T in TS:
        for ld, c0 in ((hd, 0), (2 * hd, hd), (hd + 3, 0)):
            buf = torch.randn(T, ld, generator=gen) * 2.0 + 0.5
            pos = torch.rand(T, p, generator=gen) if p else None
            gamma = (1.0 + 0.3 * torch.randn(h, dk, generator=gen)) if normed else None
            beta = 0.3 * torch.randn(h, dk, generator=gen) if normed else None
            d_out = torch.randn(T, h, DP, generator=gen)          # (the coordinate and pad columns carry values to ignore)
            ref = _headtile_f64(buf[:, c0:c0 + hd], pos, gamma, beta, d_out, h, dk, p, eps)
            bd, dd = buf.to(dev), d_out.to(dev)
            posd, gd, btd = (None if t is None else t.to(dev) for t in (pos, gamma, beta))
            X = bd[:, c0:]
            runs = []
            for _ in range(2):
                tiles, stats = _hip.headtile_fwd(X, ld, posd, gd, btd, T, h, dk, p, eps)
                dbuf = torch.full((T, ld), 7.25, device=dev)
                dg = torch.empty(h, dk, device=dev) if normed else None
                db = torch.empty(h, dk, device=dev) if normed else None
                _hip.headtile_bwd(dd, X if normed else None, ld, gd, stats, T, h, dk, p, dbuf[:, c0:], ld, dg, db)
                torch.cuda.synchronize()
                runs.append((tiles, stats, dbuf, dg, db))
            for a, b in zip(*runs):
                assert (a is None and b is None) or torch.equal(a, b), "second call differs"
            tiles, stats, dbuf, dg, db = (None if t is None else t.cpu() for t in runs[0])
            tag = (T, ld, c0)
            assert torch.equal(tiles[..., dk + p:], torch.zeros(T, h, DP - dk - p)), ("pad columns", tag)
            if p:
                assert torch.equal(tiles[..., :p], pos[:, None].expand(T, h, p)), ("coordinate columns", tag)
            outside = torch.ones(ld, dtype=torch.bool)
            outside[c0:c0 + hd] = False
            assert (dbuf[:, outside] == 7.25).all(), ("dX outside the value columns", tag)
            errs = {"tiles": rel_l2(tiles, ref[0]), "dX": rel_l2(dbuf[:, c0:c0 + hd], ref[2])}
            if normed:
                errs.update(stats=rel_l2(stats, ref[1]), dgamma=rel_l2(dg, ref[3]), dbeta=rel_l2(db, ref[4]))
            else:
                assert stats is None
                assert torch.equal(tiles[..., p:p + dk].reshape(T, hd), buf[:, c0:c0 + hd]), ("plain copy", tag)
                assert torch.equal(dbuf[:, c0:c0 + hd], d_out[..., p:p + dk].reshape(T, hd)), ("plain scatter", tag)
            print(f"h {h} dk {dk} p {p} normed {normed} T {T} ld {ld} c0 {c0}:", {k: f"{v:.1e}" for k, v in errs.items()})
            bad = {k: v for k, v in errs.items() if not v < KTOL}
            assert not bad, (tag, bad)


def test_headtile_refuses_what_it_does_not_take(GT, gpu_device):
    from galerkin_transformer import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    x = torch.zeros(4, 2048, device=gpu_device)
    o = torch.zeros(4, 2048 + 64, device=gpu_device)
    # ldx below h*dk: GT_EINVAL; dk above 256: GT_ENOTSUP; gamma without beta / stats: GT_EINVAL
    assert lib.gt_headtile_fwd(x.data_ptr(), 16, None, None, None, 4, 2, 16, 0, 1e-5, o.data_ptr(), None, st) == -1
    assert lib.gt_headtile_fwd(x.data_ptr(), 2048, None, None, None, 4, 1, 260, 0, 1e-5, o.data_ptr(), None, st) == -4
    assert lib.gt_headtile_fwd(x.data_ptr(), 32, None, x.data_ptr(), None, 4, 2, 16, 0, 1e-5, o.data_ptr(), None, st) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ modules
def _module(GT, g, dev):
    m = g.meta
    torch.manual_seed(0)
    mod = GT.SimpleAttention(m["n_head"], m["d_model"], pos_dim=m["pos_dim"], attention_type=m["attention_type"],
                             dropout=0.0, norm=m["norm"], norm_type=m["norm_type"], eps=m["eps"])
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return mod.to(dev).train()


def _run(GT, dev, g, call=None, masks=True):
    """The module on the fixture's weights and inputs.  ``call(mod, ins)`` -> (out, weight); default: the fixture's form.
    Returns (out, weight, {input: grad}, {param: grad})."""
    mod = _module(GT, g, dev)
    if masks and g.masks:
        GT.set_attention_dropout("replay")
        GT.push_attention_masks([m.to(dev) for m in g.masks])
    else:
        GT.set_attention_dropout("off")
    try:
        ins = {k: v.to(dev) for k, v in g.inputs.items()}
        for k in g.din:
            ins[k].requires_grad_(True)
        if call is None:
            out, w = mod(*(ins[k] for k in g.meta["form"]), pos=ins.get("pos"))
        else:
            out, w = call(mod, ins)
        out.backward(g.cot.to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    return out.detach(), w, {k: v.grad for k, v in ins.items() if v.requires_grad}, \
        {k: p.grad for k, p in mod.named_parameters()}


def _gate(name, errs, noise):
    print(name, "worst", max(errs.values()), {k: (f"{v:.1e}", f"{noise.get(k, 0.0):.1e}") for k, v in errs.items()
                                              if v > 0.5 * TOL})
    bad = {k: (v, max(TOL, 12.0 * noise.get(k, 0.0))) for k, v in errs.items()
           if k != "out" and not v < max(TOL, 12.0 * noise.get(k, 0.0))}
    assert errs["out"] < TOL, errs["out"]
    assert not bad, bad


@pytest.mark.parametrize("name", CROSS_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("cross/" + name)
    out, w, din, grads = _run(GT, gpu_device, g)
    gw = golden_weight(name)
    assert out.shape == g.out.shape and w is not None and w.shape == gw.shape
    assert set(din) == set(g.din)
    for k in g.dparam:
        assert grads[k] is not None, k
    errs = all_errors(out, w, din, grads, g.out, gw, g.din, g.dparam, g)
    noise = all_errors(*ref_grads(g, torch.float32), *ref_grads(g, torch.float64), g)
    _gate(name, errs, noise)


@pytest.mark.parametrize("name", ("x_galerkin_pos", "x_linear_pos", "x_fourier_pos", "x_softmax_pos"))
def test_cross_route_agrees_with_self_route(GT, gpu_device, name):
    """forward(x, x.clone(), x.clone(), pos) against forward(x, x, x, pos): the same numbers from two projection stages."""
    g = Golden("cross/" + name)
    seen = {}

    def cross(mod, ins):
        seen["k"], seen["v"] = (ins["q"].detach().clone().requires_grad_(True) for _ in range(2))
        return mod(ins["q"], seen["k"], seen["v"], pos=ins["pos"])

    oc, wc, dc, gc = _run(GT, gpu_device, g, cross, masks=False)
    os_, ws, ds, gs = _run(GT, gpu_device, g, lambda mod, ins: mod(ins["q"], ins["q"], ins["q"], pos=ins["pos"]), masks=False)
    dx = dc["q"] + seen["k"].grad + seen["v"].grad
    errs = {"out": rel_l2(oc, os_), "attn": rel_l2(wc, ws), "dx": rel_l2(dx, ds["q"])}
    errs.update(param_errors(gc, gs, g))
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.parametrize("name", ("x_galerkin_nopos", "x_linear_nopos", "x_softmax_pos"))
def test_aliased_memory_sums_its_gradients(GT, gpu_device, name):
    """forward(q, mem, mem) equals forward(q, mem, mem.clone()); in the first form mem.grad holds the sum."""
    g = Golden("cross/" + name)
    seen = {}

    def split(mod, ins):
        seen["v"] = ins["mem"].detach().clone().requires_grad_(True)
        return mod(ins["q"], ins["mem"], seen["v"], pos=ins.get("pos"))

    o1, w1, d1, g1 = _run(GT, gpu_device, g, masks=False)
    o2, w2, d2, g2 = _run(GT, gpu_device, g, split, masks=False)
    errs = {"out": rel_l2(o2, o1), "attn": rel_l2(w2, w1), "dq": rel_l2(d2["q"], d1["q"]),
            "dmem": rel_l2(d2["mem"] + seen["v"].grad, d1["mem"])}
    errs.update(param_errors(g2, g1, g))
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs
    assert rel_l2(d2["mem"], d1["mem"]) > 1e-2          # (the K part alone is not the sum)


def test_residual_and_sign_on_the_query_rows(GT, gpu_device):
    """fused_forward_cross(residual=q, sign=-1): out = q - attention, d(query) = cotangent - d(query) of the plain call."""
    g = Golden("cross/x_galerkin_nopos_wide")
    o0, _, d0, g0 = _run(GT, gpu_device, g)
    o1, _, d1, g1 = _run(GT, gpu_device, g, lambda mod, ins: mod.fused_forward_cross(ins["q"], ins["mem"], ins["mem"], None,
                                                                                 residual=ins["q"], sign=-1.0))
    dev = gpu_device
    assert rel_l2(o1, g.inputs["q"].to(dev) - o0) < 1e-5
    assert rel_l2(d1["q"], g.cot.to(dev) - d0["q"]) < 1e-5 and rel_l2(d1["mem"], -d0["mem"]) < 1e-5
    for k, v in g0.items():
        assert rel_l2(g1[k], -v) < 1e-5, k


def test_nothing_leaks_into_self_attention(GT, gpu_device):
    from test_softmax_attention_gpu import _run_fixture
    gal = Golden("enc_galerkin_c2")
    before = _run_fixture(GT, gpu_device, gal)
    for name in ("x_galerkin_nopos_replay", "x_galerkin_pos", "x_linear_pos"):
        _run(GT, gpu_device, Golden("cross/" + name))
    after = _run_fixture(GT, gpu_device, gal)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
    for k, v in before[2].items():
        assert torch.equal(v, after[2][k]), k


def test_graph_capture_replays_eager(GT, gpu_device):
    g = Golden("cross/x_galerkin_nopos")
    dev = gpu_device
    mod = _module(GT, g, dev)
    q, mem = (g.inputs[k].to(dev).requires_grad_(True) for k in ("q", "mem"))
    cot = g.cot.to(dev)
    params = list(mod.parameters())
    GT.set_attention_dropout("off")
    try:
        def step():
            return torch.autograd.grad(mod(q, mem, mem)[0], [q, mem] + params, cot)
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
