"""GPU tests of the random-feature attention baselines ('rfa' / 'favor'): the four gt_rfattn_* kernels through the binding
against the float64 restatement tests/_rfa_ref.py, the modules against the fixtures recorded from the reference
(tests/golden/rfa/), the redraw of omega, and the memory of the fused operator against a torch composition.

Bars.  Kernels: KTOL = 2e-6 relative L2 (the kernel suites' bar) for KVa (ksum column included), out, den, dQ, dK, dV, dKVa.
At n = 1 the attention returns v whatever q and k are (phi(q) . phi(k) cancels against den up to eps), so the float64 dQ and
dK are ~1e-6 of their two cancelling halves: there the absolute error is taken relative to the size of the half without
the cancellation (the gradient through phi(q) KV alone, den held constant; for dK through KV alone, ksum held constant), at
the same bar -- the rule test_softmax_attention_gpu.py states for its n = 1 case.  Large-argument case:
max(KTOL, 12 x the float32 CPU restatement's own deviation from float64 on those inputs), computed here on the CPU.
Modules: max(TOL, 12 x the fixture's recorded float32 noise) per tensor, TOL = 1e-5.
"""
import math

import pytest
import torch

from _rfa_ref import FIXTURES, RfaGolden, core, core_grads, kva, phi
from _util import TOL, rel_l2

pytestmark = pytest.mark.gpu

KTOL = 2e-6
B_ = 2
KINDS = ("rfa", "favor")


@pytest.fixture(scope="module")
def _hip(gpu_device):
    import galerkin_transformer._hip as H
    H.lib()
    return H


def _two_slab_n(H):
    n = 1
    while H.rfattn_slabs(n) < 2:
        n += 1
    return n


def _draw(n, d, seed, qk_scale=0.3):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B_ * n, 3 * d, generator=g)
    qkv[:, :2 * d] *= qk_scale
    omega = torch.randn(d, d // 2, generator=g)
    dout = torch.randn(B_ * n, d, generator=g)
    return qkv, omega, dout


def _split(qkv, n, d, dtype):
    return tuple(qkv[:, i * d:(i + 1) * d].reshape(B_, n, d).to(dtype) for i in range(3))


def _device_run(H, dev, qkv, omega, dout, n, d, kind, eps=1e-6):
    """All four kernels on poisoned buffers with guard rows behind the last sample.  Returns the outputs on the CPU."""
    nan = float("nan")
    T, G = B_ * n, 16
    qkv_d, om_d, do_d = qkv.to(dev), omega.to(dev), dout.to(dev)
    Q, K, V = qkv_d[:, :d], qkv_d[:, d:2 * d], qkv_d[:, 2 * d:]
    KVa = torch.full((B_, d, d + 4), nan, device=dev)
    H.rfattn_kv(K, V, 3 * d, om_d, B_, n, d, kind, KVa=KVa)
    out = torch.full((T + G, d), nan, device=dev)
    den = torch.full((T + G,), nan, device=dev)
    H.rfattn_q(Q, 3 * d, om_d, KVa, B_, n, d, kind, eps, out=out, den=den)
    dqkv = torch.full((T + G, 3 * d), nan, device=dev)
    dKVa = torch.full((B_, d, d + 4), nan, device=dev)
    H.rfattn_bwd(Q, K, V, 3 * d, om_d, KVa, do_d, out, den, dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:], 3 * d, B_, n, d,
                 kind, dKVa=dKVa)
    torch.cuda.synchronize()
    # rows beyond the last token were never written; everything else was
    assert torch.isnan(out[T:]).all() and torch.isnan(den[T:]).all() and torch.isnan(dqkv[T:]).all()
    res = dict(KVa=KVa, out=out[:T], den=den[:T], dQ=dqkv[:T, :d], dK=dqkv[:T, d:2 * d], dV=dqkv[:T, 2 * d:], dKVa=dKVa)
    res = {k: v.cpu() for k, v in res.items()}
    for k, v in res.items():
        assert torch.isfinite(v).all(), k
    # pad columns: written, as exact zeros
    assert (res["KVa"][:, :, d + 1:] == 0).all() and (res["dKVa"][:, :, d + 1:] == 0).all()
    return res


def _reference(qkv, omega, dout, n, d, kind, eps=1e-6):
    q, k, v = _split(qkv, n, d, torch.float64)
    om, do = omega.double(), dout.reshape(B_, n, d).double()
    out, den, M = core(q, k, v, om, kind, eps)
    dq, dk, dv, dM = core_grads(q, k, v, om, kind, do, eps)
    ref = dict(KVa=M, out=out.reshape(-1, d), den=den.reshape(-1), dQ=dq.reshape(-1, d), dK=dk.reshape(-1, d),
               dV=dv.reshape(-1, d), dKVa=dM)
    # the halves that cancel at n = 1 (module docstring)
    qq, kk = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    w = do / den.unsqueeze(-1)
    ref["dQ_raw"] = torch.autograd.grad((phi(qq, om, kind) @ M[:, :, :d] * w).sum(), qq)[0].reshape(-1, d)
    pq = phi(q, om, kind)
    ref["dK_raw"] = torch.autograd.grad(((pq @ (phi(kk, om, kind).transpose(1, 2) @ v)) * w).sum(), kk)[0].reshape(-1, d)
    assert float(den.abs().min()) >= 0.1 * float(den.abs().mean()), "ill-conditioned draw"
    return ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [32, 64, 96])
def test_kernels_against_formula(_hip, gpu_device, d, kind):
    two = _two_slab_n(_hip)
    assert _hip.rfattn_slabs(two - 1) == 1 and _hip.rfattn_slabs(two) == 2
    for n in (1, 63, 64, 70, two):
        qkv, omega, dout = _draw(n, d, 1000 * d + n)
        got = _device_run(_hip, gpu_device, qkv, omega, dout, n, d, kind)
        ref = _reference(qkv, omega, dout, n, d, kind)
        for k in ("KVa", "out", "den", "dQ", "dK", "dV", "dKVa"):
            scale = ref[k]
            if n == 1 and k in ("dQ", "dK"):
                assert float(ref[k].norm()) < 1e-4 * float(ref[k + "_raw"].norm())
                scale = ref[k + "_raw"]
            e = float((got[k].double() - ref[k]).norm()) / float(scale.norm())
            print(f"d {d} {kind} n {n} {k}: {e:.2e}")
            assert e < KTOL, (d, kind, n, k, e)
        again = _device_run(_hip, gpu_device, qkv, omega, dout, n, d, kind)
        for k in got:
            assert torch.equal(got[k], again[k]), (d, kind, n, k)


@pytest.mark.parametrize("kind", KINDS)
def test_large_arguments(_hip, gpu_device, kind):
    """|u| up to 50: gt_rfattn_kv with unit value rows at n = 1 (KVa is phi(k) itself) and at n = 70."""
    d = 96
    for n in (1, 70):
        qkv, omega, _ = _draw(n, d, 77 + n)
        # key rows along columns of omega (a random direction of that length would put favor's offset c = |s k|^2 / 2 near
        # 200 and every feature below the float32 range), 10 % noise, then scaled so that max |u| is 50
        g = torch.Generator().manual_seed(n)
        cols = torch.arange(B_ * n) % (d // 2)
        k = omega.t()[cols] * (1.0 + 0.1 * torch.randn(B_ * n, d, generator=g))
        umax = float((k.double() * d ** -0.25 @ omega.double()).abs().max())
        qkv[:, d:2 * d] = k * (50.0 / umax)
        qkv[:, 2 * d:] = 1.0
        _, k, v = _split(qkv, n, d, torch.float64)
        assert abs(float((k * d ** -0.25 @ omega.double()).abs().max()) - 50.0) < 1e-3
        ref = kva(k, v, omega.double(), kind)
        r32 = kva(k.float(), v.float(), omega, kind)
        assert rel_l2(r32, ref) < 1e-4                      # the case is inside the float32 range
        bound = max(KTOL, 12.0 * rel_l2(r32, ref))
        qkv_d = qkv.to(gpu_device)
        got = _hip.rfattn_kv(qkv_d[:, d:2 * d], qkv_d[:, 2 * d:], 3 * d, omega.to(gpu_device), B_, n, d, kind)
        e = rel_l2(got, ref)
        print(f"large arguments {kind} n {n}: {e:.2e} (bound {bound:.2e})")
        assert e < bound, (kind, n, e, bound)
        if n == 1:      # every column < d is phi(k), and so is the ksum column
            assert rel_l2(got[:, :, d], phi(k, omega.double(), kind)[:, 0]) < bound


# ------------------------------------------------------------------------------------------------- modules
def _build(g, dev):
    import galerkin_transformer as gt
    m, what = g.meta, g.meta["what"]
    if what == "attn":
        mod = gt.RandomFourierAttention(m["d_model"], 1, pos_dim=m["pos_dim"], eps=m["eps"], attention_type=g.kind)
        run = lambda x, pos: mod(x, x, x, pos=pos)
    elif what == "layer":
        mod = gt.RandomFeatureEncoderLayer(d_model=m["d_model"], n_head=1, dim_feedforward=m["dim_feedforward"],
                                           attention_type=g.kind, dropout=0.0, ffn_dropout=0.0)
        run = lambda x, pos: mod(x, pos)
    else:
        mod = gt.RandomFeatureTransformer(**m["config"])
        run = lambda x, pos: mod(x, None, pos)["preds"]
    mod.load_state_dict(g.sd, strict=True)
    mod = mod.to(dev).train()
    for sub in mod.modules():
        if isinstance(sub, gt.RandomFourierAttention):
            sub.redraw = False
    return mod, run


@pytest.mark.parametrize("name", FIXTURES)
def test_modules_against_reference(gpu_device, name):
    g = RfaGolden(name)
    mod, run = _build(g, gpu_device)
    xname = "node" if g.meta["what"] == "model" else "x"
    x = g.inputs[xname].to(gpu_device).requires_grad_(True)
    out = run(x, g.inputs["pos"].to(gpu_device))
    out.backward(g.cot.float().to(gpu_device))
    errs = {"out": rel_l2(out, g.out), "d" + xname: rel_l2(x.grad, g.din[xname])}
    for k, p in mod.named_parameters():
        errs[k] = rel_l2(p.grad, g.dparam[k])
    assert set(errs) == set(g.noise)
    bad = {}
    for k, e in errs.items():
        bound = max(TOL, 12.0 * g.noise[k])
        print(f"{name} {k}: {e:.2e} (bound {bound:.2e})")
        if not e < bound:
            bad[k] = (e, bound)
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_redraw(gpu_device, kind):
    import galerkin_transformer as gt
    from galerkin_transformer import ops
    torch.manual_seed(5)
    d, n = 32, 70
    # projections at unit gain: with the shipped 1e-2 init u is ~1e-2 and the output hardly depends on omega
    mod = gt.RandomFourierAttention(d, 1, attention_type=kind, xavier_init=1.0).to(gpu_device).train()
    x = 0.3 * torch.randn(B_, n, d, device=gpu_device)
    pos = torch.rand(B_, n, 1, device=gpu_device)
    assert mod.redraw and float(mod.feature_map.omega.abs().max()) == 0.0
    y1 = mod(x, x, x, pos=pos)
    om1 = mod.feature_map.omega.clone()
    y2 = mod(x, x, x, pos=pos)
    om2 = mod.feature_map.omega.clone()
    assert om1.shape == (d, d // 2) and float(om1.abs().max()) > 0 and not torch.equal(om1, om2)
    if kind == "favor":     # block-orthogonal: the columns of one block are orthogonal
        gram = om2.t().double() @ om2.double()
        assert float((gram - torch.diag(torch.diag(gram))).abs().max()) < 1e-4 * float(torch.diag(gram).max())
    q, k, v = mod.query_projection, mod.key_projection, mod.value_projection
    direct = ops.random_feature_attention(x, pos, torch.cat([q.weight, k.weight, v.weight]),
                                          torch.cat([q.bias, k.bias, v.bias]), om2, mod.out_projection.weight,
                                          mod.out_projection.bias, kind=kind, eps=mod.eps)
    assert rel_l2(y2, direct) < 1e-6 and rel_l2(y1, direct) > 1e-4
    mod.feature_map.deterministic_eval = True
    mod.eval()
    y3 = mod(x, x, x, pos=pos)
    assert torch.equal(mod.feature_map.omega, om2) and rel_l2(y3, direct) < 1e-6
    mod.train()
    mod.redraw = False
    mod(x, x, x, pos=pos)
    assert torch.equal(mod.feature_map.omega, om2)


# ------------------------------------------------------------------------------------------------- memory
def _torch_composition(x, pos, wqkv, bqkv, omega, wout, bout, kind, eps):
    d = x.shape[-1]
    qkv = torch.nn.functional.linear(x, wqkv, bqkv)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]

    def fmap(z):
        zs = z * d ** -0.25
        u = zs @ omega
        if kind == "rfa":
            return math.sqrt(2.0 / d) * torch.cat([torch.cos(u), torch.sin(u)], dim=-1)
        c = 0.5 * (zs * zs).sum(-1, keepdim=True) + 0.5 * math.log(d)
        return torch.cat([torch.exp(u - c), torch.exp(-u - c)], dim=-1)
    pq, pk = fmap(q), fmap(k)
    kv = pk.transpose(1, 2) @ v
    den = pq @ pk.sum(1).unsqueeze(-1) + eps
    return torch.nn.functional.linear(torch.cat([(pq @ kv) / den, pos], dim=-1), wout, bout)


@pytest.mark.parametrize("kind", KINDS)
def test_memory_below_torch_composition(gpu_device, kind):
    from galerkin_transformer import ops
    B, n, d = 2, 4096, 96
    T = B * n
    g = torch.Generator().manual_seed(3)
    dev = gpu_device
    x = (0.5 * torch.randn(B, n, d, generator=g)).to(dev)
    pos = torch.rand(B, n, 1, generator=g).to(dev)
    wqkv = (torch.randn(3 * d, d, generator=g) * 0.05).to(dev).requires_grad_(True)
    bqkv = torch.zeros(3 * d, device=dev, requires_grad=True)
    omega = torch.randn(d, d // 2, generator=g).to(dev)
    wout = (torch.randn(d, d + 1, generator=g) * 0.1).to(dev).requires_grad_(True)
    bout = torch.zeros(d, device=dev, requires_grad=True)
    cot = torch.randn(B, n, d, generator=g).to(dev)
    fused = lambda xx: ops.random_feature_attention(xx, pos, wqkv, bqkv, omega, wout, bout, kind=kind, eps=1e-6)
    plain = lambda xx: _torch_composition(xx, pos, wqkv, bqkv, omega, wout, bout, kind, 1e-6)

    def measure(fn):
        saved = []
        for it in range(2):     # the first trip warms the scratch buffer and the allocator
            saved.clear()
            xx = x.clone().requires_grad_(True)
            for p in (wqkv, bqkv, wout, bout):
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
                y = fn(xx)
            y.backward(cot)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            yv, gx = y.detach().clone(), xx.grad.clone()
            del y, xx
        uniq = {(t.data_ptr(), tuple(t.shape)): t for t in saved}
        return peak, list(uniq.values()), yv, gx

    peak_f, saved_f, y_f, gx_f = measure(fused)
    peak_t, saved_t, y_t, gx_t = measure(plain)
    print(f"{kind}: peak fused {peak_f / 2**20:.1f} MiB, torch composition {peak_t / 2**20:.1f} MiB; saved "
          f"{sum(t.numel() for t in saved_f) * 4 / 2**20:.1f} vs {sum(t.numel() for t in saved_t) * 4 / 2**20:.1f} MiB")
    assert rel_l2(y_f, y_t) < 1e-4 and rel_l2(gx_f, gx_t) < 1e-3      # the same function (the parity bars are above)
    assert peak_f < peak_t, (peak_f, peak_t)
    # token-sized tensors kept for the backward: x, the packed projection and the attention output -- with m = d a
    # [B, n, m] feature tensor would be a fourth [T, d]; the composition keeps those (and u, cos / sin or the exponents)
    big_f = sorted(tuple(t.shape) for t in saved_f if t.numel() >= T * d)
    assert big_f == [(T, d), (T, d), (T, 3 * d)], big_f
    big_t = [t for t in saved_t if t.numel() >= T * d]
    assert sum(t.numel() for t in _big(saved_f, T * d)) < sum(t.numel() for t in big_t)
    for t in _big(saved_f, T * d):     # each is a tensor the composition keeps as well: x, q | k | v, phi(q) KV / den
        flat = t.reshape(T, -1)
        hit = any(any(torch.allclose(flat[:, c * d:(c + 1) * d], s.reshape(T, -1)[:, :d], rtol=1e-3, atol=1e-5)
                      for s in saved_t if s.numel() >= T * d and s.reshape(T, -1).shape[1] >= d)
                  for c in range(flat.shape[1] // d))
        assert hit, tuple(t.shape)


def _big(saved, floor):
    return [t for t in saved if t.numel() >= floor]
