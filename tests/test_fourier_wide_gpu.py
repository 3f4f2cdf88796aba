"""The fp32-MFMA Fourier kernel at the 64- / 96-wide head tiles (DP = 68, 100; gt_fourier_attn_wide) on the device (-m gpu):
the three passes through H.fourier_attn against float64, the split of the widths between the two entry points, the module
in `f32` mode (fused against materialised, routing in every precision mode, memory linear in n, graph capture) and the
behaviour around it (narrow widths and the Galerkin path untouched).

Bars.  Kernels: max(KTOL = 2e-6, 12 x the deviation of the same formulas evaluated in float32 on the CPU from float64), per
result, relative L2 -- the large-range rule of test_softmax_wide_gpu.py; computed in the test on the CPU, never from a device
run.  Module routes: 5e-6, the bar test_kernels_gpu.py::test_fourier_fused_equals_materialised holds the narrow fp32 instances
to."""
import math
import time

import pytest
import torch

from _util import rel_l2
from test_softmax_attention_gpu import GT, KTOL, NS, B_, H_, _draw_mask, _heads, _tiles  # noqa: F401

pytestmark = pytest.mark.gpu

WIDE_DP = (68, 100)
ROUTE_TOL = 5e-6
RESULTS = ("O", "dQ", "dK", "dV")


def _formula(Q, K, V, dO, n, scale, m, dtype):
    """S = (Q' K'^T) scale .* m, O = S V' and its three gradients for the cotangent dO, in ``dtype`` on the CPU, [B, h, n, DP]."""
    q, k, v, do = (_heads(t.cpu(), n).to(dtype) for t in (Q, K, V, dO))
    S = (q @ k.transpose(-1, -2)) * scale
    dS = (do @ v.transpose(-1, -2)) * scale
    if m is not None:
        S, dS = S * m.cpu().to(dtype), dS * m.cpu().to(dtype)
    return dict(O=S @ v, dQ=dS @ k, dK=dS.transpose(-1, -2) @ q, dV=S.transpose(-1, -2) @ do)


def _device_run(_hip, dev, Q, K, V, dO, n, DP, scale, mask, drop):
    """Forward, d/dQ' and the dual d/dK' + d/dV' pass, twice: the second call is bit-identical, the pad columns are exact
    zeros, everything is finite."""
    Qd, Kd, Vd, dOd = (t.to(dev) for t in (Q, K, V, dO))
    md = None if mask is None else mask.to(dev).contiguous()

    def run():
        out = _hip.fourier_attn(Qd, None, Kd, Vd, B_, n, H_, DP, scale, md, drop, False)
        dq = _hip.fourier_attn(dOd, None, Vd, Kd, B_, n, H_, DP, scale, md, drop, False)
        dv, dk = _hip.fourier_attn(Kd, Vd, Qd, dOd, B_, n, H_, DP, scale, md, drop, True)
        return dict(O=out, dQ=dq, dK=dk, dV=dv)
    got, again = run(), run()
    torch.cuda.synchronize()
    for k in RESULTS:
        assert torch.equal(got[k], again[k]), ("second call differs", k)
        assert (got[k][..., DP - 2:] == 0).all(), ("pad columns", k)
        assert torch.isfinite(got[k]).all(), k
    return {k: _heads(t, n).cpu() for k, t in got.items()}


@pytest.mark.parametrize("mode", ("plain", "dropout", "mask"))
@pytest.mark.parametrize("DP", WIDE_DP)
def test_wide_kernels_vs_float64(GT, gpu_device, DP, mode):
    """n = 1, 63, 64, 65, 129, 257: one partial stream tile, exactly one, the tile boundary, a partial 128-owner block, more
    than one block.  Unit-normal head tiles with two zero pad columns, B = 2, h = 2."""
    from galerkin_transformer import _hip
    dev = gpu_device
    _hip.set_seed(20261018)
    for n in NS:
        scale = 1.0 / math.sqrt(DP - 2) / n
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
        r32 = _formula(Q, K, V, dO, n, scale, m, torch.float32)
        for k in RESULTS:
            bound = max(KTOL, 12.0 * rel_l2(r32[k], ref[k]))
            e = rel_l2(got[k], ref[k])
            print(f"DP {DP} {mode} n {n} {k}: {e:.2e} (bound {bound:.2e})")
            assert e < bound, (DP, mode, n, k, e, bound)


def test_entry_points_split_the_widths(GT, gpu_device):
    """gt_fourier_attn_wide answers GT_ENOTSUP (-4) for the narrow widths and for 84 / 116; gt_fourier_attn still does for
    68 and 100."""
    from galerkin_transformer import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    x = torch.zeros(64, 1, 116, device=gpu_device)
    p = x.data_ptr()
    for DP in (20, 52, 84, 116):
        assert lib.gt_fourier_attn_wide(p, None, p, p, p, None, 1, 64, 1, DP, 1.0, None, None, 0, st) == -4
        assert lib.gt_fourier_attn_wide(p, p, p, p, p, p, 1, 64, 1, DP, 1.0, None, None, 1, st) == -4
    for DP in (68, 100):
        assert lib.gt_fourier_attn(p, None, p, p, p, None, 1, 64, 1, DP, 1.0, None, None, 0, st) == -4
        assert lib.gt_fourier_attn(p, p, p, p, p, p, 1, 64, 1, DP, 1.0, None, None, 1, st) == -4
    torch.cuda.synchronize()


class _count_calls:
    """Hook H.fourier_attn and H.fourier16_attn: the head-tile widths they are called with, in order."""

    def __init__(self, H):
        self.H, self.f32, self.f16 = H, [], []

    def __enter__(self):
        H = self.H
        self.orig = (H.fourier_attn, H.fourier16_attn)
        o32, o16 = self.orig
        H.fourier_attn = lambda *a, **k: (self.f32.append(a[7]), o32(*a, **k))[1]
        H.fourier16_attn = lambda *a, **k: (self.f16.append(a[7]), o16(*a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.H.fourier_attn, self.H.fourier16_attn = self.orig


def _attention(gt, dev, d, h, p):
    torch.manual_seed(1)
    attn = gt.SimpleAttention(h, d, pos_dim=p, attention_type="fourier", norm=True, eps=1e-7, dropout=0.0).to(dev)
    with torch.no_grad():
        for prm in attn.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    return attn


def _step(H, attn, x0, pos, cot, need_w):
    """One forward + backward of the attention block under a fixed seed and salt: [out, dx, every parameter gradient]."""
    H.set_seed(4242, x0.device)
    H._salt[0] = 3
    for prm in attn.parameters():
        prm.grad = None
    x = x0.clone().requires_grad_(True)
    y, w = attn.fused_forward(x, pos, residual=x, need_weights=need_w)
    assert (w is None) == (not need_w)
    y.backward(cot)
    return [y.detach(), x.grad.detach()] + [prm.grad.detach().clone() for prm in attn.parameters()]


@pytest.mark.parametrize("B,n,d,h,p", [(2, 200, 96, 1, 1), (2, 131, 128, 2, 2), (1, 77, 96, 1, 1)])
@pytest.mark.parametrize("mode", ["off", "reference"])
def test_wide_module_fused_equals_materialised_f32(GT, gpu_device, B, n, d, h, p, mode):
    """SimpleAttention (Fourier, d_k = 96 / 64) in `f32` mode: need_weights=False -- the fused fp32 kernel, three calls at the
    wide width and none of the fp16 kernel -- against need_weights=True -- the materialising gt_gemm path, which calls neither
    -- with the same seed and salt: output, dx and every parameter gradient, attention dropout off and the reference's p = 0.5
    (one hash per element on both routes)."""
    from galerkin_transformer import _hip as H
    dev = gpu_device
    DP = H.round4(d // h + p)
    assert DP in WIDE_DP
    attn = _attention(GT, dev, d, h, p)
    x0 = torch.randn(B, n, d, device=dev)
    pos = torch.rand(B, n, p, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    res = []
    old = H.set_precision("f32")
    GT.set_attention_dropout(mode)
    try:
        assert not H.fourier16_active()
        for need_w in (True, False):
            with _count_calls(H) as calls:
                res.append(_step(H, attn, x0, pos, cot, need_w))
            assert calls.f16 == []
            assert calls.f32 == ([] if need_w else [DP] * 3)
    finally:
        GT.set_attention_dropout("reference")
        H.set_precision(old)
    names = ["out", "dx"] + [k for k, _ in attn.named_parameters()]
    errs = {k: rel_l2(b_, a) for k, a, b_ in zip(names, *res)}
    print(f"module d={d} h={h} p={p} {mode}:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < ROUTE_TOL, (k, v)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", None])
def test_routing_in_the_other_modes(GT, gpu_device, precision):
    """One forward + backward of the (1, 77, 96, 1, 1) module: the bf16 modes take the fp32 kernel three times, the default
    mode (None: whatever it is set to, the two-term fp16 arithmetic) still takes the fp16 kernel three times and the fp32 one
    never."""
    from galerkin_transformer import _hip as H
    dev = gpu_device
    B, n, d, h, p = 1, 77, 96, 1, 1
    attn = _attention(GT, dev, d, h, p)
    x0 = torch.randn(B, n, d, device=dev)
    pos = torch.rand(B, n, p, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    old = H.get_precision() if precision is None else H.set_precision(precision)
    try:
        with _count_calls(H) as calls:
            res = _step(H, attn, x0, pos, cot, False)
        if precision is None:
            assert H.fourier16_active()
            assert calls.f16 == [100] * 3 and calls.f32 == []
        else:
            assert calls.f32 == [100] * 3 and calls.f16 == []
    finally:
        H.set_precision(old)
    assert all(torch.isfinite(t).all() for t in res)


def test_wide_encoder_layer_memory_is_linear_in_n_f32(GT, gpu_device):
    """test_fourier16_wide_gpu.py::test_wide_encoder_layer_memory_is_linear_in_n in `f32` mode: one encoder layer of the
    shipped ex1 shape (d_model = 96, one head, one coordinate: DP = 100) at n = 32 768, forward + backward: the rise of the
    peak allocation stays below n^2 * 4 / 4 bytes (1.07 GB).  The fused fp32 route has no pre-split images, so it allocates
    less than the fp16 one; the materialised route keeps S and forms dS, 2 n^2 * 4 = 8.6 GB, and cannot pass.
    Rise and time on an MI355X: not measured yet (the test prints both)."""
    from galerkin_transformer import _hip as H
    dev = gpu_device
    B, n, d = 1, 32768, 96
    torch.manual_seed(0)
    layer = GT.SimpleTransformerEncoderLayer(d_model=d, pos_dim=1, n_head=1, dim_feedforward=2 * d,
                                             attention_type="fourier").to(dev)
    x = torch.randn(B, n, d, device=dev, requires_grad=True)
    pos = torch.rand(B, n, 1, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    old = H.set_precision("f32")
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        y = layer(x, pos)
        y.backward(cot)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rise = torch.cuda.max_memory_allocated(dev) - base
    finally:
        H.set_precision(old)
    print(f"peak rise {rise / 2 ** 20:.0f} MiB at n = {n} (n^2 * 4 bytes = {n * n * 4 / 2 ** 20:.0f} MiB), first call {dt:.2f} s")
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert rise < n * n * 4 / 4, rise


def test_graph_capture_replays_eager_f32(GT, gpu_device):
    """One forward + backward of the (1, 77, 96, 1, 1) module in `f32` mode, captured and replayed: bit-identical to eager."""
    from galerkin_transformer import _hip as H
    dev = gpu_device
    B, n, d, h, p = 1, 77, 96, 1, 1
    attn = _attention(GT, dev, d, h, p)
    x = torch.randn(B, n, d, device=dev).requires_grad_(True)
    pos = torch.rand(B, n, p, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    params = list(attn.parameters())
    old = H.set_precision("f32")
    GT.set_attention_dropout("off")
    try:
        def step():
            return torch.autograd.grad(attn.fused_forward(x, pos, residual=x, need_weights=False)[0], [x] + params, cot)
        with _count_calls(H) as calls:
            eager = [t.clone() for t in step()]
        assert calls.f32 == [100] * 3 and calls.f16 == []
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
        H.set_precision(old)
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def test_nothing_leaks(GT, gpu_device):
    """Around a wide fp32 step: a narrow Fourier layer (DP = 36) in `f32` mode still takes gt_fourier_attn, and a Galerkin layer
    at d_k = 96 gives the output it gave before."""
    from galerkin_transformer import _hip as H
    dev = gpu_device
    torch.manual_seed(5)
    gal = GT.SimpleTransformerEncoderLayer(d_model=96, pos_dim=1, n_head=1, dim_feedforward=192,
                                           attention_type="galerkin").to(dev).eval()
    narrow = GT.SimpleTransformerEncoderLayer(d_model=64, pos_dim=2, n_head=2, dim_feedforward=128,
                                              attention_type="fourier").to(dev)
    wide = GT.SimpleTransformerEncoderLayer(d_model=96, pos_dim=1, n_head=1, dim_feedforward=192,
                                            attention_type="fourier").to(dev)
    n = 150
    xg, pg = torch.randn(2, n, 96, device=dev), torch.rand(2, n, 1, device=dev)
    xn, pn = torch.randn(2, n, 64, device=dev, requires_grad=True), torch.rand(2, n, 2, device=dev)
    xw = torch.randn(2, n, 96, device=dev, requires_grad=True)

    def galerkin():
        H.set_seed(7, dev)
        with torch.no_grad():
            return gal(xg, pg).clone()
    old = H.set_precision("f32")
    try:
        before = galerkin()
        with H.Profile() as prof:
            wide(xw, pg).sum().backward()
            torch.cuda.synchronize()
        keys = [r[0] for r in prof.records]
        assert keys.count("gt_fourier_attn_wide") == 3 and "gt_fourier_attn" not in keys and "gt_fourier16_attn" not in keys
        with H.Profile() as prof:
            narrow(xn, pn).sum().backward()
            torch.cuda.synchronize()
        keys = [r[0] for r in prof.records]
        assert keys.count("gt_fourier_attn") == 3 and "gt_fourier_attn_wide" not in keys and "gt_fourier16_attn" not in keys
        assert [r[6][3] for r in prof.records if r[0] == "gt_fourier_attn"] == [36] * 3
        after = galerkin()
    finally:
        H.set_precision(old)
    assert torch.isfinite(before).all() and torch.equal(before, after)
