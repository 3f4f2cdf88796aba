"""gt_fourier16_* at the wide head tiles DP = 68 (d_k = 64) and DP = 100 (d_k = 96, the shipped ex1_burgers configuration),
case by case what tests/test_fourier16_gpu.py asks of DP = 20 / 36 / 52: the three uses against the float64 restatement with
no mask, an explicit mask and the three dropout modes, operand magnitudes far from 1, bit-identical reruns -- then the module
level (fused against materialising, same seed and salt) and the capability itself: memory linear in n.

The gate is that file's TOL: the arithmetic is the same (two-term split, three MFMAs, running exponent, alternating chain
signs), only the contraction of the first product is longer.  The fp32-MFMA kernel has no instance at these widths, so the
dropout masks are taken from the materialising path's own draws on a matrix of ones."""
import math

import pytest
import torch

from _util import rel_l2
from test_fourier16_gpu import TOL, _ref, _run16, _tiles

pytestmark = pytest.mark.gpu

MODULE_TOL = 1e-5   # the module gate of tests/test_modules_gpu.py

# both widths; n not a multiple of 32, n < 32, n = 32, h > 1, n >= 1000; the last two are big enough (16+ tiles and
# B h ceil(tiles / 8) >= 384) for the forward and d/dQ' passes to take the 8-wave launch
CASES = [(2, 200, 4, 68), (1, 77, 2, 100), (2, 131, 2, 100), (1, 1000, 2, 68), (1, 1031, 1, 100), (3, 32, 1, 100),
         (1, 5, 2, 68), (1, 5, 1, 100), (48, 512, 4, 68), (64, 520, 2, 100)]
DROP_CASES = [(2, 200, 4, 68), (1, 77, 2, 100), (2, 131, 2, 100)]


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


def _check(got, ref, DP, what):
    errs = {name: rel_l2(g, r) for name, g, r in zip(("out", "dQ", "dK", "dV"), got, ref)}
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for name, g in zip(errs, got):
        assert torch.isfinite(g).all(), name
        assert errs[name] < TOL, (name, errs[name])
        assert float(g[..., -2:].abs().max()) == 0.0, name          # pad columns of the outputs are exact zeros


@pytest.mark.parametrize("B,n,h,DP", CASES)
@pytest.mark.parametrize("mode", ["plain", "mask"])
def test_wide_matches_float64(H, gpu_device, B, n, h, DP, mode):
    dev = gpu_device
    Q, K, V, dO = (t.to(dev) for t in _tiles(B, n, h, DP, seed=n + DP))
    scale = 1.0 / math.sqrt(DP - 2) / n
    mask = None
    if mode == "mask":
        mask = (2.0 * (torch.rand(B, h, n, n, generator=torch.Generator().manual_seed(5)) < 0.5).float()).to(dev)
    ref = _ref(Q, K, V, dO, B, n, h, DP, scale, mask)
    got = _run16(H, Q, K, V, dO, B, n, h, DP, scale, mask, None)
    _check(got, ref, DP, f"{mode} B={B} n={n} h={h} DP={DP}")
    again = _run16(H, Q, K, V, dO, B, n, h, DP, scale, mask, None)
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                    # no atomics, no order left to the scheduler


@pytest.mark.parametrize("B,n,h,DP", DROP_CASES)
@pytest.mark.parametrize("p", [0.5, 0.3])
def test_wide_dropout_draws_the_mask_of_the_materialising_path(H, gpu_device, B, n, h, DP, p):
    """Per-element mode (p = 0.5 runs the top-bit shortcut, 0.3 the full hash): the mask is the one gt_dropout_apply draws on a
    [B, h, n, n] matrix with the same descriptor (flat index ((b h + head) n + query) n + key, the index of the score gt_gemm's
    drop= epilogue), replayed in float64."""
    dev = gpu_device
    Q, K, V, dO = (t.to(dev) for t in _tiles(B, n, h, DP, seed=7 * n))
    scale = 1.0 / math.sqrt(DP - 2) / n
    H.set_seed(991, dev)
    drop = H.dropout_desc(p, 11, dev)
    mask = H.dropout_apply(torch.ones(B, h, n, n, device=dev), drop)
    vals = set(round(v, 5) for v in mask.unique().tolist())
    assert vals == {0.0, round(1.0 / (1.0 - p), 5)}, vals
    assert abs(float((mask > 0).float().mean()) - (1.0 - p)) < 4.0 / math.sqrt(mask.numel())
    ref = _ref(Q, K, V, dO, B, n, h, DP, scale, mask)
    got = _run16(H, Q, K, V, dO, B, n, h, DP, scale, None, drop, block16=False)
    _check(got, ref, DP, f"dropout p={p} B={B} n={n} h={h} DP={DP}")
    again = _run16(H, Q, K, V, dO, B, n, h, DP, scale, None, drop, block16=False)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,n,h,DP", DROP_CASES + [(1, 5, 2, 68), (1, 5, 1, 100)])
def test_wide_block_mask(H, gpu_device, B, n, h, DP):
    """block16: gt_dropout_block16 materialises the p = 0.5 mask per 4 x 4 block; the three fused passes are held to float64 with
    exactly that mask; half the entries kept, the 16 bits of a block uncorrelated (as test_fourier16_block_mask)."""
    dev = gpu_device
    Q, K, V, dO = (t.to(dev) for t in _tiles(B, n, h, DP, seed=11 * n))
    scale = 1.0 / math.sqrt(DP - 2) / n
    H.set_seed(77, dev)
    drop = H.dropout_desc(0.5, 21, dev)
    mask = H.dropout_block16(torch.ones(B, h, n, n, device=dev), B * h, n, drop)
    assert set(mask.unique().tolist()) <= {0.0, 2.0}
    ref = _ref(Q, K, V, dO, B, n, h, DP, scale, mask)
    got = _run16(H, Q, K, V, dO, B, n, h, DP, scale, None, drop, block16=True)
    _check(got, ref, DP, f"block mask B={B} n={n} h={h} DP={DP}")
    again = _run16(H, Q, K, V, dO, B, n, h, DP, scale, None, drop, block16=True)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    if n >= 128:
        keep = (mask > 0).float()
        assert abs(float(keep.mean()) - 0.5) < 4.0 / math.sqrt(keep.numel())
        n4 = n // 4 * 4
        blocks = keep[..., :n4, :n4].reshape(B * h, n4 // 4, 4, n4 // 4, 4).permute(0, 1, 3, 2, 4).reshape(-1, 16)
        c = torch.corrcoef(blocks.T.double())
        off = c - torch.eye(16, device=dev, dtype=torch.float64)
        assert float(off.abs().max()) < 6.0 / math.sqrt(blocks.shape[0])


@pytest.mark.parametrize("DP", [68, 100])
@pytest.mark.parametrize("scales", [(1e-6, 1e5, 1e-3, 1e8), (1e4, 1e4, 1e4, 1e4), (1e-12, 1e-12, 1e-12, 1e-12)])
def test_wide_operand_magnitudes(H, gpu_device, scales, DP):
    """Per-tile exponents + the running accumulator exponent: tensors far from unit scale, token rows spread over three
    decades inside every tile."""
    dev = gpu_device
    B, n, h = 1, 333, 2
    Q, K, V, dO = (t.to(dev) for t in _tiles(B, n, h, DP, seed=3, scales=scales, ramp=3.0))
    scale = 1.0 / n
    ref = _ref(Q, K, V, dO, B, n, h, DP, scale, None)
    got = _run16(H, Q, K, V, dO, B, n, h, DP, scale, None, None)
    _check(got, ref, DP, f"magnitudes {scales} DP={DP}")


@pytest.mark.parametrize("B,n,h,DP", [(2, 300, 2, 68), (2, 300, 1, 100)])
@pytest.mark.parametrize("mode", ["plain", "block"])
def test_wide_dual_pass_equals_two_single_passes(H, gpu_device, B, n, h, DP, mode):
    """The dual pass is two single-output passes over the same owners that share their stream tiles -- O1 from (F1; T1, T2),
    O2 from (F2; T2, T1), the same products in the same order under the same running exponents -- so the results agree bit for
    bit, whichever way the library runs it (at DP = 68 it runs the two passes)."""
    dev = gpu_device
    Q, K, V, dO = (t.to(dev) for t in _tiles(B, n, h, DP, seed=13, ramp=2.0))
    iq, ik, iv, ido = H.fourier16_presplit((Q, K, V, dO), B, n, h, DP)
    H.set_seed(31, dev)
    drop = H.dropout_desc(0.5, 9, dev) if mode == "block" else None
    dv, dk = H.fourier16_attn(ik, iv, iq, ido, B, n, h, DP, 1.0 / n, None, drop, True)
    dv1 = H.fourier16_attn(ik, None, iq, ido, B, n, h, DP, 1.0 / n, None, drop, True)
    dk1 = H.fourier16_attn(iv, None, ido, iq, B, n, h, DP, 1.0 / n, None, drop, True)
    torch.cuda.synchronize()
    assert torch.equal(dv, dv1) and torch.equal(dk, dk1)


def test_unbuilt_widths_are_refused(H, gpu_device):
    """The dispatchers have no default arm: a width without an instance is GT_ENOTSUP, never the nearest instance."""
    dev = gpu_device
    for DP in (84, 64, 96, 116):
        x = torch.zeros(40, 1, DP, device=dev)
        with pytest.raises(H.GtNotSupported):
            H.fourier16_presplit((x,), 1, 40, 1, DP)
        img = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        with pytest.raises(H.GtNotSupported):
            H.fourier16_attn(img, None, img, img, 1, 40, 1, DP, 1.0, None, None, False)


@pytest.mark.parametrize("B,n,d,h,p", [(2, 200, 96, 1, 1), (2, 131, 128, 2, 2), (1, 77, 96, 1, 1)])
@pytest.mark.parametrize("mode", ["off", "reference"])
def test_wide_module_fused_equals_materialised(H, gpu_device, B, n, d, h, p, mode):
    """SimpleAttention (Fourier, d_k = 96 / 64): fused_forward(need_weights=False) -- the fused kernels, which the wide head
    tiles now take -- against need_weights=True -- the materialising gt_gemm path -- with the same seed and salt: outputs, input
    gradient and every parameter gradient, attention dropout off and the reference's p = 0.5 (block mask on both paths)."""
    import galerkin_transformer as gt
    from galerkin_transformer import ops
    dev = gpu_device
    assert H.fourier16_active() and H.round4(d // h + p) in (68, 100)
    torch.manual_seed(1)
    attn = gt.SimpleAttention(h, d, pos_dim=p, attention_type="fourier", norm=True, eps=1e-7, dropout=0.0).to(dev)
    with torch.no_grad():
        for prm in attn.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    x0 = torch.randn(B, n, d, device=dev)
    pos = torch.rand(B, n, p, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    res, calls = [], []
    orig = H.fourier16_attn
    H.fourier16_attn = lambda *a, **k: (calls.append(a[7]), orig(*a, **k))[1]
    gt.set_attention_dropout(mode)
    try:
        for need_w in (True, False):
            H.set_seed(4242, dev)
            H._salt[0] = 3
            for prm in attn.parameters():
                prm.grad = None
            x = x0.clone().requires_grad_(True)
            before = len(calls)
            y, w = attn.fused_forward(x, pos, residual=x, need_weights=need_w)
            assert (w is None) == (not need_w)
            y.backward(cot)
            # the materialising path never enters the fused kernel; the fused one runs it three times at this width
            assert calls[before:] == ([] if need_w else [H.round4(d // h + p)] * 3)
            res.append([y.detach(), x.grad.detach()] + [prm.grad.detach().clone() for prm in attn.parameters()])
    finally:
        gt.set_attention_dropout("reference")
        H.fourier16_attn = orig
    names = ["out", "dx"] + [k for k, _ in attn.named_parameters()]
    errs = {k: rel_l2(b_, a) for k, a, b_ in zip(names, *res)}
    print(f"module d={d} h={h} p={p} {mode}:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < MODULE_TOL, (k, v)


def test_wide_encoder_layer_memory_is_linear_in_n(H, gpu_device):
    """One encoder layer of the shipped ex1 shape (d_model = 96, one head, one coordinate: DP = 100) at n = 32 768, forward +
    backward: the rise of the peak allocation stays below n^2 * 4 / 4 bytes (1.07 GB).  Every buffer of the fused path is
    linear in n (head tiles 3 x 13 MB, four image blocks of 28 MB, the layer's activations); the materialising path keeps
    S and forms dS, 2 n^2 * 4 = 8.6 GB, and cannot pass."""
    import galerkin_transformer as gt
    dev = gpu_device
    B, n, d = 1, 32768, 96
    torch.manual_seed(0)
    layer = gt.SimpleTransformerEncoderLayer(d_model=d, pos_dim=1, n_head=1, dim_feedforward=2 * d,
                                             attention_type="fourier").to(dev)
    x = torch.randn(B, n, d, device=dev, requires_grad=True)
    pos = torch.rand(B, n, 1, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    y = layer(x, pos)
    y.backward(cot)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak rise {rise / 2 ** 20:.0f} MiB at n = {n} (n^2 * 4 bytes = {n * n * 4 / 2 ** 20:.0f} MiB)")
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert rise < n * n * 4 / 4, rise
