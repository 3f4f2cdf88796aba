"""The elementwise helpers of csrc/gt_ops.hip past their first grid-stride trip (-m gpu): gt_dropout_apply and gt_act_bwd
(4096 blocks: the second trip begins at element 1 048 576) at n = 1 048 833, gt_dropact_fwd / gt_dropact_bwd (8192 blocks of
f32x4: 8 388 608) at n = 8 389 635 = 8 388 608 + 1027 -- a partial block in the second trip and a scalar tail of 3 -- and
the scalar branch gt_dropact_* take when an operand is off a 16-byte boundary.

Bars.  KTOL = 2e-6 relative L2 against the float64 chain (the bar of test_kernels_gpu.py), and per element
|y - y64| <= 4 * 2^-23 * (|y64| + 1) for the fused dropout / activation pair: a skipped or repeated element is off by the
size of the value, far outside either.  The float32 torch chain on the same data is held to the per-element bar first; were
it outside, 4 x its figure would be the bar.  Measured (kernel, float32 torch) at 8 389 635, SiLU / SiLU: y 2.7e-7,
2.3e-7; gx 3.9e-7, 3.2e-7; ReLU / none: 4.8e-8 both; relative L2 at most 8.9e-8; gt_act_bwd SiLU 5.4e-8.
ReLU and identity gradients, p = 0 and the masks: exact.
"""
import pytest
import torch
import torch.nn.functional as F

from _util import rel_l2

pytestmark = pytest.mark.gpu

KTOL = 2e-6
ELT = 4 * 2.0 ** -23
N_1M = 1_048_576 + 257          # dropout_apply, act_bwd: second trip of 257 elements (one block and one thread)
N_8M = 8_388_608 + 1027         # dropact: second trip of 256 f32x4 (one block), then the tail of 3
N_SCALAR = 12_289               # dropact off a 16-byte boundary: 13 blocks, four trips of the scalar loop
SEED, SALT = 77, 11
ACT = {"relu": torch.relu, "silu": F.silu, "none": lambda t: t}


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


@pytest.fixture(scope="module")
def big():
    """x and the cotangent for the 8 M cases (CPU, float32), drawn once."""
    g = torch.Generator().manual_seed(90)
    return torch.randn(N_8M, generator=g), torch.randn(N_8M, generator=g)


def elt_err(a, b64):
    return float(((a.detach().double().cpu() - b64).abs() / (b64.abs() + 1)).max())


def masks(H, dev, n, p1, p2):
    """The two keep-scale masks the fused kernels draw at (SEED, SALT ..): read off ops.dropout of ones with the same
    seed and salts (gt_dropout_apply, which crosses its stride boundaries at other indices than gt_dropact_*)."""
    from galerkin_transformer import ops
    H.set_seed(SEED, dev)
    H._salt[0] = SALT
    ones = torch.ones(n, device=dev)
    return ops.dropout(ones, p1), ops.dropout(ones, p2)


def chain(x, gy, m1, m2, a1, a2, dtype):
    """act2(m2 * act1(m1 * x)) and its gradient for the cotangent gy, in plain torch on the CPU."""
    x = x.detach().to("cpu", dtype).requires_grad_(True)
    y = ACT[a2](ACT[a1](x * m1.to("cpu", dtype)) * m2.to("cpu", dtype))
    (gx,) = torch.autograd.grad(y, x, gy.to("cpu", dtype))
    return y.detach(), gx


def check_dropact(tag, y, gx, x, gy, m1, m2, a1, a2):
    y64, gx64 = chain(x, gy, m1, m2, a1, a2, torch.float64)
    y32, gx32 = chain(x, gy, m1, m2, a1, a2, torch.float32)
    for name, got, t32, want in (("y", y, y32, y64), ("gx", gx, gx32, gx64)):
        e, e32, l2 = elt_err(got, want), elt_err(t32, want), rel_l2(got, want)
        bar = ELT if e32 <= ELT else 4 * e32
        print(f"{tag} {name}: rel_l2 {l2:.2e} (bar {KTOL:.0e}); per element {e:.2e}, float32 torch {e32:.2e} (bar {bar:.2e})")
        assert l2 < KTOL, (tag, name, l2)
        assert e <= bar, (tag, name, e, e32, bar)


# ----------------------------------------------------------------------------------------------- dropout_apply
def test_dropout_apply_second_trip(H, gpu_device):
    """n = 1 048 833, p = 0.3: the mask depends on the element index alone (the first 4096 elements against a 4096-element
    call, the last 4096 -- which straddle the stride boundary -- against gt_dropact_fwd, still in its first trip there), the
    kept share is within 0.005 of 0.7 (more than 10 binomial standard deviations), kept values are 1 / 0.7; p = 0 copies."""
    dev, n, p = gpu_device, N_1M, 0.3
    H.set_seed(SEED, dev)
    d = H.dropout_desc(p, SALT, dev)
    ones = torch.ones(n, device=dev)
    out = H.dropout_apply(ones, d)
    assert torch.equal(out[:4096], H.dropout_apply(ones[:4096].clone(), d))
    fused = H.dropact_fwd(ones, d, H.ACT_NONE, H.dropout_desc(0.0, 0, dev), H.ACT_NONE)
    assert torch.equal(out[-4096:], fused[-4096:]) and torch.equal(out, fused)
    kept = out != 0
    share = kept.float().mean().item()
    print(f"dropout_apply: kept share {share:.5f}")
    assert abs(share - (1 - p)) < 0.005
    scale = 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))            # 1.f / (1.f - p), as the library forms it
    assert torch.equal(out[kept].cpu(), scale.expand(int(kept.sum())))
    assert abs(float(scale) - 1 / 0.7) < 2.0 ** -23 * (1 / 0.7)
    x = torch.randn(n, generator=torch.Generator().manual_seed(92)).to(dev)
    same = H.dropout_apply(x, H.dropout_desc(0.0, SALT, dev))
    assert torch.equal(same.view(torch.int32), x.view(torch.int32))
    tail = H.dropout_apply(x, d)                                           # and real data goes through the same mask
    assert torch.equal(tail, x * out)


# ----------------------------------------------------------------------------------------------- dropact
@pytest.mark.parametrize("p1,a1,p2,a2", [(0.1, "silu", 0.05, "silu"), (0.0, "relu", 0.2, "none")])
def test_dropact_second_trip(H, gpu_device, big, p1, a1, p2, a2):
    """ops.drop_act forward and backward at n = 8 389 635 against the float64 chain with the masks read off ops.dropout."""
    from galerkin_transformer import ops
    dev = gpu_device
    x0, gy0 = big
    H.set_seed(SEED, dev)
    H._salt[0] = SALT
    x = x0.to(dev).requires_grad_(True)
    y = ops.drop_act(x, p1, a1, True, p2, a2)
    y.backward(gy0.to(dev))
    m1, m2 = masks(H, dev, N_8M, p1, p2)
    for m, p in ((m1, p1), (m2, p2)):
        assert abs((m != 0).float().mean().item() - (1 - p)) < 0.005
    check_dropact(f"dropact {p1} {a1} {p2} {a2}", y, x.grad, x0, gy0, m1, m2, a1, a2)


def test_dropact_scalar_branch(H, gpu_device):
    """x, gy and the output one float into larger buffers (4 bytes off a 16-byte boundary): the kernels take their scalar
    loop (vec == 0).  Same checks at n = 12 289, and the floats around the output views keep their sentinel."""
    dev, n = gpu_device, N_SCALAR
    p1, a1, p2, a2 = 0.1, "silu", 0.05, "silu"
    g = torch.Generator().manual_seed(93)
    xb, gb = torch.randn(n + 8, generator=g).to(dev), torch.randn(n + 8, generator=g).to(dev)
    yb, gxb = torch.full((n + 8,), -1234.5, device=dev), torch.full((n + 8,), -1234.5, device=dev)
    x, gy, y, gx = (t[1:n + 1] for t in (xb, gb, yb, gxb))
    assert all(t.data_ptr() % 16 == 4 for t in (x, gy, y, gx))
    H.set_seed(SEED, dev)
    d1, d2 = H.dropout_desc(p1, SALT, dev), H.dropout_desc(p2, SALT + 1, dev)
    H._launch("gt_dropact_fwd", x, y, n, d1, H.ACT_CODE[a1], d2, H.ACT_CODE[a2])
    H._launch("gt_dropact_bwd", x, gy, gx, n, d1, H.ACT_CODE[a1], d2, H.ACT_CODE[a2])
    m1, m2 = masks(H, dev, n, p1, p2)
    check_dropact("dropact scalar", y, gx, x, gy, m1, m2, a1, a2)
    for b in (yb, gxb):
        assert float(b[0]) == -1234.5 and bool((b[n + 1:] == -1234.5).all())
    # the aligned call on the same values gives the same bits: the two loops differ in nothing but their indexing
    assert torch.equal(y, H.dropact_fwd(x.clone(), d1, H.ACT_CODE[a1], d2, H.ACT_CODE[a2]))
    assert torch.equal(gx, H.dropact_bwd(x.clone(), gy.clone(), d1, H.ACT_CODE[a1], d2, H.ACT_CODE[a2]))


# ----------------------------------------------------------------------------------------------- act_bwd
@pytest.mark.parametrize("act", ["silu", "relu", "none"])
def test_act_bwd_second_trip(H, gpu_device, act):
    """gt_act_bwd at n = 1 048 833 against float64 autograd; ReLU and the identity exactly."""
    dev, n = gpu_device, N_1M
    g = torch.Generator().manual_seed(94)
    pre, dout = torch.randn(n, generator=g), torch.randn(n, generator=g)
    got = H.act_bwd(dout.to(dev), pre.to(dev), H.ACT_CODE[act])
    x64 = pre.double().requires_grad_(True)
    (want,) = torch.autograd.grad(ACT[act](x64), x64, dout.double())
    l2 = rel_l2(got, want)
    print(f"act_bwd {act}: rel_l2 {l2:.2e} (bar {KTOL:.0e}), per element {elt_err(got, want):.2e}")
    assert l2 < KTOL
    if act != "silu":
        exact = dout if act == "none" else torch.where(pre > 0, dout, torch.zeros_like(dout))
        assert torch.equal(got.cpu(), exact)
