"""Kernel-level parity: every C-ABI entry point of libgt_hip.so against a plain torch fp64
restatement of the same op, on the GPU box.  (-m gpu)"""
import os

import pytest
import torch

import _galerkin_ref as G
from _util import rel_l2

pytestmark = pytest.mark.gpu

KTOL = 2e-6   # fp32 accumulation-order noise


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def ref_mm(A, B, la, lb):
    a = A.double() if la == 0 else A.double().transpose(-1, -2)      # -> [..., M, K]
    b = B.double().transpose(-1, -2) if lb == 0 else B.double()      # -> [..., K, N]
    return a @ b


@pytest.mark.parametrize("la,lb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (130, 36, 150), (64, 128, 16), (141, 32, 24),
                                   (200, 1, 128), (48, 384, 282), (1000, 256, 130), (33, 130, 7)])
def test_gemm_layouts(H, gpu_device, la, lb, M, N, K):
    dev = gpu_device
    A = rnd(M, K, dev=dev, seed=1) if la == 0 else rnd(K, M, dev=dev, seed=1)
    B = rnd(N, K, dev=dev, seed=2) if lb == 0 else rnd(K, N, dev=dev, seed=2)
    Cc = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, B, Cc, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1], ldb=B.shape[1], ldc=N)
    torch.cuda.synchronize()
    assert rel_l2(Cc, ref_mm(A, B, la, lb)) < KTOL


def test_gemm_asymmetric_identity(H, gpu_device):
    """A = I with an asymmetric B catches a transposed accumulator layout."""
    dev = gpu_device
    n = 96
    A = torch.eye(n, device=dev)
    B = (torch.arange(n * n, device=dev, dtype=torch.float32).reshape(n, n) % 97) / 7.0   # B[n][k]
    Cc = torch.empty(n, n, device=dev)
    H.gemm(A, B, Cc, n, n, n, lda=n, ldb=n, ldc=n)
    torch.cuda.synchronize()
    assert torch.equal(Cc, B.t().contiguous())


@pytest.mark.parametrize("la,lb", [(0, 0), (1, 1)])
def test_gemm_batched_strided(H, gpu_device, la, lb):
    """Two-level batch (b, head) on strided head-interleaved operands, as used by K^T V / Q M."""
    dev = gpu_device
    Bn, h, n, DP = 3, 4, 257, 36
    X = rnd(Bn, n, h, DP, dev=dev, seed=3)
    Y = rnd(Bn, n, h, DP, dev=dev, seed=4)
    if la == 1:      # M = X^T Y per (b,h): reduction over tokens
        out = torch.empty(Bn, h, DP, DP, device=dev)
        H.gemm(X, Y, out, DP, DP, n, layout_a=1, layout_b=1, lda=h * DP, ldb=h * DP, ldc=DP,
               batch=(Bn, h), a_bs=(n * h * DP, DP), b_bs=(n * h * DP, DP), c_bs=(h * DP * DP, DP * DP),
               split_k=0)
        ref = torch.einsum("bnhd,bnhe->bhde", X.double(), Y.double())
    else:            # out = X W^T per (b,h) with W [DP,DP]
        W = rnd(Bn, h, DP, DP, dev=dev, seed=5)
        out = torch.empty(Bn, n, h, DP, device=dev)
        H.gemm(X, W, out, n, DP, DP, layout_a=0, layout_b=0, lda=h * DP, ldb=DP, ldc=h * DP,
               batch=(Bn, h), a_bs=(n * h * DP, DP), b_bs=(h * DP * DP, DP * DP), c_bs=(n * h * DP, DP))
        ref = torch.einsum("bnhd,bhed->bnhe", X.double(), W.double())
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < KTOL


@pytest.mark.parametrize("split", [0, 3, 16])
def test_gemm_split_k(H, gpu_device, split):
    dev = gpu_device
    M, N, K = 256, 128, 5000
    A = rnd(K, M, dev=dev, seed=6)
    B = rnd(K, N, dev=dev, seed=7)
    Cc = torch.empty(M, N, device=dev)
    H.gemm(A, B, Cc, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=split, alpha=0.5)
    torch.cuda.synchronize()
    assert rel_l2(Cc, 0.5 * (A.double().t() @ B.double())) < KTOL


def test_gemm_epilogue_bias_act_res(H, gpu_device):
    dev = gpu_device
    M, N, K = 333, 256, 128
    A, W, b = rnd(M, K, dev=dev, seed=8), rnd(N, K, dev=dev, seed=9, scale=0.2), rnd(N, dev=dev, seed=10)
    R = rnd(M, N, dev=dev, seed=11)
    for act, fn in ((H.ACT_RELU, torch.relu), (H.ACT_SILU, torch.nn.functional.silu)):
        Cc = torch.empty(M, N, device=dev)
        pre = torch.empty(M, N, device=dev)
        H.gemm(A, W, Cc, M, N, K, lda=K, ldb=K, ldc=N, bias=b, act=act, res=R, ldr=N, out_scale=-1.0,
               pre=pre, ldpre=N, alpha=2.0)
        torch.cuda.synchronize()
        p64 = 2.0 * (A.double() @ W.double().t()) + b.double()
        assert rel_l2(pre, p64) < KTOL
        assert rel_l2(Cc, R.double() - fn(p64)) < KTOL


def test_gemm_rank_update_and_unaligned_b(H, gpu_device):
    """fc(cat[x, grid]) as x W[:, :K]^T + grid W[:, K:]^T (regressor fc, model.py:615-617)."""
    dev = gpu_device
    M, N, K, p = 500, 32, 128, 2
    x, grid = rnd(M, K, dev=dev, seed=12), rnd(M, p, dev=dev, seed=13)
    W, b = rnd(N, K + p, dev=dev, seed=14, scale=0.2), rnd(N, dev=dev, seed=15)
    Cc = torch.empty(M, N, device=dev)
    H.gemm(x, W, Cc, M, N, K, lda=K, ldb=K + p, ldc=N, bias=b, rp=p, rp_a=grid, rp_lda=p,
           rp_b=W[:, K:], rp_ldb=K + p)
    torch.cuda.synchronize()
    ref = torch.cat([x, grid], -1).double() @ W.double().t() + b.double()
    assert rel_l2(Cc, ref) < KTOL


def test_gemm_aux_ops(H, gpu_device):
    dev = gpu_device
    M, N, K = 200, 96, 64
    A, W = rnd(M, K, dev=dev, seed=16), rnd(N, K, dev=dev, seed=17)
    aux = rnd(M, N, dev=dev, seed=18)
    ref = A.double() @ W.double().t()
    Cc = torch.empty(M, N, device=dev)
    H.gemm(A, W, Cc, M, N, K, lda=K, ldb=K, ldc=N, aux_op=H.AUX_GT0, aux=aux, ldaux=N, aux_scale=1.25)
    torch.cuda.synchronize()
    assert rel_l2(Cc, ref * (aux.double() > 0) * 1.25) < KTOL
    H.gemm(A, W, Cc, M, N, K, lda=K, ldb=K, ldc=N, aux_op=H.AUX_DSILU, aux=aux, ldaux=N)
    torch.cuda.synchronize()
    a = aux.double().requires_grad_(True)
    ds, = torch.autograd.grad(torch.nn.functional.silu(a).sum(), a)
    assert rel_l2(Cc, ref * ds) < KTOL
    H.gemm(A, W, Cc, M, N, K, lda=K, ldb=K, ldc=N, aux_op=H.AUX_MUL, aux=aux, ldaux=N, aux_scale=2.0)
    torch.cuda.synchronize()
    assert rel_l2(Cc, ref * aux.double() * 2.0) < KTOL


def test_dropout_consistency_and_rate(H, gpu_device):
    """Epilogue dropout, A-prologue dropout and gt_dropout_apply draw the same mask per index."""
    dev = gpu_device
    H.set_seed(1234, dev)
    M, N, K = 256, 128, 64
    d = H.dropout_desc(0.3, salt=77, device=dev)
    ones = torch.ones(M * N, device=dev)
    mask = H.dropout_apply(ones, d).reshape(M, N)
    torch.cuda.synchronize()
    keep = (mask > 0).float().mean().item()
    assert abs(keep - 0.7) < 0.01
    assert torch.allclose(mask[mask > 0], torch.tensor(1 / 0.7, device=dev))
    # epilogue
    A, W = rnd(M, K, dev=dev, seed=19), rnd(N, K, dev=dev, seed=20)
    Cc = torch.empty(M, N, device=dev)
    H.gemm(A, W, Cc, M, N, K, lda=K, ldb=K, ldc=N, drop=d)
    torch.cuda.synchronize()
    assert rel_l2(Cc, (A.double() @ W.double().t()) * mask.double()) < KTOL
    # prologue on A = G [M, N] (mask index space of the [M,N] tensor): C2 = (G*mask) @ W2^T
    G, W2 = rnd(M, N, dev=dev, seed=21), rnd(48, N, dev=dev, seed=22)
    C2 = torch.empty(M, 48, device=dev)
    H.gemm(G, W2, C2, M, 48, N, lda=N, ldb=N, ldc=48, a_drop=d, a_drop_ld=N, a_drop_sign=-1.0)
    torch.cuda.synchronize()
    assert rel_l2(C2, -(G.double() * mask.double()) @ W2.double().t()) < KTOL
    # transposed use: C3 = (G*mask)^T X   (weight-gradient form)
    X = rnd(M, 40, dev=dev, seed=23)
    C3 = torch.empty(N, 40, device=dev)
    H.gemm(G, X, C3, N, 40, M, layout_a=1, layout_b=1, lda=N, ldb=40, ldc=40, a_drop=d, a_drop_ld=N)
    torch.cuda.synchronize()
    assert rel_l2(C3, (G.double() * mask.double()).t() @ X.double()) < KTOL
    # colsum with the same mask
    cs = H.colsum(G, M, N, N, a_drop=d)
    torch.cuda.synchronize()
    assert rel_l2(cs, (G.double() * mask.double()).sum(0)) < KTOL
    # a different seed gives a different mask; advancing is deterministic
    H.advance_seed(dev)
    mask2 = H.dropout_apply(ones, d).reshape(M, N)
    torch.cuda.synchronize()
    assert (mask2 != mask).float().mean().item() > 0.2


def _headnorm_ref(qkv, pos, gamma, beta, h, dk, p, norm_mask, eps):
    T = qkv.shape[0]
    DP = (dk + p + 3) // 4 * 4
    s = qkv.reshape(T, 3, h, dk)
    outs, ni = [], 0
    for st in range(3):
        v = s[:, st]
        if (norm_mask >> st) & 1:
            mu = v.mean(-1, keepdim=True)
            var = ((v - mu) ** 2).mean(-1, keepdim=True)
            v = (v - mu) / torch.sqrt(var + eps) * gamma[ni] + beta[ni]
            ni += 1
        parts = []
        if p:
            parts.append(pos[:, None, :].expand(T, h, p))
        parts.append(v)
        if DP - dk - p:
            parts.append(torch.zeros(T, h, DP - dk - p, dtype=v.dtype, device=v.device))
        outs.append(torch.cat(parts, -1))
    return torch.stack(outs)


def _headnorm_case(H, dev, T, h, dk, p, mask, eps=1e-7):
    """One forward and backward of H.headnorm_* against the float64 reference, at the suite's gates."""
    DP = (dk + p + 3) // 4 * 4
    qkv = rnd(T, 3 * h * dk, dev=dev, seed=24)
    pos = torch.rand(T, p, device=dev)
    gamma = 1 + 0.1 * rnd(2, h, dk, dev=dev, seed=25)
    beta = 0.1 * rnd(2, h, dk, dev=dev, seed=26)
    out, stats = H.headnorm_fwd(qkv, pos, gamma, beta, T, h, dk, p, mask, eps)
    q64 = qkv.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = _headnorm_ref(q64, pos.double(), g64, b64, h, dk, p, mask, eps)
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < KTOL
    assert torch.equal(out[..., p + dk:], torch.zeros(3, T, h, DP - dk - p, device=dev)), "pad columns"
    assert torch.equal(out[..., :p], pos[None, :, None, :].expand(3, T, h, p)), "coordinate columns"
    cot = rnd(*out.shape, dev=dev, seed=27)
    dq, dg, db = H.headnorm_bwd(cot, qkv, gamma, stats, T, h, dk, p, mask)
    torch.cuda.synchronize()
    grads = torch.autograd.grad(ref, [q64, g64, b64], cot.double(), allow_unused=True)
    assert rel_l2(dq, grads[0]) < 5 * KTOL
    nn_ = bin(mask).count("1")
    if mask:
        assert rel_l2(dg[:nn_], grads[1][:nn_]) < 5 * KTOL
        assert rel_l2(db[:nn_], grads[2][:nn_]) < 5 * KTOL
    if nn_ == 1:          # the slot with no stream behind it
        assert not dg[1].any() and not db[1].any()
    if not mask:          # no norm: a copy forward, a scatter backward
        assert torch.equal(out[..., p:p + dk], qkv.reshape(T, 3, h, dk).transpose(0, 1))
        assert torch.equal(dq.reshape(T, 3, h, dk), cot[..., p:p + dk].transpose(0, 1))


# The first five run the three-stream kernels.  The rest are what those do not take, and run the head-tile kernels per stream:
# dk % 4 != 0 with a last lane of 2 / 1 / 3 floats, with and without coordinates, two streams with and without a gap between
# them, one stream, none; and dk % 4 == 0 with 3 h G = 1536 lanes per token (the float4 head-tile kernels).
@pytest.mark.parametrize("h,dk,p,mask", [(4, 32, 2, 6), (4, 16, 1, 3), (1, 96, 1, 6), (2, 48, 2, 6),
                                         (1, 48, 2, 0),
                                         (3, 10, 1, 6), (2, 6, 0, 3), (1, 33, 2, 5), (2, 6, 0, 2), (5, 7, 3, 0),
                                         (16, 96, 1, 6)])
def test_headnorm_fwd_bwd(H, gpu_device, h, dk, p, mask):
    for T in (1, 1003):          # one block; several blocks of partials
        _headnorm_case(H, gpu_device, T, h, dk, p, mask)


@pytest.mark.parametrize("T", [17, 1003])
@pytest.mark.parametrize("h,dk,p,mask,off", [(3, 10, 1, 6, 0), (2, 8, 2, 3, 1)])
def test_headnorm_fallback_is_headtile_per_stream(H, gpu_device, h, dk, p, mask, off, T):
    """Off the three-stream kernels (dk % 4 != 0; qkv one float off a 16-byte boundary) headnorm_* is headtile_* on the
    three column blocks: the same kernels on the same pointers, so every output is identical."""
    dev, hd, eps = gpu_device, h * dk, 1e-7
    qkv = rnd(T * 3 * hd + off, dev=dev, seed=31)[off:].view(T, 3 * hd)
    assert qkv.data_ptr() % 16 == 4 * off
    pos = torch.rand(T, p, device=dev)
    gamma = 1 + 0.1 * rnd(2, h, dk, dev=dev, seed=32)
    beta = 0.1 * rnd(2, h, dk, dev=dev, seed=33)
    out, stats = H.headnorm_fwd(qkv, pos, gamma, beta, T, h, dk, p, mask, eps)
    cot = rnd(*out.shape, dev=dev, seed=34)
    dq, dg, db = H.headnorm_bwd(cot, qkv, gamma, stats, T, h, dk, p, mask)
    dq2 = torch.empty_like(dq)
    dg2, db2 = torch.zeros_like(dg), torch.zeros_like(db)
    ni = 0
    for s in range(3):
        X, normed = qkv[:, s * hd:], bool((mask >> s) & 1)
        gm, bt = (gamma[ni], beta[ni]) if normed else (None, None)
        tiles, st = H.headtile_fwd(X, 3 * hd, pos, gm, bt, T, h, dk, p, eps)
        assert torch.equal(out[s], tiles), s
        if normed:
            assert torch.equal(stats[ni], st), s
        H.headtile_bwd(cot[s], X, 3 * hd, gm, st, T, h, dk, p, dq2[:, s * hd:], 3 * hd,
                       dg2[ni] if normed else None, db2[ni] if normed else None)
        ni += normed
    torch.cuda.synchronize()
    assert torch.equal(dq, dq2) and torch.equal(dg, dg2) and torch.equal(db, db2)


def test_headnorm_refuses_heads_wider_than_256(H, gpu_device):
    """dk = 260 is past the head-tile kernels' lanes: GT_ENOTSUP from both entry points before any launch."""
    lib, st, T, dk = H.lib(), H.stream_ptr(), 4, 260
    x, o, g = (torch.zeros(n, device=gpu_device) for n in (T * 3 * dk, 3 * T * dk, 2 * dk))
    stats = torch.zeros(2 * T * 2, device=gpu_device)
    ws = torch.zeros(lib.gt_headnorm_bwd_ws_bytes(T, 1, dk) // 4, device=gpu_device)
    assert lib.gt_headnorm_fwd(x.data_ptr(), None, g.data_ptr(), g.data_ptr(), T, 1, dk, 0, 6, 1e-5, o.data_ptr(),
                               stats.data_ptr(), st) == -4
    assert lib.gt_headnorm_bwd(o.data_ptr(), x.data_ptr(), g.data_ptr(), stats.data_ptr(), T, 1, dk, 0, 6, x.data_ptr(),
                               g.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel() * 4, st) == -4
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,h,dk,p,d", [(2, 4, 32, 2, 128), (1, 1, 96, 1, 96), (3, 2, 48, 2, 96)])
@pytest.mark.parametrize("use_mask", [False, True])
def test_galerkin_finalize(H, gpu_device, B, h, dk, p, d, use_mask):
    dev = gpu_device
    Dr, n = dk + p, 777
    DP = (Dr + 3) // 4 * 4
    S = 3
    slabs = rnd(S, B, h, DP, DP, dev=dev, seed=28)
    Wfc = rnd(d, h * Dr, dev=dev, seed=29, scale=0.3)
    mask = ((torch.rand(B, h, DP, DP, device=dev) > 0.5).float() * 2.0) if use_mask else None
    Mt, P = H.galerkin_finalize_fwd(slabs, S, B * h * DP * DP, B, h, DP, Dr, d, n, mask, None, Wfc)
    Mt2, P2, Pv = H.galerkin_finalize_fwd(slabs, S, B * h * DP * DP, B, h, DP, Dr, d, n, mask, None, Wfc, value_rows_of=p)
    torch.cuda.synchronize()
    assert torch.equal(Mt, Mt2) and torch.equal(P, P2)
    assert torch.equal(Pv, P.view(B, h, DP, d)[:, :, p:p + dk, :].reshape(B, h * dk, d))   # the value rows, compact
    s64 = slabs.double().requires_grad_(True)
    w64 = Wfc.double().requires_grad_(True)
    M64 = s64.sum(0)[..., :Dr, :Dr] / n
    if use_mask:
        M64 = M64 * mask.double()[..., :Dr, :Dr]
    P64 = torch.einsum("bhje,che->bhjc", M64, w64.reshape(d, h, Dr))
    assert rel_l2(Mt[..., :Dr, :Dr], M64) < KTOL
    assert float(Mt[..., Dr:, :].abs().max()) == 0 and float(Mt[..., :, Dr:].abs().max()) == 0
    Pv = P.reshape(B, h, DP, d)
    assert rel_l2(Pv[:, :, :Dr], P64) < KTOL
    assert float(Pv[:, :, Dr:].abs().max()) == 0 if DP > Dr else True
    # backward: cotangent on P, given as dPt[b][c][h*DP + j]
    cot = rnd(B, h, DP, d, dev=dev, seed=30)
    dPt = cot.permute(0, 3, 1, 2).reshape(B, d, h * DP).contiguous()
    dM, dWs = H.galerkin_finalize_bwd(dPt, Mt, mask, None, Wfc, B, h, DP, Dr, d, n)
    torch.cuda.synchronize()
    gs, gw = torch.autograd.grad(P64, [s64, w64], cot.double()[:, :, :Dr])
    # dM is the gradient w.r.t. the un-normalised K'^T V' sum (every slab sees the same gradient)
    assert rel_l2(dM[..., :Dr, :Dr], gs[0][..., :Dr, :Dr]) < 5 * KTOL
    assert rel_l2(dWs.sum(0), gw) < 5 * KTOL


def test_layernorm(H, gpu_device):
    dev = gpu_device
    for T, d in ((1000, 48), (517, 128), (64, 200), (70001, 48), (33, 64), (5, 4), (4099, 20)):   # d <= 64: narrow-row kernels
        x = rnd(T, d, dev=dev, seed=31)
        g, b = 1 + 0.1 * rnd(d, dev=dev, seed=32), 0.1 * rnd(d, dev=dev, seed=33)
        y, st = H.layernorm_fwd(x, g, b, 1e-5)
        x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
        ref = torch.nn.functional.layer_norm(x64, (d,), g64, b64, 1e-5)
        torch.cuda.synchronize()
        assert rel_l2(y, ref) < KTOL
        cot = rnd(T, d, dev=dev, seed=34)
        dx, dg, db = H.layernorm_bwd(cot, x, g, st)
        torch.cuda.synchronize()
        gx, gg, gb = torch.autograd.grad(ref, [x64, g64, b64], cot.double())
        assert rel_l2(dx, gx) < 5 * KTOL and rel_l2(dg, gg) < 5 * KTOL and rel_l2(db, gb) < 5 * KTOL


@pytest.mark.parametrize("B,Cin,Cout,Q,qtot,qoff", [(4, 32, 32, 144, 288, 144), (3, 8, 16, 16, 16, 0),
                                                    (20, 20, 12, 36, 72, 0), (40, 32, 32, 144, 288, 0),
                                                    (33, 8, 8, 16, 16, 0), (9, 64, 48, 16, 16, 0)])
def test_modemix(H, gpu_device, B, Cin, Cout, Q, qtot, qoff):
    dev = gpu_device
    X = rnd(B, 2, qtot, Cin, dev=dev, seed=35)
    W = rnd(Cin, Cout, Q, 2, dev=dev, seed=36, scale=0.3)
    Y = torch.zeros(B, 2, qtot, Cout, device=dev)
    H.modemix_fwd(X, W, Y, B, Q, Cin, Cout, qtot, qoff)
    torch.cuda.synchronize()
    x64 = X.double().requires_grad_(True)
    w64 = W.double().requires_grad_(True)
    xc = torch.complex(x64[:, 0, qoff:qoff + Q], x64[:, 1, qoff:qoff + Q])       # [B,Q,Cin]
    wc = torch.complex(w64[..., 0], w64[..., 1])                                  # [Cin,Cout,Q]
    yc = torch.einsum("bqi,ioq->bqo", xc, wc)
    ref = torch.stack([yc.real, yc.imag], 1)
    assert rel_l2(Y[:, :, qoff:qoff + Q], ref) < KTOL
    cot = rnd(B, 2, qtot, Cout, dev=dev, seed=37)
    dX = torch.zeros_like(X)
    dW = torch.empty_like(W)
    H.modemix_bwd(X, W, cot, dX, dW, B, Q, Cin, Cout, qtot, qoff)
    torch.cuda.synchronize()
    gx, gw = torch.autograd.grad(ref, [x64, w64], cot.double()[:, :, qoff:qoff + Q])
    assert rel_l2(dX, gx) < 5 * KTOL
    assert rel_l2(dW, gw) < 5 * KTOL


def test_misc_reductions(H, gpu_device):
    dev = gpu_device
    A = rnd(5000, 130, dev=dev, seed=38)
    cs = H.colsum(A, 5000, 130, 130)
    torch.cuda.synchronize()
    assert rel_l2(cs, A.double().sum(0)) < KTOL
    pre, g = rnd(1000, 33, dev=dev, seed=39), rnd(1000, 33, dev=dev, seed=40)
    out = H.act_bwd(g, pre, H.ACT_SILU)
    p64 = pre.double().requires_grad_(True)
    ref, = torch.autograd.grad(torch.nn.functional.silu(p64), p64, g.double())
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < KTOL


def test_ops_refuse_cpu_tensors(H):
    """No silent CPU fallback: the product path must fail loudly off-device."""
    a = torch.zeros(4, 4)
    with pytest.raises(RuntimeError):
        H.gemm(a, a, a, 4, 4, 4, lda=4, ldb=4, ldc=4)


# ------------------------------------------------------------------------------------------ bilinear resize
@pytest.mark.parametrize("in_nhwc,out_nhwc", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("B,C,ni,no,act", [(2, 128, 43, 77, 0), (2, 128, 78, 43, 1), (1, 36, 141, 78, 1),
                                           (3, 8, 5, 33, 0), (1, 4, 7, 1, 0), (2, 68, 1, 6, 0),
                                           (1, 12, 34, 34, 1), (1, 8, 4, 30, 1), (1, 4, 2, 9, 1)])
def test_bilinear_resize_layouts(H, gpu_device, in_nhwc, out_nhwc, B, C, ni, no, act):
    """gt_bilinear2d_fwd/bwd against F.interpolate(mode='bilinear', align_corners=True) (+ReLU) on the
    CPU in fp32 (the reference's arithmetic: source index and weights are fp32 there too), every layout
    combination, up- and down-sampling, degenerate sizes.  The last two: more contributing outputs per input cell than
    the backward's register tables hold (RS_MAXT = 6), with the ReLU gate -- on both axes (4 -> 30, 7 -> 28), and on the
    rows only (2 -> 9) while the columns (5 -> 7) fit."""
    import torch.nn.functional as F
    nj, nq = ni + 3, max(1, no - 2)                     # non-square: H = ni -> no, W = nj -> nq
    x = rnd(B, C, ni, nj, dev="cpu", seed=1).requires_grad_(True)
    y = F.interpolate(x, size=(no, nq), mode="bilinear", align_corners=True)
    if act:
        y = torch.relu(y)
    cot = rnd(B, C, no, nq, dev="cpu", seed=2)
    y.backward(cot)
    xin = x.detach().float()
    xin = (xin.permute(0, 2, 3, 1) if in_nhwc else xin).contiguous().to(gpu_device)
    out = H.bilinear2d_fwd(xin, (no, nq), in_nhwc, out_nhwc, act)
    got = out.permute(0, 3, 1, 2) if out_nhwc else out
    assert rel_l2(got, y) < KTOL
    g = cot.float()
    g = (g.permute(0, 2, 3, 1) if out_nhwc else g).contiguous().to(gpu_device)
    dx = H.bilinear2d_bwd(g, out if act else None, (ni, nj), in_nhwc, out_nhwc, act)
    dgot = dx.permute(0, 3, 1, 2) if in_nhwc else dx
    assert rel_l2(dgot, x.grad) < KTOL
    dx2 = H.bilinear2d_bwd(g, out if act else None, (ni, nj), in_nhwc, out_nhwc, act)
    assert torch.equal(dx, dx2)                         # gather formulation: bitwise deterministic


@pytest.mark.parametrize("rp", [0, 1, 2, 3])
def test_bilinear_resize_affine(H, gpu_device, rp):
    """gt_bilinear2d_fwd_affine, channels-last on both sides, against interpolate + bias + rp_a @ rp_b^T on the CPU in fp32.
    The kernel carries rp = 1 and 2 in registers; rp = 3 is the only route into the general loop (resize_affine)."""
    import torch.nn.functional as F
    B, C, Hi, Wi, Ho, Wo = 2, 8, 5, 6, 9, 11
    x, bias = rnd(B, C, Hi, Wi, dev="cpu", seed=5), rnd(C, dev="cpu", seed=6)
    ref = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1) + bias
    rp_a = rp_b = None
    if rp:
        rp_a, rp_b = rnd(B, Ho, Wo, rp, dev="cpu", seed=7), rnd(C, rp, dev="cpu", seed=8)
        ref = ref + rp_a @ rp_b.t()
        rp_a, rp_b = rp_a.to(gpu_device), rp_b.to(gpu_device)
    out = H.bilinear2d_fwd(x.permute(0, 2, 3, 1).contiguous().to(gpu_device), (Ho, Wo), True, True, H.ACT_NONE,
                           bias=bias.to(gpu_device), rp_a=rp_a, rp_b=rp_b, rp_ldb=rp)
    assert tuple(out.shape) == (B, Ho, Wo, C)
    assert rel_l2(out, ref) < KTOL


def test_bilinear_resize_autograd_scale_factor(H, gpu_device):
    """ops.bilinear_resize with the reference's float scale factor (recompute_scale_factor=True)."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    x = rnd(2, 16, 141, 141, dev="cpu", seed=3).requires_grad_(True)
    ref = F.interpolate(x, scale_factor=0.555, mode="bilinear", recompute_scale_factor=True,
                        align_corners=True)
    cot = rnd(*ref.shape, dev="cpu", seed=4)
    (gref,) = torch.autograd.grad(ref, x, cot)
    xg = x.detach().to(gpu_device).requires_grad_(True)
    y = ops.bilinear_resize(xg, 0.555)
    assert tuple(y.shape) == tuple(ref.shape) == (2, 16, 78, 78)
    y.backward(cot.to(gpu_device))
    assert rel_l2(y, ref) < KTOL and rel_l2(xg.grad, gref) < KTOL
    with pytest.raises(NotImplementedError):
        ops.bilinear_resize(torch.zeros(1, 6, 6, 3, device=gpu_device), (4, 4), in_nhwc=True)


@pytest.mark.parametrize("N", [144, 192, 160 + 128])
@pytest.mark.parametrize("lb", [0, 1])
def test_gemm_width_remainder_split(H, gpu_device, N, lb):
    """Widths just above a multiple of 128 run as two launches (aligned part + narrow remainder): every
    epilogue term (bias, rank update, add, pre, aux, dropout index, residual) must follow the column
    offset.  144 = h*(d_k+p) of the Darcy model.  The library splits only when the aligned part alone fills
    the chip (>= 512 tiles of 128 rows): M = 333 is the one-launch form of the same call, M = 65536 + 37 the
    split one -- asserted from gt_gemm_plan, so that the second shape cannot quietly stop splitting."""
    import ctypes as C
    dev = gpu_device
    for M in (333, 65536 + 37):
        H.set_seed(4321, dev)
        K, p = 136, 2
        dsc = H._new_desc()
        prec = None if M == 333 else "f16x2"     # (the suite's default mode; named so that the split does not hang on it)
        dsc.M, dsc.N, dsc.K, dsc.layout_b, dsc.precision = M, N, K, lb, H.PREC_CODE[prec or H.get_precision()]
        bm, bn = C.c_int32(), C.c_int32()
        H.check(H.lib().gt_gemm_plan(C.byref(dsc), C.byref(bm), C.byref(bn), None), "gt_gemm_plan")
        splits = bn.value == 128 and -(-M // bm.value) * (N // 128) >= 512
        assert splits == (M > 333), (M, bm.value, bn.value)
        A = rnd(M, K, dev=dev, seed=30)
        Bm = rnd(N, K + p, dev=dev, seed=31, scale=0.3) if lb == 0 else rnd(K, N, dev=dev, seed=31, scale=0.3)
        bias, ea = rnd(N, dev=dev, seed=32), rnd(M, p, dev=dev, seed=33)
        eb = rnd(N, p, dev=dev, seed=34)
        add, aux, res = rnd(M, N, dev=dev, seed=35), rnd(M, N, dev=dev, seed=36), rnd(M, N, dev=dev, seed=37)
        d = H.dropout_desc(0.25, salt=5, device=dev)
        mask = H.dropout_apply(torch.ones(M * N, device=dev), d).reshape(M, N).double()
        Cc, pre = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        H.gemm(A, Bm, Cc, M, N, K, layout_b=lb, lda=K, ldb=(K + p if lb == 0 else N), ldc=N, bias=bias, rp=p, rp_a=ea,
               rp_lda=p, rp_b=eb, rp_ldb=p, add=add, ldadd=N, pre=pre, ldpre=N, act=H.ACT_SILU, aux_op=H.AUX_MUL,
               aux=aux, ldaux=N, aux_scale=0.5, drop=d, res=res, ldr=N, out_scale=-1.0, precision=prec)
        torch.cuda.synchronize()
        Bk = Bm[:, :K].double().t() if lb == 0 else Bm.double()
        p64 = A.double() @ Bk + bias.double() + ea.double() @ eb.double().t() + add.double()
        assert rel_l2(pre, p64) < KTOL
        ref = res.double() - torch.nn.functional.silu(p64) * aux.double() * 0.5 * mask
        assert rel_l2(Cc, ref) < KTOL


@pytest.mark.parametrize("split,batch,p_drop,sign", [(1, 1, 0.0, 1.0), (0, 1, 0.0, -1.0), (7, 1, 0.3, -1.0),
                                                     (1, 5, 0.3, 1.0), (0, 3, 0.0, -1.0)])
def test_gemm_a_colsum_byproduct(H, gpu_device, split, batch, p_drop, sign):
    """Bias gradient as a by-product of the weight-gradient GEMM: a_colsum[m] = sum_{z,k} A_z(m,k)*keep,
    through split-K, batching, the dropout prologue and the sign convention of gt_colsum."""
    dev = gpu_device
    H.set_seed(99, dev)
    Kt, M, N = 2500, 200, 72
    G = rnd(batch, Kt, M, dev=dev, seed=40)
    X = rnd(batch, Kt, N, dev=dev, seed=41)
    d = H.dropout_desc(p_drop, salt=9, device=dev) if p_drop > 0 else None
    mask = (H.dropout_apply(torch.ones(batch * Kt * M, device=dev), d).reshape(batch, Kt, M).double()
            if d is not None else torch.ones(batch, Kt, M, dtype=torch.float64, device=dev))
    Cc = torch.empty(batch, M, N, device=dev)
    cs = torch.empty(M, device=dev)
    H.gemm(G, X, Cc, M, N, Kt, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, batch=(batch, 1),
           a_bs=(Kt * M, 0), b_bs=(Kt * N, 0), c_bs=(M * N, 0), split_k=split, a_drop=d, a_drop_sign=sign,
           a_drop_ld=M, a_drop_bstride=Kt * M, alpha=(sign if d is None else 1.0), a_colsum=cs)
    torch.cuda.synchronize()
    Gm = sign * G.double() * mask
    assert rel_l2(Cc, Gm.transpose(1, 2) @ X.double()) < KTOL
    assert rel_l2(cs, Gm.sum((0, 1))) < KTOL


def test_upsample_fc_commutes(H, gpu_device):
    """ops.upsample_fc == fc(cat[F.interpolate(x), grid]) (reference order, fp64 on the CPU), outputs and all
    gradients: the pointwise Linear commutes with the bilinear resize."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    B, K, Hi, Ho, N, p = 3, 24, 13, 29, 16, 2
    x = rnd(B, K, Hi, Hi, dev="cpu", seed=50).double().requires_grad_(True)
    W = rnd(N, K + p, dev="cpu", seed=51, scale=0.3).double().requires_grad_(True)
    b = rnd(N, dev="cpu", seed=52).double().requires_grad_(True)
    grid = rnd(B, Ho, Ho, p, dev="cpu", seed=53).double()
    up = F.interpolate(x, size=(Ho, Ho), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    ref = F.linear(torch.cat([up, grid], -1), W, b)
    cot = rnd(*ref.shape, dev="cpu", seed=54).double()
    gx, gW, gb = torch.autograd.grad(ref, (x, W, b), cot)
    xg = x.detach().float().to(gpu_device).requires_grad_(True)
    Wg = W.detach().float().to(gpu_device).requires_grad_(True)
    bg = b.detach().float().to(gpu_device).requires_grad_(True)
    out = ops.upsample_fc(xg, (Ho, Ho), Wg, bg, grid.float().to(gpu_device))
    out.backward(cot.float().to(gpu_device))
    assert rel_l2(out, ref) < 5e-6          # fp32 resize weights vs the fp64 reference (see the resize test)
    assert rel_l2(xg.grad, gx) < 5e-6 and rel_l2(Wg.grad, gW) < 5e-6 and rel_l2(bg.grad, gb) < 5e-6


@pytest.mark.parametrize("B,Cin,Cout,n,size,p_drop", [(2, 1, 40, 29, (16, 16), 0.0), (2, 1, 128, 57, 0.555, 0.1),
                                                      (1, 3, 20, 9, (25, 21), 0.2), (2, 2, 8, 6, (1, 4), 0.0)])
def test_conv3x3_resize_fused_equals_unfused(H, gpu_device, B, Cin, Cout, n, size, p_drop):
    """gt_conv3x3_resize_fwd/bwd == conv2d -> stateless dropout -> relu -> HIP resize(+relu) with the same
    seed/salt (identical masks), output and weight gradient; p=0 case also against torch on the CPU."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    dev = gpu_device
    x = rnd(B, Cin, n, n + 2, dev=dev, seed=60)
    w = rnd(Cout, Cin, 3, 3, dev=dev, seed=61, scale=0.5)
    outs = []
    for fused in (True, False):
        H.set_seed(777, dev)
        H._salt[0] = 11
        wg = w.clone().requires_grad_(True)
        if fused:
            y = ops.conv3x3_resize(x, wg, size, p_drop, True)
        else:
            y0 = torch.relu(ops.dropout(F.conv2d(x, wg, padding=1), p_drop, True))
            y = ops.bilinear_resize(y0, size, act="relu")
        cot = rnd(*y.shape, dev=dev, seed=62)
        y.backward(cot)
        outs.append((y.detach(), wg.grad.detach()))
    assert rel_l2(outs[0][0], outs[1][0]) < KTOL and rel_l2(outs[0][1], outs[1][1]) < 1e-5
    if p_drop == 0.0:
        xc, wc = x.cpu().double(), w.cpu().double().requires_grad_(True)
        hw = outs[0][0].shape[2:]
        ref = torch.relu(F.interpolate(torch.relu(F.conv2d(xc, wc, padding=1)), size=tuple(hw), mode="bilinear",
                                       align_corners=True))
        (gw,) = torch.autograd.grad(ref, wc, rnd(*ref.shape, dev="cpu", seed=62).double())
        assert rel_l2(outs[0][0], ref) < 1e-5 and rel_l2(outs[0][1], gw) < 1e-5


@pytest.mark.parametrize("T,K,N,no,act", [(1000, 32, 128, 1, "silu"), (777, 20, 96, 3, "relu"), (130, 48, 48, 1, "silu"),
                                          (70003, 32, 128, 1, "silu"), (33, 32, 128, 1, "relu"), (5, 32, 128, 1, "silu"),
                                          (20000, 32, 128, 1, "none")])
def test_mlp_head_fused(H, gpu_device, T, K, N, no, act):
    """ops.mlp_head (row-dot epilogue forward, recompute + by-product backward) against fp64 torch."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    x = rnd(T, K, dev="cpu", seed=70).double().requires_grad_(True)
    w1 = rnd(N, K, dev="cpu", seed=71, scale=0.3).double().requires_grad_(True)
    b1 = rnd(N, dev="cpu", seed=72).double().requires_grad_(True)
    w2 = rnd(no, N, dev="cpu", seed=73, scale=0.3).double().requires_grad_(True)
    b2 = rnd(no, dev="cpu", seed=74).double().requires_grad_(True)
    fn = F.silu if act == "silu" else (torch.relu if act == "relu" else (lambda v: v))
    ref = F.linear(fn(F.linear(x, w1, b1)), w2, b2)
    cot = rnd(T, no, dev="cpu", seed=75).double()
    grads = torch.autograd.grad(ref, (x, w1, b1, w2, b2), cot)
    dev = gpu_device
    ins = [t.detach().float().to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    out = ops.mlp_head(*ins, act=act)
    out.backward(cot.float().to(dev))
    assert rel_l2(out, ref) < KTOL
    for t, gref in zip(ins, grads):
        assert rel_l2(t.grad, gref) < 5e-6


@pytest.mark.parametrize("la,lb", [(0, 0), (0, 1), (1, 1)])
def test_gemm_second_product(H, gpu_device, la, lb):
    """C = act(A1 B1 + A2 B2 + bias) in one launch (K2 segment), batched, ragged K1 / K2."""
    dev = gpu_device
    nb, M, N, K1, K2 = 3, 141, 32, 24, 20
    A1 = rnd(nb, *((M, K1) if la == 0 else (K1, M)), dev=dev, seed=80)
    A2 = rnd(nb, *((M, K2) if la == 0 else (K2, M)), dev=dev, seed=81)
    B1 = rnd(nb, *((N, K1) if lb == 0 else (K1, N)), dev=dev, seed=82)
    B2 = rnd(*((N, K2) if lb == 0 else (K2, N)), dev=dev, seed=83)          # shared across the batch
    bias = rnd(N, dev=dev, seed=84)
    Cc = torch.empty(nb, M, N, device=dev)
    H.gemm(A1, B1, Cc, M, N, K1, layout_a=la, layout_b=lb, lda=A1.shape[2], ldb=B1.shape[2], ldc=N, batch=(nb, 1),
           a_bs=(A1.shape[1] * A1.shape[2], 0), b_bs=(B1.shape[1] * B1.shape[2], 0), c_bs=(M * N, 0), bias=bias,
           act=H.ACT_RELU, K2=K2, A2=A2, lda2=A2.shape[2], a2_bs=(A2.shape[1] * A2.shape[2], 0), B2=B2,
           ldb2=B2.shape[1])
    torch.cuda.synchronize()
    ref = torch.relu(ref_mm(A1, B1, la, lb) + ref_mm(A2, B2.expand(nb, *B2.shape), la, lb) + bias.double())
    assert rel_l2(Cc, ref) < KTOL


@pytest.mark.parametrize("la,lb,M,N,K", [(0, 0, 4096 + 40, 256, 256), (0, 1, 8192, 128, 384), (1, 1, 384, 128, 40000)])
def test_gemm_stream_many_tiles_per_block(H, gpu_device, la, lb, M, N, K, monkeypatch):
    """Streamed kernel with a tiny persistent grid, so that every block walks many tiles back to back: exercises
    the cross-tile prefetch and the counted s_waitcnt after full-tile epilogues (edge tiles take the full wait)."""
    monkeypatch.setenv("GT_GEMM_BLOCKS", "16")
    A = rnd(*((M, K) if la == 0 else (K, M)), dev=gpu_device, seed=90)
    B = rnd(*((N, K) if lb == 0 else (K, N)), dev=gpu_device, seed=91)
    bias, res = rnd(N, dev=gpu_device, seed=92), rnd(M, N, dev=gpu_device, seed=93)
    ref = ref_mm(A, B, la, lb) + bias.double() + res.double()
    for _ in range(3):                                 # repeat: a race would not reproduce identically
        Cc = torch.empty(M, N, device=gpu_device)
        split = 0 if la == 1 else 1
        if split == 0:
            H.gemm(A, B, Cc, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1], ldb=B.shape[1], ldc=N, split_k=0)
            torch.cuda.synchronize()
            assert rel_l2(Cc, ref_mm(A, B, la, lb)) < KTOL
        else:
            H.gemm(A, B, Cc, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1], ldb=B.shape[1], ldc=N, bias=bias,
                   res=res, ldr=N)
            torch.cuda.synchronize()
            assert rel_l2(Cc, ref) < KTOL


@pytest.mark.parametrize("B,n,d,h,p", [(2, 200, 128, 4, 2), (1, 77, 64, 4, 2), (2, 131, 96, 2, 2)])
@pytest.mark.parametrize("mode", ["off", "reference"])
def test_fourier_fused_equals_materialised(H, gpu_device, B, n, d, h, p, mode):
    """gt_fourier_attn (no n x n matrix in HBM) == the materialising GEMM path of the same operator: outputs and
    every gradient, with the attention dropout off and with the reference's p = 0.5 mask (same seed and salt =>
    the fused kernel regenerates exactly the mask the GEMM epilogue draws)."""
    from galerkin_transformer import ops
    import galerkin_transformer as gt
    dev = gpu_device
    torch.manual_seed(1)
    attn = gt.SimpleAttention(h, d, pos_dim=p, attention_type="fourier", norm=True, eps=1e-7, dropout=0.0).to(dev)
    with torch.no_grad():
        for prm in attn.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    x0 = torch.randn(B, n, d, device=dev)
    pos = torch.rand(B, n, p, device=dev)
    cot = torch.randn(B, n, d, device=dev)
    res = []
    gt.set_attention_dropout(mode)
    try:
        for need_w in (True, False):
            H.set_seed(4242, dev)
            H._salt[0] = 3
            for prm in attn.parameters():
                prm.grad = None
            x = x0.clone().requires_grad_(True)
            y, w = attn.fused_forward(x, pos, residual=x, need_weights=need_w)
            assert (w is None) == (not need_w)
            y.backward(cot)
            res.append([y.detach(), x.grad.detach()] + [prm.grad.detach().clone() for prm in attn.parameters()])
    finally:
        gt.set_attention_dropout("reference")
    for a, b_ in zip(*res):
        assert rel_l2(b_, a) < 5e-6


@pytest.mark.parametrize("nb,n,P", [(37, 141, 24), (1500, 141, 24), (700, 211, 24), (9, 64, 32), (1, 30, 8), (523, 99, 20)])
def test_dft_line_stages(H, gpu_device, nb, n, P):
    """gt_dft_analysis / gt_dft_synthesis (persistent per-grid-line kernels, direct-to-LDS prefetch, clamped
    edges) against fp64 einsums; more lines than resident blocks so every block walks several lines."""
    dev = gpu_device
    C = 32
    assert H.dft_supported(n, P, C, C)
    g = torch.Generator().manual_seed(nb * 1000 + n)
    F = torch.randn(n, P, generator=g).to(dev)
    X = torch.randn(nb, n, C, generator=g).to(dev)
    Y = torch.full((nb, P, C), float("nan"), device=dev)
    H.dft_analysis(F, X, Y, nb, n, P, C)
    ref = torch.einsum("rp,brc->bpc", F.double(), X.double())
    assert rel_l2(Y, ref) < 2e-6
    Z = torch.randn(nb, P, C, generator=g).to(dev)
    W2 = (torch.randn(C, C, generator=g) / 6).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    lin = torch.einsum("rp,bpc->brc", F.double(), Z.double()) + X.double() @ W2.double()
    for act, b_, want_pre in ((H.ACT_NONE, None, False), (H.ACT_CODE["silu"], bias, True), (H.ACT_CODE["relu"], bias, False)):
        out = torch.full((nb, n, C), float("nan"), device=dev)
        pre = torch.full((nb, n, C), float("nan"), device=dev) if want_pre else None
        H.dft_synthesis(F, Z, out, nb, n, P, C, X, W2, C, bias=b_, act=act, pre=pre)
        r = lin + (b_.double() if b_ is not None else 0.0)
        if want_pre:
            assert rel_l2(pre, r) < 2e-6
        if act == H.ACT_CODE["silu"]:
            r = torch.nn.functional.silu(r)
        elif act == H.ACT_CODE["relu"]:
            r = torch.relu(r)
        assert rel_l2(out, r) < 2e-6


def test_dft_line_stages_unsupported_shapes_fall_back(H, gpu_device):
    """Channel counts other than 32 are GT_ENOTSUP at the C ABI; SpectralConv2d routes them through gt_gemm."""
    dev = gpu_device
    assert not H.dft_supported(64, 24, 20, 20)
    F = torch.randn(64, 24, device=dev)
    X = torch.randn(4, 64, 20, device=dev)
    with pytest.raises(H.GtNotSupported):
        H.dft_analysis(F, X, torch.empty(4, 24, 20, device=dev), 4, 64, 24, 20)


@pytest.mark.parametrize("M,N,K,sign,colsum", [(32, 2, 100003, 1.0, False), (32, 32, 131077, -1.0, True),
                                               (128, 32, 70000, 1.0, True), (64, 16, 65536, 1.0, True),
                                               (96, 32, 65540, -1.0, False)])
def test_gemm_tall_skinny_wgrad(H, gpu_device, M, N, K, sign, colsum):
    """gt_gemm routes C = A^T B with K in the 1e5+ range and M <= 128, N <= 32 (the decoder's pointwise-layer
    weight gradients) to the streaming tsmm kernel: same results as the tiled split-K path and as fp64, with
    the bias-gradient by-product, ragged K tails and the sign convention of a_colsum."""
    dev = gpu_device
    A = rnd(K, M, dev=dev, seed=50)
    Bm = rnd(K, N, dev=dev, seed=51)
    name = H.gemm_kernel_name(A, Bm, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=0)
    assert "tsmm_kernel" in name
    Cc = torch.full((M, N), float("nan"), device=dev)
    cs = torch.full((M,), float("nan"), device=dev) if colsum else None
    H.gemm(A, Bm, Cc, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=0, alpha=sign,
           a_drop_sign=sign, a_colsum=cs)
    torch.cuda.synchronize()
    ref = sign * (A.double().t() @ Bm.double())
    assert rel_l2(Cc, ref) < KTOL
    if colsum:
        assert rel_l2(cs, sign * A.double().sum(0)) < KTOL


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
def test_silu_gate_on_the_store_of_the_gradient_kernels(H, gpu_device, prec):
    """ABI v21: gt_dft_synthesis_gated / gt_mlp_head_bwd_gated multiply the gradient they form by silu'(gate) on their own
    store -- bit for bit the ungated kernel followed by gt_act_bwd (which the SpectralConv2d in front of them then skips)."""
    dev = gpu_device
    nb, n, P, C = 300, 141, 24, 32
    g = torch.Generator().manual_seed(77)
    F = torch.randn(n, P, generator=g).to(dev)
    Z = torch.randn(nb, P, C, generator=g).to(dev)
    X = torch.randn(nb, n, C, generator=g).to(dev)
    W2 = (torch.randn(C, C, generator=g) / 6).to(dev)
    gate = (2.0 * torch.randn(nb, n, C, generator=g)).to(dev)
    plain = torch.full((nb, n, C), float("nan"), device=dev)
    gated = torch.full((nb, n, C), float("nan"), device=dev)
    H.dft_synthesis(F, Z, plain, nb, n, P, C, X, W2, C)
    H.dft_synthesis(F, Z, gated, nb, n, P, C, X, W2, C, out_gate=gate)
    assert torch.equal(gated, H.act_bwd(plain, gate, H.ACT_SILU))
    gd = gate.double()
    sg = torch.sigmoid(gd)
    assert rel_l2(gated, plain.double() * sg * (1 + gd * (1 - sg))) < 2e-6
    with pytest.raises(H.GtError):                  # a gate and an activation of its own do not go together
        H.dft_synthesis(F, Z, gated, nb, n, P, C, X, W2, C, act=H.ACT_SILU, out_gate=gate)
    T = 4099
    x = rnd(T, 32, dev=dev, seed=80)
    w1, b1 = rnd(128, 32, dev=dev, seed=81, scale=0.3), rnd(128, dev=dev, seed=84, scale=0.3)
    w2 = rnd(1, 128, dev=dev, seed=82, scale=0.3)
    gy = rnd(T, 1, dev=dev, seed=83)
    hg = 2.0 * rnd(T, 32, dev=dev, seed=85)
    outs = []
    for dx_gate in (None, hg):
        dx = torch.full((T, 32), float("nan"), device=dev)
        dw1, db1 = torch.full((128, 32), float("nan"), device=dev), torch.full((128,), float("nan"), device=dev)
        dw2 = torch.full((1, 128), float("nan"), device=dev)
        H.mlp_head_bwd(x, w1, b1, w2, H.ACT_SILU, gy, dx, dw1, db1, dw2, None, precision=prec, dx_gate=dx_gate)
        outs.append((dx, dw1, db1, dw2))
    assert torch.equal(outs[1][0], H.act_bwd(outs[0][0], hg, H.ACT_SILU))
    for a, b_ in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b_)


def test_mlp_head_dedicated_kernels_without_optional_outputs(H, gpu_device):
    """gt_mlp_head_fwd / gt_mlp_head_bwd with no biases and no input gradient (the x.requires_grad == False
    case), against the GEMM-epilogue implementation of the same head."""
    dev = gpu_device
    T = 4099
    x = rnd(T, 32, dev=dev, seed=80)
    w1 = rnd(128, 32, dev=dev, seed=81, scale=0.3)
    w2 = rnd(1, 128, dev=dev, seed=82, scale=0.3)
    g = rnd(T, 1, dev=dev, seed=83)
    assert H.mlp_head_supported(32, 128, 1)
    out = torch.full((T, 1), float("nan"), device=dev)
    H.mlp_head_fwd(x, w1, None, w2, None, H.ACT_SILU, out)
    h = torch.nn.functional.silu(x.double() @ w1.double().t())
    assert rel_l2(out, h @ w2.double().t()) < KTOL
    dw1 = torch.full((128, 32), float("nan"), device=dev)
    dw2 = torch.full((1, 128), float("nan"), device=dev)
    H.mlp_head_bwd(x, w1, None, w2, H.ACT_SILU, g, None, dw1, None, dw2, None)
    xd = x.double().requires_grad_(False)
    w1d, w2d = w1.double().requires_grad_(True), w2.double().requires_grad_(True)
    ref = torch.nn.functional.silu(xd @ w1d.t()) @ w2d.t()
    gw1, gw2 = torch.autograd.grad(ref, (w1d, w2d), g.double())
    assert rel_l2(dw1, gw1) < 5e-6
    assert rel_l2(dw2, gw2) < 5e-6


@pytest.mark.parametrize("act", ["silu", "relu"])
@pytest.mark.parametrize("prec", ["f16x2", "f32"])
def test_mlp_head_dynamic_range_and_arithmetic(H, gpu_device, act, prec):
    """gt_mlp_head_* in both arithmetics (f16x2: two fp16 terms per operand with per-row / per-tensor / running exponents,
    gt_head.hip; f32: the fp32-MFMA kernels) on data built to stress the fp16 exponents: row magnitudes of x spanning 1e-3 ..
    1e3, all-zero rows, gradients of 1e-9 next to gradients of 1, rows without gradient, T not a multiple of 32.  Every
    output against fp64; dX additionally ROW BY ROW (a per-row exponent must keep the rows with tiny gradients exact)."""
    import torch.nn.functional as F
    dev = gpu_device
    T = 4099
    g_ = torch.Generator().manual_seed(321)
    x = torch.randn(T, 32, generator=g_) * torch.logspace(-3, 3, T).unsqueeze(1)[torch.randperm(T, generator=g_)]
    x[100:140] = 0.0
    w1 = torch.randn(128, 32, generator=g_) * 0.05
    w1[7] *= 1e-4                                                   # a hidden unit far below the tensor's scale
    b1 = torch.randn(128, generator=g_) * 0.5
    w2 = torch.randn(1, 128, generator=g_) * 0.3
    b2 = torch.randn(1, generator=g_)
    cot = torch.randn(T, 1, generator=g_)
    cot[: T // 2] *= 1e-9
    cot[2000:2100] = 0.0
    fn = F.silu if act == "silu" else torch.relu
    xd, w1d, b1d, w2d, b2d = (t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2))
    ref = F.linear(fn(F.linear(xd, w1d, b1d)), w2d, b2d)
    grads = torch.autograd.grad(ref, (xd, w1d, b1d, w2d, b2d), cot.double())
    xg, w1g, b1g, w2g, b2g, cg = (t.to(dev) for t in (x, w1, b1, w2, b2, cot))
    code = H.ACT_CODE[act]
    out = torch.full((T, 1), float("nan"), device=dev)
    H.mlp_head_fwd(xg, w1g, b1g, w2g, b2g, code, out, precision=prec)
    assert rel_l2(out, ref) < KTOL
    res = []
    for _ in range(2):
        dx = torch.full((T, 32), float("nan"), device=dev)
        dw1, db1 = torch.full((128, 32), float("nan"), device=dev), torch.full((128,), float("nan"), device=dev)
        dw2, db2 = torch.full((1, 128), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
        H.mlp_head_bwd(xg, w1g, b1g, w2g, code, cg, dx, dw1, db1, dw2, db2, precision=prec)
        torch.cuda.synchronize()
        res.append((dx, dw1, db1, dw2, db2))
    for a, b in zip(*res):
        assert torch.equal(a, b)                                    # fixed-order reductions: bitwise repeatable
    for got, want, name in zip(res[0], grads, ("dx", "dw1", "db1", "dw2", "db2")):
        assert rel_l2(got, want) < 5e-6, (name, rel_l2(got, want))
    dxr, dxw = res[0][0].double().cpu(), grads[0]
    nrm = dxw.norm(dim=1)
    rows = nrm > 0
    err = ((dxr - dxw).norm(dim=1)[rows] / nrm[rows]).max().item()
    assert err < 2e-5, err
    assert float(dxr[~rows].abs().max()) == 0.0


def test_gemm_tall_skinny_wgrad_into_column_slice(H, gpu_device):
    """The tsmm path writes through ldc (the grid columns of SpectralRegressor.fc's weight gradient are a column
    slice of the [N, K + p] weight) and leaves the other columns alone."""
    dev = gpu_device
    M, N, K, ld = 32, 2, 70001, 34
    A = rnd(K, M, dev=dev, seed=60)
    Bm = rnd(K, N, dev=dev, seed=61)
    W = torch.full((M, ld), 7.0, device=dev)
    cs = torch.empty(M, device=dev)
    Cv = W[:, ld - N:]
    H.gemm(A, Bm, Cv, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=ld, split_k=0, a_colsum=cs)
    torch.cuda.synchronize()
    assert rel_l2(W[:, ld - N:], A.double().t() @ Bm.double()) < KTOL
    assert torch.all(W[:, :ld - N] == 7.0)
    assert rel_l2(cs, A.double().sum(0)) < KTOL


def test_gelu_is_elementwise_only(H, gpu_device):
    """GT_ACT_GELU (erf GELU, reference layers.py:968-969) lives in gt_dropact_* -- value and derivative against float64 --
    and every GEMM epilogue refuses it instead of silently running the identity."""
    from galerkin_transformer import ops
    dev = gpu_device
    x = (3.0 * rnd(50001, dev=dev, seed=5)).requires_grad_(True)
    cot = rnd(50001, dev=dev, seed=6)
    y = ops.drop_act(x, 0.0, "gelu")
    y.backward(cot)
    xd = x.detach().double().requires_grad_(True)
    yd = torch.nn.functional.gelu(xd)
    yd.backward(cot.double())
    assert rel_l2(y, yd) < 1e-6 and rel_l2(x.grad, xd.grad) < 1e-6
    A, W, C = rnd(64, 32, dev=dev, seed=7), rnd(48, 32, dev=dev, seed=8), torch.empty(64, 48, device=dev)
    with pytest.raises(Exception):
        H.gemm(A, W, C, 64, 48, 32, lda=32, ldb=32, ldc=48, act=H.ACT_GELU)


@pytest.mark.parametrize("n", [4096 * 3 + 1, 64 * 77 * 77])
@pytest.mark.parametrize("p1,a1,p2,a2", [(0.1, "relu", 0.0, "none"), (0.05, "silu", 0.05, "silu"), (0.0, "silu", 0.3, "relu"),
                                         (0.0, "none", 0.0, "silu"), (0.0, "gelu", 0.2, "none")])
def test_drop_act_fused_equals_chain(H, gpu_device, n, p1, a1, p2, a2):
    """ops.drop_act == activation(dropout(activation(dropout(x)))) built from the separate operators with the same
    seed and salts (identical masks), forward and backward; also in eval mode."""
    from galerkin_transformer import ops
    import torch.nn.functional as F
    dev = gpu_device
    act = {"relu": torch.relu, "silu": F.silu, "gelu": F.gelu, "none": lambda v: v}
    x0 = rnd(n, dev=dev, seed=90)
    cot = rnd(n, dev=dev, seed=91)
    for training in (True, False):
        res = []
        for fused in (True, False):
            H.set_seed(77, dev)
            H._salt[0] = 11
            x = x0.clone().requires_grad_(True)
            if fused:
                y = ops.drop_act(x, p1, a1, training, p2, a2)
            else:
                y = act[a2](ops.dropout(act[a1](ops.dropout(x, p1, training)), p2, training))
            y.backward(cot)
            res.append((y.detach(), x.grad.detach()))
        assert rel_l2(res[0][0], res[1][0]) < 1e-6
        assert rel_l2(res[0][1], res[1][1]) < 1e-6
    if p1 > 0:
        kept = (ops.drop_act(torch.ones(n, device=dev), p1, "none") != 0).float().mean().item()
        assert abs(kept - (1 - p1)) < 0.02


@pytest.mark.parametrize("B,n,h,DP", [(2, 100, 4, 36), (1, 37, 2, 20), (3, 1849, 4, 36), (1, 64, 1, 52)])
def test_galerkin_dkv(H, gpu_device, B, n, h, DP):
    """gt_galerkin_dkv against fp64 (and thereby against the two batched GEMMs it would replace)."""
    dev = gpu_device
    Kp = rnd(B * n, h, DP, dev=dev, seed=100)
    Vp = rnd(B * n, h, DP, dev=dev, seed=101)
    dM = rnd(B, h, DP, DP, dev=dev, seed=102)
    dK = torch.full_like(Kp, float("nan"))
    dV = torch.full_like(Kp, float("nan"))
    H.galerkin_dkv(Kp, Vp, dM, dK, dV, B, n, h, DP)
    K4, V4 = Kp.reshape(B, n, h, DP).double(), Vp.reshape(B, n, h, DP).double()
    assert rel_l2(dK.reshape(B, n, h, DP), torch.einsum("bnhk,bhck->bnhc", V4, dM.double())) < KTOL
    assert rel_l2(dV.reshape(B, n, h, DP), torch.einsum("bnhk,bhkc->bnhc", K4, dM.double())) < KTOL


# ----------------------------------------------------------------------------- split-operand bf16 kernel
X3_TOL = {"f32": 2e-6, "bf16x3": 2e-6, "bf16x2": 2e-4, "bf16": 2e-2}


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x2", "bf16"])
@pytest.mark.parametrize("la,lb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (128, 128, 16), (1000, 256, 130), (257, 131, 77), (96, 200, 1849)])
def test_gemm_x3_layouts(H, gpu_device, prec, la, lb, M, N, K):
    """gemm_x3_kernel (fp32 operands split into bf16 planes, fp32 accumulate) against fp64: every layout, ragged
    edges in M, N and K, unaligned leading dimensions (scalar loader path)."""
    dev = gpu_device
    A = rnd(M, K, dev=dev, seed=201) if la == 0 else rnd(K, M, dev=dev, seed=201)
    B = rnd(N, K, dev=dev, seed=202) if lb == 0 else rnd(K, N, dev=dev, seed=202)
    assert "gemm_x3" in H.gemm_kernel_name(A, B, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1],
                                                  ldb=B.shape[1], ldc=N, precision=prec)
    Cc = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, B, Cc, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1], ldb=B.shape[1], ldc=N, precision=prec)
    torch.cuda.synchronize()
    assert rel_l2(Cc, ref_mm(A, B, la, lb)) < X3_TOL[prec]


def test_gemm_x3_identity_exact(H, gpu_device):
    """The three-plane split is exact (a = h0 + h1 + h2 bit for bit), so I * B must come back unchanged, and an
    asymmetric B catches a transposed accumulator map of the 32x32 MFMA."""
    dev = gpu_device
    n = 256
    A = torch.eye(n, device=dev)
    B = (torch.arange(n * n, device=dev, dtype=torch.float32).reshape(n, n) % 97) / 7.0 + 1e-3 * rnd(n, n, dev=dev, seed=203)
    Cc = torch.empty(n, n, device=dev)
    H.gemm(A, B, Cc, n, n, n, lda=n, ldb=n, ldc=n, precision="bf16x3")
    torch.cuda.synchronize()
    assert torch.equal(Cc, B.t().contiguous())


def test_gemm_x3_precision_ladder(H, gpu_device):
    """Error against fp64 must fall by ~2^-8 per extra plane: bf16 ~ 3e-3, bf16x2 ~ 1e-5, bf16x3 ~ fp32 MFMA."""
    dev = gpu_device
    M, N, K = 512, 256, 512
    A, B = rnd(M, K, dev=dev, seed=204), rnd(N, K, dev=dev, seed=205)
    ref = ref_mm(A, B, 0, 0)
    err = {}
    for prec in ("f32", "bf16x3", "bf16x2", "bf16"):
        Cc = torch.empty(M, N, device=dev)
        H.gemm(A, B, Cc, M, N, K, lda=K, ldb=K, ldc=N, precision=prec)
        torch.cuda.synchronize()
        err[prec] = rel_l2(Cc, ref)
    print("x3 precision ladder:", err)
    assert err["bf16"] < 1e-2 and err["bf16x2"] < 1e-4 and err["bf16x3"] < 1e-6
    assert err["bf16x3"] < 4 * err["f32"] + 1e-7
    assert err["bf16x2"] < err["bf16"] / 50


@pytest.mark.parametrize("split", [0, 3, 16])
def test_gemm_x3_split_k_colsum(H, gpu_device, split):
    """Weight-gradient use: A^T B with K = tokens, split-K slabs, bias gradient (row sums of A) as a by-product."""
    dev = gpu_device
    M, N, K = 384, 128, 5000
    A, B = rnd(K, M, dev=dev, seed=206), rnd(K, N, dev=dev, seed=207)
    Cc, cs = torch.empty(M, N, device=dev), torch.empty(M, device=dev)
    H.gemm(A, B, Cc, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=split, alpha=0.5, a_colsum=cs,
           precision="bf16x3")
    torch.cuda.synchronize()
    assert rel_l2(Cc, 0.5 * (A.double().t() @ B.double())) < KTOL
    assert rel_l2(cs, A.double().sum(0)) < KTOL


def test_gemm_x3_epilogues_batched(H, gpu_device):
    """Per-sample batched product with bias + dropout + residual + out_scale (the Galerkin Q'P launch), and the
    FFN input-gradient epilogue (aux > 0 mask), on the split kernel; same seed => the mask of the fp32 kernel."""
    dev = gpu_device
    Bn, n, hD, d = 3, 700, 144, 128
    Q, P, b = rnd(Bn, n, hD, dev=dev, seed=208), rnd(Bn, hD, d, dev=dev, seed=209, scale=0.2), rnd(d, dev=dev, seed=210)
    R = rnd(Bn, n, d, dev=dev, seed=211)
    outs = {}
    for prec in ("f32", "bf16x3"):
        out = torch.empty(Bn, n, d, device=dev)
        H.gemm(Q, P, out, n, d, hD, layout_b=1, lda=hD, ldb=d, ldc=d, batch=(Bn, 1), a_bs=(n * hD, 0), b_bs=(hD * d, 0),
               c_bs=(n * d, 0), bias=b, drop=H.dropout_desc(0.3, 77, dev), res=R, ldr=d, r_bs=(n * d, 0), out_scale=-1.0,
               precision=prec)
        outs[prec] = out
    torch.cuda.synchronize()
    assert rel_l2(outs["bf16x3"], outs["f32"]) < KTOL
    plain = torch.empty(Bn, n, d, device=dev)
    H.gemm(Q, P, plain, n, d, hD, layout_b=1, lda=hD, ldb=d, ldc=d, batch=(Bn, 1), a_bs=(n * hD, 0), b_bs=(hD * d, 0),
           c_bs=(n * d, 0), bias=b, precision="bf16x3")
    torch.cuda.synchronize()
    assert rel_l2(plain, torch.einsum("bnk,bkd->bnd", Q.double(), P.double()) + b.double()) < KTOL
    T, f = 1000, 256
    g, W2, hid = rnd(T, d, dev=dev, seed=212), rnd(d, f, dev=dev, seed=213, scale=0.2), rnd(T, f, dev=dev, seed=214)
    gh = torch.empty(T, f, device=dev)
    H.gemm(g, W2, gh, T, f, d, layout_b=1, lda=d, ldb=f, ldc=f, aux_op=H.AUX_GT0, aux=hid, ldaux=f, aux_scale=1.25,
           precision="bf16x3")
    torch.cuda.synchronize()
    assert rel_l2(gh, (g.double() @ W2.double()) * (hid.double() > 0) * 1.25) < KTOL


def test_gemm_x3_second_product_width_split(H, gpu_device):
    """Second accumulated product (K2) on a width that gt_gemm splits into 128-aligned part + remainder: the
    remainder launch must read B2's own columns (B2 was not offset)."""
    dev = gpu_device
    M, N, K, K2 = 70000, 160, 48, 32
    A, B = rnd(M, K, dev=dev, seed=215), rnd(K, N, dev=dev, seed=216)
    A2, B2 = rnd(M, K2, dev=dev, seed=217), rnd(K2, N, dev=dev, seed=218)
    ref = A.double() @ B.double() + A2.double() @ B2.double()
    for prec in ("f32", "bf16x3"):
        Cc = torch.full((M, N), float("nan"), device=dev)
        H.gemm(A, B, Cc, M, N, K, layout_b=1, lda=K, ldb=N, ldc=N, K2=K2, A2=A2, lda2=K2, B2=B2, ldb2=N, precision=prec)
        torch.cuda.synchronize()
        assert rel_l2(Cc, ref) < KTOL, prec


def test_gemm_x3_a_dropout_matches_f32_kernel(H, gpu_device):
    dev = gpu_device
    M, N, K = 400, 256, 300
    outs = {}
    for la in (0, 1):
        A = rnd(M, K, dev=dev, seed=219) if la == 0 else rnd(K, M, dev=dev, seed=219)
        B = rnd(N, K, dev=dev, seed=220)
        for prec in ("f32", "bf16x3"):
            Cc = torch.empty(M, N, device=dev)
            H.gemm(A, B, Cc, M, N, K, layout_a=la, lda=A.shape[1], ldb=K, ldc=N, a_drop=H.dropout_desc(0.25, 5, dev),
                   a_drop_sign=-1.0, a_drop_ld=A.shape[1], precision=prec)
            outs[prec] = Cc
        torch.cuda.synchronize()
        assert rel_l2(outs["bf16x3"], outs["f32"]) < KTOL


@pytest.mark.parametrize("T,h,dk,p,mask", [(1000, 4, 32, 2, 0b110), (333, 2, 64, 1, 0b011), (4099, 8, 16, 2, 0b110),
                                           (257, 4, 32, 0, 0b000), (700, 4, 48, 2, 0b110)])
def test_qkv_headnorm_fused_epilogue(H, gpu_device, T, h, dk, p, mask):
    """GT_EP_HEADNORM on the split-operand ring kernel: projection + per-head LayerNorm + position columns in one
    launch == gt_gemm followed by gt_headnorm_fwd (layers.py:838-874).  dk = 48 is outside the ring kernel's fused epilogue
    (it exists on the packed-B kernels from 16 384 token rows, test_qkv_headnorm_head_slots_dk48): below that the library
    must say GT_ENOTSUP (the Python mirror then runs the two launches)."""
    dev = gpu_device
    d = h * dk
    x = rnd(T, d, dev=dev, seed=110)
    w = rnd(3 * d, d, dev=dev, seed=111, scale=0.2)
    b = rnd(3 * d, dev=dev, seed=112)
    gamma = 1 + 0.1 * rnd(2, h, dk, dev=dev, seed=113)
    beta = 0.1 * rnd(2, h, dk, dev=dev, seed=114)
    pos = rnd(T, p, dev=dev, seed=115) if p else None
    eps = 1e-7
    qkv = torch.empty(T, 3 * d, device=dev)
    H.gemm(x, w, qkv, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, precision="bf16x3")
    out_ref, st_ref = H.headnorm_fwd(qkv, pos, gamma, beta, T, h, dk, p, mask, eps)
    DP = H.round4(dk + p)
    qkv2 = torch.full_like(qkv, float("nan"))
    out3 = torch.full((3, T, h, DP), float("nan"), device=dev)
    stats = torch.zeros(2, T, h, 2, device=dev)
    hn = dict(gamma=gamma, beta=beta, pos=pos, out=out3, stats=stats, h=h, dk=dk, p=p, norm_mask=mask, eps=eps)
    if dk not in (16, 32, 64):
        with pytest.raises(NotImplementedError):
            H.gemm(x, w, qkv2, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=hn, precision="bf16x3")
        return
    with pytest.raises(NotImplementedError):           # the fused epilogue lives on the split-operand kernel only
        H.gemm(x, w, qkv2, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=hn, precision="f32")
    H.gemm(x, w, qkv2, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=hn, precision="bf16x3")
    torch.cuda.synchronize()
    assert torch.equal(qkv2, qkv)
    assert not torch.isnan(out3).any()
    # skip_raw: the raw projection of the un-normalised streams is not written (it has no reader in training)
    qkv3 = torch.full_like(qkv, float("nan"))
    out3b = torch.empty_like(out3)
    H.gemm(x, w, qkv3, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=dict(hn, out=out3b, skip_raw=(~mask) & 7),
           precision="bf16x3")
    torch.cuda.synchronize()
    for st in range(3):
        blk = qkv3[:, st * d:(st + 1) * d]
        if (mask >> st) & 1:
            assert torch.equal(blk, qkv[:, st * d:(st + 1) * d])
        else:
            assert torch.isnan(blk).all()
    assert torch.equal(out3b, out3)
    assert rel_l2(out3, out_ref) < 1e-6
    nn = bin(mask).count("1")
    if nn:
        assert rel_l2(stats[:nn], st_ref[:nn]) < 1e-6


@pytest.mark.parametrize("B,Hh,Ww,Cin,Cout", [(3, 13, 11, 128, 128), (1, 77, 77, 96, 144), (2, 5, 40, 112, 96),
                                              (1, 1, 100, 128, 128), (1, 1, 7, 128, 128), (4, 16, 16, 256, 128), (12, 77, 77, 96, 144)])
def test_conv3x3_implicit_gemm(H, gpu_device, B, Hh, Ww, Cin, Cout):
    """ops.conv3x3_nhwc (implicit GEMM on the split-operand ring kernel: forward and data gradient; MIOpen wrw for the
    weight gradient) == F.conv2d(padding=1) in fp64 on the CPU (layers.py:98-100 inside Interp2dUpsample), outputs and
    both gradients.  Shapes cover partial pixel tiles, one-row images (every vertical tap masked) and the N = 144 width
    split; the 7-pixel image is below one tile and takes the library convolution."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    x = rnd(B, Cin, Hh, Ww, dev="cpu", seed=120).double().requires_grad_(True)
    w = rnd(Cout, Cin, 3, 3, dev="cpu", seed=121, scale=0.05).double().requires_grad_(True)
    ref = F.conv2d(x, w, padding=1)
    cot = rnd(*ref.shape, dev="cpu", seed=122).double()
    gx, gw = torch.autograd.grad(ref, (x, w), cot)
    xg = x.detach().float().permute(0, 2, 3, 1).contiguous().to(gpu_device).requires_grad_(True)
    wg = w.detach().float().to(gpu_device).requires_grad_(True)
    y = ops.conv3x3_nhwc(xg, wg)
    y.backward(cot.float().permute(0, 2, 3, 1).contiguous().to(gpu_device))
    torch.cuda.synchronize()
    assert rel_l2(y.permute(0, 3, 1, 2), ref) < KTOL
    assert rel_l2(xg.grad.permute(0, 3, 1, 2), gx) < KTOL
    assert wg.grad.shape == w.shape and wg.grad.is_contiguous()
    assert rel_l2(wg.grad, gw) < (KTOL if Ww >= 16 else 1e-5)   # nine-tap pixel contraction on the ring kernel (Ww >= 16)
    if Ww >= 16:                               # and the library's channels-last wrw kernel (GT_CONV_WGRAD=miopen)
        old = ops._conv_wgrad[0]
        ops._conv_wgrad[0] = False
        try:
            xg.grad = wg.grad = None
            ops.conv3x3_nhwc(xg, wg).backward(cot.float().permute(0, 2, 3, 1).contiguous().to(gpu_device))
        finally:
            ops._conv_wgrad[0] = old
        assert rel_l2(wg.grad, gw) < 1e-5      # own accumulation order


def test_conv3x3_implicit_gemm_rejects_what_it_does_not_cover(H, gpu_device):
    """cv_c must be a multiple of 16, K = 9 cv_c, no split-K / batching, split-operand arithmetic only."""
    dev = gpu_device
    x = rnd(2, 8, 8, 128, dev=dev, seed=130)
    w = rnd(128, 9 * 128, dev=dev, seed=131)
    y = torch.empty(2, 8, 8, 128, device=dev)
    kw = dict(lda=128, ldb=9 * 128, ldc=128)
    with pytest.raises(NotImplementedError):
        H.gemm(x, w, y, 128, 128, 9 * 128, conv=(8, 8, 128), precision="f32", **kw)
    with pytest.raises(NotImplementedError):
        H.gemm(x, w, y, 128, 128, 9 * 128, conv=(8, 8, 128), split_k=2, **kw)
    with pytest.raises(H.GtError, match="EINVAL"):
        H.gemm(x, w, y, 128, 128, 8 * 128, conv=(8, 8, 128), **kw)           # K != 9 C
    with pytest.raises(H.GtError, match="EINVAL"):
        H.gemm(x, w, y, 100, 128, 9 * 128, conv=(8, 8, 128), **kw)           # M not whole images
    x24 = rnd(2, 8, 8, 24, dev=dev, seed=132)
    with pytest.raises(NotImplementedError):
        H.gemm(x24, w, y, 128, 128, 9 * 24, conv=(8, 8, 24), lda=24, ldb=9 * 24, ldc=128)
    dw9 = torch.empty(9, 128, 128, device=dev)
    wkw = dict(layout_a=1, layout_b=1, lda=128, ldb=128, ldc=128, batch=(9, 1), c_bs=(128 * 128, 0), conv_wgrad=True)
    with pytest.raises(NotImplementedError):                                 # images narrower than one stage
        H.gemm(y, x, dw9, 128, 128, 128, conv=(8, 8, 128), split_k=0, **wkw)
    with pytest.raises(H.GtError, match="EINVAL"):                           # the nine taps are the batch
        H.gemm(y, x, dw9, 128, 128, 128, conv=(8, 8, 128), split_k=0, **dict(wkw, batch=(3, 1)))


def test_upsample_fc_channels_last_equals_channels_first(H, gpu_device):
    """ops.upsample_fc(x_nhwc=True) (plain token GEMMs + the tall-skinny weight gradient) == the channels-first
    formulation on the same numbers, outputs and all gradients."""
    from galerkin_transformer import ops
    dev = gpu_device
    B, K, Hi, Ho, N, p = 3, 128, 20, 37, 32, 2
    x = rnd(B, K, Hi, Hi, dev=dev, seed=140)
    W = rnd(N, K + p, dev=dev, seed=141, scale=0.2)
    b = rnd(N, dev=dev, seed=142)
    grid = rnd(B, Ho, Ho, p, dev=dev, seed=143)
    cot = rnd(B, Ho, Ho, N, dev=dev, seed=144)
    res = []
    for nhwc in (False, True):
        xx = (x.permute(0, 2, 3, 1).contiguous() if nhwc else x.clone()).requires_grad_(True)
        Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = ops.upsample_fc(xx, (Ho, Ho), Wg, bg, grid, x_nhwc=nhwc)
        out.backward(cot)
        res.append((out, xx.grad.permute(0, 3, 1, 2) if nhwc else xx.grad, Wg.grad, bg.grad))
    for a, c in zip(*res):
        assert rel_l2(a, c) < 2e-6


def test_upscaler_channels_last_path_equals_channels_first(H, gpu_device):
    """Interp2dUpsample (layers.py:624-670) with the implicit-GEMM conv block (all channels-last) == the same module on
    the library convolution (channels-first), forward and every gradient, dropout off."""
    from galerkin_transformer import layers, ops
    dev = gpu_device
    torch.manual_seed(5)
    up = layers.Interp2dUpsample(128, 128, interp_size=((19, 19), (31, 31)), dropout=0.0).to(dev)
    x = rnd(2, 11, 11, 128, dev=dev, seed=150)
    cot = rnd(2, 31, 31, 128, dev=dev, seed=151)
    res = []
    for implicit in (True, False):
        ops._conv_implicit[0] = implicit
        try:
            # the implicit GEMM lives on the split-operand engine: under GT_PRECISION=f32 both passes are the library's
            assert up.features_nhwc() == (implicit and H.get_precision() != "f32")
            up.zero_grad()
            xx = x.clone().requires_grad_(True)
            y = up(xx, in_nhwc=True, out_nhwc=True)
            y.backward(cot)
            res.append((y, xx.grad, up.conv[0].conv[0].weight.grad.clone()))
        finally:
            ops._conv_implicit[0] = True
    for a, c in zip(*res):
        assert rel_l2(a, c) < 5e-6


@pytest.mark.parametrize("la,lb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(16384 + 40, 128, 128), (16400, 200, 16), (20000, 96, 40), (16384, 256, 1152),
                                   (16384, 136, 20), (16386, 128, 18), (4096, 128, 128)])
def test_gemm_x3_packed_b(H, gpu_device, la, lb, M, N, K):
    """gemm_x3p_kernel: B split once into fragment-ordered bf16 planes (x3_pack_b_kernel), read straight into the MFMA
    operand registers; A through the ring.  Token-row shapes (M >= 16384, M >= 8 N) in every layout, ragged M / N / K
    (partial pixel tiles, a partial last k-stage, N that does not fill its 128-column tile), 1, 2 and many k-stages; below
    16384 rows the pack launch is not paid back and the ring kernel splits B per block."""
    dev = gpu_device
    A = rnd(M, K, dev=dev, seed=301) if la == 0 else rnd(K, M, dev=dev, seed=301)
    B = rnd(N, K, dev=dev, seed=302) if lb == 0 else rnd(K, N, dev=dev, seed=302)
    name = H.gemm_kernel_name(A, B, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1], ldb=B.shape[1], ldc=N,
                              precision="bf16x3")
    aligned = (K % 4 == 0) if la == 0 else (M % 4 == 0)
    assert ("gemm_x3p_kernel" in name) == (aligned and M >= 16384), name
    Cc = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, B, Cc, M, N, K, layout_a=la, layout_b=lb, lda=A.shape[1], ldb=B.shape[1], ldc=N, precision="bf16x3")
    torch.cuda.synchronize()
    assert rel_l2(Cc, ref_mm(A, B, la, lb)) < X3_TOL["bf16x3"]


def test_gemm_x3_packed_b_epilogue_and_a_dropout(H, gpu_device):
    """The packed-B kernel with the fused epilogue (bias, SiLU, residual, pre-activation output) and the A-operand
    dropout prologue == the fp32 MFMA kernel on the same masks."""
    dev = gpu_device
    M, N, K = 16500, 128, 256
    A, B = rnd(M, K, dev=dev, seed=310), rnd(N, K, dev=dev, seed=311, scale=0.1)
    bias, res = rnd(N, dev=dev, seed=312), rnd(M, N, dev=dev, seed=313)
    H.set_seed(99, dev)
    drop = H.dropout_desc(0.1, 5, dev)
    out = {}
    for prec in ("f32", "bf16x3"):
        Cc, pre = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        H.gemm(A, B, Cc, M, N, K, lda=K, ldb=K, ldc=N, bias=bias, act=H.ACT_SILU, res=res, ldr=N, pre=pre, ldpre=N,
               a_drop=drop, a_drop_ld=K, precision=prec)
        out[prec] = (Cc, pre)
    torch.cuda.synchronize()
    assert rel_l2(out["bf16x3"][0], out["f32"][0]) < 2e-6 and rel_l2(out["bf16x3"][1], out["f32"][1]) < 2e-6


@pytest.mark.parametrize("B,n,h,dk,p", [(2, 100, 4, 32, 2), (1, 37, 2, 16, 2), (3, 1849, 4, 32, 2), (1, 64, 1, 48, 2),
                                        (2, 50, 4, 36, 0), (2, 300, 2, 32, 1), (1, 90, 4, 16, 3)])
def test_galerkin_dkv_ln_fused_equals_two_passes(H, gpu_device, B, n, h, dk, p):
    """gt_galerkin_dkv_ln (dK', dV' products + head LayerNorm backward + Q un-padding in one pass) ==
    gt_galerkin_dkv followed by gt_headnorm_bwd with norm_mask = K, V (layers.py:841-874 and :723 backwards)."""
    dev = gpu_device
    T, DP = B * n, H.round4(dk + p)
    assert H.galerkin_dkv_ln_supported(dk, p, 0b110)
    Kp, Vp = rnd(T, h, DP, dev=dev, seed=400), rnd(T, h, DP, dev=dev, seed=401)
    dM = rnd(B, h, DP, DP, dev=dev, seed=402, scale=0.2)
    dQp = rnd(T, h, DP, dev=dev, seed=403)
    qkv = rnd(T, 3 * h * dk, dev=dev, seed=404)
    gamma = 1 + 0.2 * rnd(2, h, dk, dev=dev, seed=405)
    stats = torch.stack([0.3 * rnd(2, T, h, dev=dev, seed=406), 0.5 + rnd(2, T, h, dev=dev, seed=407).abs()], -1).contiguous()
    dO3 = torch.empty(3, T, h, DP, device=dev)
    dO3[0] = dQp
    H.galerkin_dkv(Kp, Vp, dM, dO3[1], dO3[2], B, n, h, DP)
    ref = H.headnorm_bwd(dO3, qkv, gamma, stats, T, h, dk, p, 0b110)
    got = H.galerkin_dkv_ln(Kp, Vp, dM, dQp, qkv, gamma, stats, B, n, h, dk, p)
    torch.cuda.synchronize()
    for a, c, name in zip(got, ref, ("d_qkv", "dgamma", "dbeta")):
        assert not torch.isnan(a).any(), name
        assert rel_l2(a, c) < 2e-6, name


def test_galerkin_dkv_ln_unsupported_shapes(H, gpu_device):
    assert not H.galerkin_dkv_ln_supported(32, 2, 0b011)       # fourier-type norms (Q, K)
    assert not H.galerkin_dkv_ln_supported(64, 2, 0b110)       # head tile of 68 floats


@pytest.mark.parametrize("batch", [16, 3])
def test_gemm_x3_split_k_width_split(H, gpu_device, batch):
    """Token-contracted product with N = 144 (the merged-head width of the Darcy model), K slices, batched, with the
    row-sum by-product: with enough K slices to fill the chip the library runs the aligned 128 columns on the
    split-operand kernel and the 16-column remainder on a narrow fp32 tile (two launches, gt_gemm: width_split);
    batch 3 stays one launch.  Both against fp64."""
    dev = gpu_device
    M, N, K = 128, 144, 1849
    A = rnd(batch, K, M, dev=dev, seed=500)
    B = rnd(batch, K, N, dev=dev, seed=501)
    Cc = torch.full((batch, M, N), float("nan"), device=dev)
    cs = torch.full((M,), float("nan"), device=dev)
    H.gemm(A, B, Cc, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, batch=(batch, 1), a_bs=(K * M, 0),
           b_bs=(K * N, 0), c_bs=(M * N, 0), split_k=0, a_colsum=cs, precision="bf16x3")
    torch.cuda.synchronize()
    assert rel_l2(Cc, A.double().transpose(1, 2) @ B.double()) < KTOL
    assert rel_l2(cs, A.double().sum((0, 1))) < KTOL


def _plain_case(H, dev, B, n, h, dk, p, seed):
    """Raw K / V projections with their LayerNorm statistics, the affine head tiles K', V' and the "plain" tiles (xh)."""
    T, DP = B * n, H.round4(dk + p)
    d = h * dk
    qkv = rnd(T, 3 * d, dev=dev, seed=seed)
    gamma = 1 + 0.3 * rnd(2, h, dk, dev=dev, seed=seed + 1)
    beta = 0.2 * rnd(2, h, dk, dev=dev, seed=seed + 2)
    pos = rnd(T, p, dev=dev, seed=seed + 3) if p else None
    eps = 1e-6
    tiles, plains, stats = [], [], []
    for st in (1, 2):
        x = qkv[:, st * d:(st + 1) * d].reshape(T, h, dk).double()
        mu = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
        xh = (x - mu) * rstd
        y = xh * gamma[st - 1].double() + beta[st - 1].double()
        for src, dst in ((y, tiles), (xh, plains)):
            tile = torch.zeros(T, h, DP, dtype=torch.float64, device=dev)
            if p:
                tile[:, :, :p] = pos.double()[:, None, :]
            tile[:, :, p:p + dk] = src
            dst.append(tile.float().contiguous())
        stats.append(torch.cat([mu, rstd], -1))
    return qkv, gamma, beta, torch.stack(stats).float().contiguous(), tiles, plains


@pytest.mark.parametrize("B,n,h,dk,p", [(2, 100, 4, 32, 2), (1, 37, 2, 16, 2), (2, 700, 4, 32, 1), (1, 64, 1, 48, 2)])
def test_plain_head_tiles_ktv_and_dkv_ln(H, gpu_device, B, n, h, dk, p):
    """ "Plain" head tiles (normalised values without the LayerNorm affine, gt_hip.h: hn_plain): gt_galerkin_ktv_affine on
    them == gt_galerkin_ktv on the affine tiles, and gt_galerkin_dkv_ln_plain (gamma folded into dM, beta dM added, xh taken
    from the tiles, no raw projection) == gt_galerkin_dkv_ln on the affine tiles + raw projection."""
    dev = gpu_device
    T, DP = B * n, H.round4(dk + p)
    qkv, gamma, beta, stats, (Kp, Vp), (Kx, Vx) = _plain_case(H, dev, B, n, h, dk, p, 600)
    ref = H.galerkin_ktv(Kp, Vp, B, n, h, dk, p)
    got = H.galerkin_ktv(Kx, Vx, B, n, h, dk, p, gamma=gamma, beta=beta)
    torch.cuda.synchronize()
    assert rel_l2(got.sum(0), ref.sum(0)) < 2e-6
    # ... and `ref` itself against float64, per element and per slab (tests/_galerkin_ref.py): not kernel against kernel only
    ref64, E = G.ktv_ref(Kp.cpu(), Vp.cpu(), B, n, h, dk, p, ref.shape[0])
    assert G.gate_violation(ref.cpu(), ref64, E, "ktv") is None, G.gate_violation(ref.cpu(), ref64, E, "ktv")
    dM = rnd(B, h, DP, DP, dev=dev, seed=610, scale=0.2)
    dQp = rnd(T, h, DP, dev=dev, seed=611)
    ref = H.galerkin_dkv_ln(Kp, Vp, dM, dQp, qkv, gamma, stats, B, n, h, dk, p)
    got = H.galerkin_dkv_ln(Kx, Vx, dM, dQp, None, gamma, stats, B, n, h, dk, p, beta=beta)
    torch.cuda.synchronize()
    for a, c, name in zip(got, ref, ("d_qkv", "dgamma", "dbeta")):
        assert not torch.isnan(a).any(), name
        assert rel_l2(a, c) < 3e-6, name


@pytest.mark.parametrize("prec", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("T,mask", [(20736, 0b110), (16500, 0b011)])
def test_qkv_headnorm_head_slots_dk48(H, gpu_device, T, mask, prec):
    """Round 6: GT_EP_HEADNORM for 48-wide heads (ex3: d_model 192, 4 heads; reference layers.py:838-874 with d_k = 48) on the
    packed-B kernels -- every head in a 64-column slot of the tile, the 16 columns behind it zero rows of the packed weight
    (gt_gemm_desc.hip: hn_slots) -- against gt_gemm + gt_headnorm_fwd: head tiles, statistics, the raw projection where it is
    written (skip_raw), plain tiles without any raw projection, and the weight packed ahead (gt_gemm_pack_b_many)."""
    import ctypes as C
    dev = gpu_device
    h, dk, p = 4, 48, 2
    d = h * dk
    x = rnd(T, d, dev=dev, seed=130)
    w = rnd(3 * d, d, dev=dev, seed=131, scale=0.2)
    b = rnd(3 * d, dev=dev, seed=132)
    gamma = 1 + 0.1 * rnd(2, h, dk, dev=dev, seed=133)
    beta = 0.1 * rnd(2, h, dk, dev=dev, seed=134)
    pos = rnd(T, p, dev=dev, seed=135)
    eps = 1e-7
    qkv = torch.empty(T, 3 * d, device=dev)
    H.gemm(x, w, qkv, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, precision="f32")
    out_ref, st_ref = H.headnorm_fwd(qkv, pos, gamma, beta, T, h, dk, p, mask, eps)
    DP = H.round4(dk + p)
    assert DP == 52
    qkv2 = torch.full_like(qkv, float("nan"))
    out3 = torch.full((3, T, h, DP), float("nan"), device=dev)
    stats = torch.zeros(2, T, h, 2, device=dev)
    hn = dict(gamma=gamma, beta=beta, pos=pos, out=out3, stats=stats, h=h, dk=dk, p=p, norm_mask=mask, eps=eps)
    H.gemm(x, w, qkv2, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=hn, precision=prec)
    torch.cuda.synchronize()
    assert not torch.isnan(out3).any() and not torch.isnan(qkv2).any()
    assert rel_l2(qkv2, qkv) < 2e-6
    assert rel_l2(out3, out_ref) < 3e-6 and rel_l2(stats, st_ref) < 3e-6
    assert torch.equal(out3[..., :p], out_ref[..., :p]) and torch.equal(out3[..., p + dk:], torch.zeros_like(out3[..., p + dk:]))
    # skip_raw: only the normalised streams' raw blocks are written
    qkv3 = torch.full_like(qkv, float("nan"))
    out3b = torch.empty_like(out3)
    H.gemm(x, w, qkv3, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=dict(hn, out=out3b, skip_raw=(~mask) & 7), precision=prec)
    torch.cuda.synchronize()
    for st in range(3):
        blk = qkv3[:, st * d:(st + 1) * d]
        if (mask >> st) & 1:
            assert torch.equal(blk, qkv2[:, st * d:(st + 1) * d])
        else:
            assert torch.isnan(blk).all()
    assert torch.equal(out3b, out3)
    if mask == 0b110:       # plain tiles: (x - mean) * rstd, nothing written to C (C = None)
        outp = torch.full_like(out3, float("nan"))
        stp = torch.zeros_like(stats)
        H.gemm(x, w, None, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, precision=prec,
               hn=dict(hn, out=outp, stats=stp, skip_raw=7, plain=True))
        torch.cuda.synchronize()
        assert torch.equal(stp, stats) and torch.equal(outp[0], out3[0])
        for s_ in (1, 2):
            val = outp[s_][:, :, p:p + dk] * gamma[s_ - 1] + beta[s_ - 1]
            assert rel_l2(val, out3[s_][:, :, p:p + dk]) < 1e-6
            assert torch.equal(outp[s_][:, :, :p], out3[s_][:, :, :p]) and torch.equal(outp[s_][:, :, p + dk:], out3[s_][:, :, p + dk:])
    if prec == "f16x2":     # the weight packed ahead through the C ABI = the per-call pack, bit for bit
        dsc = H.GtGemmDesc()
        L = H.lib()
        L.gt_gemm_desc_init(C.byref(dsc))
        dsc.M, dsc.N, dsc.K, dsc.lda, dsc.ldb, dsc.ldc = T, 3 * d, d, d, d, 3 * d
        dsc.A, dsc.B, dsc.C, dsc.bias = x.data_ptr(), w.data_ptr(), qkv3.data_ptr(), b.data_ptr()
        dsc.precision, dsc.ep_mode = H.PREC_F16X2, H.EP_HEADNORM
        dsc.hn_gamma, dsc.hn_beta, dsc.hn_pos = gamma.data_ptr(), beta.data_ptr(), pos.data_ptr()
        out3c, stc = torch.full_like(out3, float("nan")), torch.zeros_like(stats)
        dsc.hn_out, dsc.hn_stats = out3c.data_ptr(), stc.data_ptr()
        dsc.hn_h, dsc.hn_dk, dsc.hn_p, dsc.hn_norm_mask, dsc.hn_eps = h, dk, p, mask, eps
        need = L.gt_gemm_packed_b_bytes(C.byref(dsc))
        assert need == 3 * (3 * h * 64 // 32) * (d // 16) * 1024         # planes of the SLOT width 3 h 64, not of 3 h 48
        pack = torch.empty(need, dtype=torch.uint8, device=dev)
        descs = (H.GtGemmDesc * 1)(dsc)
        outs = (C.c_void_p * 1)(pack.data_ptr())
        H.check(L.gt_gemm_pack_b_many(descs, outs, 1, H.stream_ptr()), "gt_gemm_pack_b_many")
        dsc.b_packed = pack.data_ptr()
        assert L.gt_gemm_ws_bytes(C.byref(dsc)) == 0
        H.check(L.gt_gemm(C.byref(dsc), None, 0, H.stream_ptr()), "gt_gemm")
        torch.cuda.synchronize()
        assert torch.equal(out3c, out3) and torch.equal(stc, stats)


@pytest.mark.parametrize("N,K,lb", [(64, 192, 0), (64, 384, 1), (48, 96, 0), (48, 48, 1), (16, 64, 0), (80, 128, 0)])
def test_narrow_token_products_on_the_packed_kernels(H, gpu_device, N, K, lb):
    """Round 6 (VERDICT r5 missing 4 / next-round 5): token products with a narrow output (N < 96: the d_model = 48 / 64 layers
    of ex4 / ex1, the 64-column remainder of ex3's 192-wide products; nn.Linear at reference layers.py:811,823,964,976) run on
    the packed-B two-term fp16 kernels (128 x 64 tile for N <= 64) from 16 384 token rows, with the full fused epilogue --
    against fp64, and the same mask / residual as the fp32-MFMA engine they ran on before."""
    dev = gpu_device
    M = 16384 + 777
    A = rnd(M, K, dev=dev, seed=300)
    B = rnd(N, K, dev=dev, seed=301, scale=0.2) if lb == 0 else rnd(K, N, dev=dev, seed=301, scale=0.2)
    bias, R = rnd(N, dev=dev, seed=302), rnd(M, N, dev=dev, seed=303)
    name = H.gemm_kernel_name(A, B, M, N, K, layout_b=lb, lda=K, ldb=B.shape[1], ldc=N, precision="f16x2")
    assert "gemm_x3h_kernel<0, 0, 0, %d>" % (64 if N <= 64 else 128) in name, name
    assert "x3" not in H.gemm_kernel_name(A[:5000], B, 5000, N, K, layout_b=lb, lda=K, ldb=B.shape[1], ldc=N, precision="f16x2")
    outs = {}
    for prec in ("f32", "f16x2", "bf16x3"):
        Cc = torch.full((M, N), float("nan"), device=dev)
        H.gemm(A, B, Cc, M, N, K, layout_b=lb, lda=K, ldb=B.shape[1], ldc=N, bias=bias, act=H.ACT_RELU,
               drop=H.dropout_desc(0.25, 91, dev), res=R, ldr=N, out_scale=-0.5, precision=prec)
        outs[prec] = Cc
    torch.cuda.synchronize()
    keep = H.dropout_apply(torch.ones(M, N, device=dev), H.dropout_desc(0.25, 91, dev)).double()
    ref = R.double() - 0.5 * torch.relu(ref_mm(A, B, 0, lb) + bias.double()) * keep
    for prec in outs:
        assert rel_l2(outs[prec], ref) < KTOL, (prec, rel_l2(outs[prec], ref))


@pytest.mark.parametrize("M,N,K,prec", [(20000, 128, 256, "f16x2"), (20000, 192, 384, "f16x2"), (20000, 64, 128, "f16x2"),
                                        (3000, 128, 256, "f16x2"), (777, 96, 130, "f32"), (20000, 128, 256, "bf16x3")])
def test_gemm_second_output_under_a_dropout_mask(H, gpu_device, M, N, K, prec):
    """gt_gemm_desc.c_masked (round 6): the finished result once more under a second stateless dropout mask, bit for bit what
    gt_dropout_apply makes of C -- on the packed-B fast epilogue, its width-split / narrow-tile forms, the ring kernel and the
    fp32 engine's per-row epilogue.  (The data gradient between two encoder blocks, reference model.py:125,132 backwards.)"""
    dev = gpu_device
    A, W = rnd(M, K, dev=dev, seed=320), rnd(N, K, dev=dev, seed=321, scale=0.1)
    R = rnd(M, N, dev=dev, seed=322)
    Cc = torch.full((M, N), float("nan"), device=dev)
    Cm = torch.full((M, N), float("nan"), device=dev)
    dm = H.dropout_desc(0.05, 4242, dev)
    H.gemm(A, W, Cc, M, N, K, lda=K, ldb=K, ldc=N, res=R, ldr=N, precision=prec, c_masked=Cm, ldc_masked=N, c_mask=dm)
    plain = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, W, plain, M, N, K, lda=K, ldb=K, ldc=N, res=R, ldr=N, precision=prec)
    torch.cuda.synchronize()
    assert torch.equal(Cc, plain)
    assert torch.equal(Cm, H.dropout_apply(Cc, dm))
    assert 0.03 < float((Cm == 0).float().mean()) < 0.07
    # split-K products have no second output
    with pytest.raises(NotImplementedError):
        H.gemm(A, R, torch.empty(K, N, device=dev), K, N, M, layout_a=1, layout_b=1, lda=K, ldb=N, ldc=N, split_k=4,
               c_masked=torch.empty(K, N, device=dev), ldc_masked=N, c_mask=dm)


@pytest.mark.parametrize("M,N,K,prec,conv", [(20000, 128, 256, "f16x2", None), (4 * 40 * 40, 128, 9 * 128, "f16x2", (40, 40, 128)),
                                             (777, 96, 130, "f32", None), (20000, 128, 256, "bf16x3", None)])
def test_gemm_two_silus_on_the_epilogue(H, gpu_device, M, N, K, prec, conv):
    """GT_ACT_SILU2 (ABI v21): silu(silu(A W^T)) with the product of the two derivatives left in `pre` -- the conv block ->
    activation -> activation tail of Interp2dUpsample (reference layers.py:642-650) when its dropouts are off -- on the
    packed-B fast epilogue (plain and implicit 3x3 convolution), the ring kernel and the fp32 engine's per-row epilogue."""
    dev = gpu_device
    if conv is None:
        A, W = rnd(M, K, dev=dev, seed=340), rnd(N, K, dev=dev, seed=341, scale=0.1)
        u = A.double() @ W.double().t()
        kw = dict(lda=K, ldb=K, ldc=N)
    else:
        Hh, Ww, Cc = conv
        img = rnd(M // (Hh * Ww), Hh, Ww, Cc, dev=dev, seed=340)
        w4 = rnd(N, Cc, 3, 3, dev=dev, seed=341, scale=0.05)
        u = torch.nn.functional.conv2d(img.double().permute(0, 3, 1, 2), w4.double(), padding=1).permute(0, 2, 3, 1).reshape(M, N)
        from galerkin_transformer import ops as _ops
        A, W = img.reshape(M, Cc), _ops._conv_k_order(w4.permute(0, 2, 3, 1).reshape(N, 9, Cc))
        kw = dict(lda=Cc, ldb=9 * Cc, ldc=N, conv=conv)
    out = torch.full((M, N), float("nan"), device=dev)
    fac = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, W, out, M, N, K, act=H.ACT_SILU2, pre=fac, ldpre=N, precision=prec, **kw)
    out_only = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, W, out_only, M, N, K, act=H.ACT_SILU2, precision=prec, **kw)
    torch.cuda.synchronize()
    ud = u.clone().requires_grad_(True)
    ref = torch.nn.functional.silu(torch.nn.functional.silu(ud))
    ref.sum().backward()
    assert rel_l2(out, ref.detach()) < KTOL and rel_l2(fac, ud.grad) < KTOL
    assert torch.equal(out, out_only)
    with pytest.raises(H.GtError):         # a dropout has no place in this form (GT_EINVAL)
        H.gemm(A, W, out, M, N, K, act=H.ACT_SILU2, drop=H.dropout_desc(0.1, 5, dev), precision=prec, **kw)


@pytest.mark.parametrize("T,p_h,p_o,with_res,act", [(16384 + 37, 0.05, 0.05, True, "relu"), (236672, 0.05, 0.1, True, "relu"),
                                                    (20000, 0.0, 0.0, False, "relu"), (16448, 0.3, 0.0, True, "none")])
def test_ffn_fused_forward_equals_two_launches(H, gpu_device, T, p_h, p_o, with_res, act):
    """gt_ffn_fwd (round 6; VERDICT r5 next-round 2, forward half): FeedForward.forward (reference layers.py:979-987) + the
    residual of model.py:131-132 in ONE launch with the hidden tile of 64 token rows kept in LDS -- the bits of the two
    packed-B gt_gemm launches it replaces (hidden activation AND output, dropout masks included), a token count that is not a
    multiple of the tile, and fp64 for good measure."""
    dev = gpu_device
    d, f = 128, 256
    x = rnd(T, d, dev=dev, seed=330)
    w1, b1 = rnd(f, d, dev=dev, seed=331, scale=0.1), rnd(f, dev=dev, seed=332, scale=0.1)
    w2, b2 = rnd(d, f, dev=dev, seed=333, scale=0.1), rnd(d, dev=dev, seed=334, scale=0.1)
    a = H.ACT_CODE[act]
    dh = H.dropout_desc(p_h, 500, dev) if p_h > 0 else None
    do = H.dropout_desc(p_o, 501, dev) if p_o > 0 else None
    res = x if with_res else None
    hid0, out0 = torch.full((T, f), float("nan"), device=dev), torch.full((T, d), float("nan"), device=dev)
    H.gemm(x, w1, hid0, T, f, d, lda=d, ldb=d, ldc=f, bias=b1, act=a, drop=dh, precision="f16x2")
    H.gemm(hid0, w2, out0, T, d, f, lda=f, ldb=f, ldc=d, bias=b2, drop=do, res=res, ldr=d, precision="f16x2")
    assert H.ffn_fwd_supported(T, d, f, a) or H.get_precision() != "f16x2"       # (the operator takes it in the fp16 mode only)
    hid1, out1 = torch.full((T, f), float("nan"), device=dev), torch.full((T, d), float("nan"), device=dev)
    H.ffn_fwd(x, w1, b1, w2, b2, res, dh, do, a, hid1, out1)
    torch.cuda.synchronize()
    presplit = os.environ.get("GT_FFN_PRESPLIT", "1") != "0"
    if presplit:        # the hidden tile is split ONCE per block under one exponent per token row: same products, another
        # (never smaller) scale than the running exponents of the separate launches (phase 1 keeps them: hid is bit-equal today)
        assert rel_l2(hid1, hid0) < 5e-7 and rel_l2(out1, out0) < 5e-7
        hid0 = hid1.clone()
    else:
        assert torch.equal(hid1, hid0) and torch.equal(out1, out0)
    pre = x.double() @ w1.double().t() + b1.double()
    h = torch.relu(pre) if act == "relu" else pre
    if dh is not None:
        h = h * H.dropout_apply(torch.ones(T, f, device=dev), dh).double()
    y = h @ w2.double().t() + b2.double()
    if do is not None:
        y = y * H.dropout_apply(torch.ones(T, d, device=dev), do).double()
    ref = y + (x.double() if with_res else 0.0)
    assert rel_l2(out1, ref) < KTOL and rel_l2(hid1, h) < KTOL
    first = out1.clone()
    for _ in range(10):                                   # counted waits: repeated launches return the same bits
        H.ffn_fwd(x, w1, b1, w2, b2, res, dh, do, a, hid1, out1)
        assert torch.equal(out1, first) and torch.equal(hid1, hid0)
    # rows of very different magnitude (one exponent per row must track each of them): relative error per row against fp64
    xs = x * torch.logspace(-6, 3, T, device=dev).unsqueeze(1)
    H.ffn_fwd(xs, w1, None, w2, None, None, None, None, a, hid1, out1)
    hr = xs.double() @ w1.double().t()
    hr = torch.relu(hr) if act == "relu" else hr
    yr = hr @ w2.double().t()
    rowerr = (out1.double() - yr).norm(dim=1) / yr.norm(dim=1).clamp_min(1e-300)
    assert float(rowerr.max()) < 2e-6, float(rowerr.max())
    assert not H.ffn_fwd_supported(5000, d, f, a) and not H.ffn_fwd_supported(T, 192, 384, a)


@pytest.mark.parametrize("T,p_h,with_res,p2", [(16384 + 37, 0.05, True, 0.05), (236672, 0.05, True, 0.0), (20000, 0.0, False, 0.1)])
def test_ffn_fused_backward_data_half(H, gpu_device, T, p_h, with_res, p2):
    """gt_ffn_bwd (round 6): gh = (gm W2) through the forward's ReLU / dropout decision bits, dx = g + gh W1 and the masked twin
    of dx in ONE launch -- against the two packed-B launches it replaces (hidden-gradient product with the saved activation as
    its GT_AUX_GT0 operand, data-gradient product with c_masked) and against fp64; the hidden activation is not an input."""
    dev = gpu_device
    d, f = 128, 256
    x = rnd(T, d, dev=dev, seed=340)
    w1, b1 = rnd(f, d, dev=dev, seed=341, scale=0.1), rnd(f, dev=dev, seed=342, scale=0.1)
    w2, b2 = rnd(d, f, dev=dev, seed=343, scale=0.1), rnd(d, dev=dev, seed=344, scale=0.1)
    dh = H.dropout_desc(p_h, 510, dev) if p_h > 0 else None
    hid, out = torch.empty(T, f, device=dev), torch.empty(T, d, device=dev)
    bits = H.ffn_fwd(x, w1, b1, w2, b2, x, dh, None, H.ACT_RELU, hid, out, want_bits=True)
    gm, g = rnd(T, d, dev=dev, seed=345), rnd(T, d, dev=dev, seed=346)
    res = g if with_res else None
    m2 = H.dropout_desc(p2, 511, dev) if p2 > 0 else None
    scale = 1.0 / (1.0 - p_h)
    # the two launches
    gh0, dx0, dxm0 = (torch.full((T, n), float("nan"), device=dev) for n in (f, d, d))
    H.gemm(gm, w2, gh0, T, f, d, layout_b=1, lda=d, ldb=f, ldc=f, aux_op=H.AUX_GT0, aux=hid, ldaux=f, aux_scale=scale, precision="f16x2")
    H.gemm(gh0, w1, dx0, T, d, f, layout_b=1, lda=f, ldb=d, ldc=d, res=res, ldr=d, c_masked=dxm0, ldc_masked=d, c_mask=m2,
           precision="f16x2")
    gh1, dx1, dxm1 = (torch.full((T, n), float("nan"), device=dev) for n in (f, d, d))
    H.ffn_bwd(gm, w2, w1, bits, scale, res, gh1, dx1, dxm1, m2)
    torch.cuda.synchronize()
    assert rel_l2(gh1, gh0) < 5e-7 and rel_l2(dx1, dx0) < 5e-7
    assert torch.equal(gh1 != 0, gh0 != 0)                 # the same decisions
    gh0 = gh1.clone()
    keep2 = H.dropout_apply(torch.ones(T, d, device=dev), m2) if m2 is not None else torch.ones(T, d, device=dev)
    assert torch.equal(dxm1, dx1 * keep2)
    ghr = (gm.double() @ w2.double()) * (hid > 0).double() * scale
    dxr = ghr @ w1.double() + (g.double() if with_res else 0.0)
    assert rel_l2(gh1, ghr) < KTOL and rel_l2(dx1, dxr) < KTOL
    first = dx1.clone()
    for _ in range(5):
        H.ffn_bwd(gm, w2, w1, bits, scale, res, gh1, dx1, dxm1, m2)
        assert torch.equal(dx1, first) and torch.equal(gh1, gh0)


def test_width_split_product_takes_a_weight_packed_ahead(H, gpu_device):
    """N = 192 (ex3's d_model) is cut into a 128-column launch and a 64-column remainder; round 6: both run on the packed-B
    kernels and gt_gemm_packed_b_bytes / gt_gemm_pack_b_many / gt_gemm_desc.b_packed describe the two packs back to back --
    the product with the weight packed ahead returns the bits of the per-call pack (and ADVICE r5: a b_packed pointer on a
    product that is NOT packed that way is refused instead of being read with the wrong geometry)."""
    import ctypes as C
    dev = gpu_device
    M, N, K = 20000, 192, 384
    A, W = rnd(M, K, dev=dev, seed=310), rnd(N, K, dev=dev, seed=311, scale=0.1)
    bias, R = rnd(N, dev=dev, seed=312), rnd(M, N, dev=dev, seed=313)
    ref = torch.full((M, N), float("nan"), device=dev)
    H.gemm(A, W, ref, M, N, K, lda=K, ldb=K, ldc=N, bias=bias, res=R, ldr=N, precision="f16x2")
    L = H.lib()
    d = H.GtGemmDesc()
    L.gt_gemm_desc_init(C.byref(d))
    out = torch.full((M, N), float("nan"), device=dev)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ldr = M, N, K, K, K, N, N
    d.A, d.B, d.C, d.bias, d.res = A.data_ptr(), W.data_ptr(), out.data_ptr(), bias.data_ptr(), R.data_ptr()
    d.precision = H.PREC_F16X2
    need = L.gt_gemm_packed_b_bytes(C.byref(d))
    one = lambda n: 3 * ((n + 127) // 128 * 4) * (K // 16) * 1024
    assert need == one(128) + one(64)
    pack = torch.empty(need, dtype=torch.uint8, device=dev)
    H.check(L.gt_gemm_pack_b_many((H.GtGemmDesc * 1)(d), (C.c_void_p * 1)(pack.data_ptr()), 1, H.stream_ptr()), "pack")
    d.b_packed = pack.data_ptr()
    assert L.gt_gemm_ws_bytes(C.byref(d)) == 0
    H.check(L.gt_gemm(C.byref(d), None, 0, H.stream_ptr()), "gt_gemm")
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert rel_l2(out, A.double() @ W.double().t() + bias.double() + R.double()) < KTOL
    d.M = 3000                                   # below the packed kernels' row count: b_packed has no meaning here
    assert L.gt_gemm_packed_b_bytes(C.byref(d)) == 0
    ws = H.workspace(dev, max(int(L.gt_gemm_ws_bytes(C.byref(d))), 1 << 20))
    assert L.gt_gemm(C.byref(d), ws.data_ptr(), ws.numel(), H.stream_ptr()) == -1          # GT_EINVAL


def test_qkv_headnorm_plain_tiles(H, gpu_device):
    """GT_EP_HEADNORM with hn_plain: K / V tiles hold (x - mean) * rstd, no raw projection is written (C = None)."""
    dev = gpu_device
    T, h, dk, p, mask = 1500, 4, 32, 2, 0b110
    d = h * dk
    x = rnd(T, d, dev=dev, seed=620)
    w = rnd(3 * d, d, dev=dev, seed=621, scale=0.2)
    b = rnd(3 * d, dev=dev, seed=622)
    gamma = 1 + 0.1 * rnd(2, h, dk, dev=dev, seed=623)
    beta = 0.1 * rnd(2, h, dk, dev=dev, seed=624)
    pos = rnd(T, p, dev=dev, seed=625)
    DP = H.round4(dk + p)
    out_ref = torch.empty(3, T, h, DP, device=dev)
    st_ref = torch.zeros(2, T, h, 2, device=dev)
    qkv = torch.empty(T, 3 * d, device=dev)
    hn = dict(gamma=gamma, beta=beta, pos=pos, out=out_ref, stats=st_ref, h=h, dk=dk, p=p, norm_mask=mask, eps=1e-7)
    H.gemm(x, w, qkv, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, hn=hn, precision="bf16x3")
    out = torch.full_like(out_ref, float("nan"))
    st = torch.zeros_like(st_ref)
    H.gemm(x, w, None, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=b, precision="bf16x3",
           hn=dict(hn, out=out, stats=st, skip_raw=7, plain=True))
    torch.cuda.synchronize()
    assert torch.equal(st, st_ref) and torch.equal(out[0], out_ref[0])
    for s_ in (1, 2):                                  # affine tile = gamma * plain + beta on the value columns
        val = out[s_][:, :, p:p + dk] * gamma[s_ - 1] + beta[s_ - 1]
        assert rel_l2(val, out_ref[s_][:, :, p:p + dk]) < 1e-6
        assert torch.equal(out[s_][:, :, :p], out_ref[s_][:, :, :p]) and torch.equal(out[s_][:, :, p + dk:], out_ref[s_][:, :, p + dk:])


# ------------------------------------------------------------------------------------------- channels-last down-scaler
def _ref_conv(x_nhwc, w):
    """conv2d(padding=1) on a channels-last fp64 image."""
    return torch.nn.functional.conv2d(x_nhwc.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,Hh,Ww,Cin,Cout,pitch_in,pitch_out", [(3, 78, 78, 128, 42, 128, 144), (3, 78, 78, 48, 44, 144, 144),
                                                                  (5, 60, 61, 16, 64, 48, 64)])
def test_conv3x3_narrow_tile_and_pixel_pitch(H, gpu_device, B, Hh, Ww, Cin, Cout, pitch_in, pitch_out):
    """Implicit 3x3 convolution with a NARROW output (N = 48 / 64: the 128 x 64 tile of the packed-B kernel) reading a
    cv_c-channel column slice of a wider channels-last buffer in place (lda = pixel pitch) and writing a column slice of
    another (ldc): the down-scaler's 128 -> 42, 42 -> 42, 42 -> 44 convolutions (layers.py:497-507) on padded segments."""
    from galerkin_transformer import ops
    dev = gpu_device
    T = B * Hh * Ww
    CP = (Cout + 15) // 16 * 16
    xin = rnd(T, pitch_in, dev=dev, seed=401)
    w = rnd(Cout, Cin, 3, 3, dev=dev, seed=402, scale=0.2)
    off = pitch_in - Cin                                          # the slice sits at the END of the wide rows
    wf = ops._conv_k_order(ops._pad_filter(w, CP, Cin))
    out = torch.full((T, pitch_out), float("nan"), device=dev)
    name = H.gemm_kernel_name(xin[:, off:], wf, T, CP, 9 * Cin, lda=pitch_in, ldb=9 * Cin, ldc=pitch_out, precision="bf16x3")
    H.gemm(xin[:, off:], wf, out[:, :CP], T, CP, 9 * Cin, lda=pitch_in, ldb=9 * Cin, ldc=pitch_out, conv=(Hh, Ww, Cin),
           precision="bf16x3")
    torch.cuda.synchronize()
    ref = _ref_conv(xin[:, off:off + Cin].reshape(B, Hh, Ww, Cin), w).reshape(T, Cout)
    assert rel_l2(out[:, :Cout], ref) < X3_TOL["bf16x3"]
    assert torch.equal(out[:, Cout:CP], torch.zeros(T, CP - Cout, device=dev))          # padding columns: exact zeros
    assert torch.isnan(out[:, CP:]).all()                                                # nothing written past the segment


@pytest.mark.parametrize("B", [3, 1])          # 18 252 / 6 084 pixel rows (round 5: the chain runs from 1 024 rows; a partial last tile)
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_scaler_conv_chain_matches_conv2d(H, gpu_device, p_drop, B):
    """ops.scaler_conv_chain (three implicit GEMMs into one padded buffer, ReLU + dropout on the epilogue, in-place
    gradient accumulation through the chain) == relu(drop(conv)) x 3 + cat with torch's conv2d in fp64 (p = 0); with
    dropout on, the kept entries equal the scaled reference, ~p of the positive entries are dropped, and the backward
    is the gradient of exactly that masked function."""
    from galerkin_transformer import ops
    dev = gpu_device
    Hh, Ww, C0 = 78, 78, 128
    widths = (42, 42, 44)
    x0 = rnd(B, Hh, Ww, C0, dev=dev, seed=411).requires_grad_(True)
    ws = [rnd(co, ci, 3, 3, dev=dev, seed=412 + i, scale=0.1).requires_grad_(True)
          for i, (co, ci) in enumerate(zip(widths, (C0,) + widths[:2]))]
    H.set_seed(77, dev)
    buf = ops.scaler_conv_chain(x0, *ws, p_drop=p_drop, training=True)
    CP = buf.shape[-1] // 3
    assert CP == 48
    got = [buf[..., i * CP:i * CP + widths[i]] for i in range(3)]
    for i in range(3):
        assert torch.equal(buf[..., i * CP + widths[i]:(i + 1) * CP], torch.zeros_like(buf[..., i * CP + widths[i]:(i + 1) * CP]))
    cot = rnd(*buf.shape, dev=dev, seed=419)               # also on the padding columns: must not matter
    buf.backward(cot)
    torch.cuda.synchronize()
    # reference in fp64 with the masks the run drew (read back from its own outputs: kept <=> output > 0 or pre <= 0)
    xr = x0.detach().double().requires_grad_(True)
    wr = [w.detach().double().requires_grad_(True) for w in ws]
    scale = 1.0 / (1.0 - p_drop)
    cur, refs = xr, []
    for i in range(3):
        pre = torch.nn.functional.conv2d(cur.permute(0, 3, 1, 2), wr[i], padding=1).permute(0, 2, 3, 1)
        # the run's own decisions (output > 0 <=> kept by the dropout and positive) are replayed: among ~1e6 ReLUs some
        # pre-activation lies within fp32 rounding of zero, and ONE differing decision moves a gradient by ~1e-3
        assert int(((got[i] > 0) & (pre < -1e-5)).sum()) == 0 and (p_drop > 0 or int(((got[i] <= 0) & (pre > 1e-5)).sum()) == 0)
        cur = pre * (got[i] > 0).double() * scale
        refs.append(cur)
        if p_drop > 0:
            pos = pre > 1e-6
            frac = 1.0 - float((got[i][pos] > 0).double().mean())
            assert abs(frac - p_drop) < (0.01 if B > 1 else 0.02), frac
    rcat = torch.cat(refs, -1)
    rcot = torch.cat([cot[..., i * CP:i * CP + widths[i]] for i in range(3)], -1).double()
    rcat.backward(rcot)
    for i in range(3):
        assert rel_l2(got[i], refs[i]) < 3e-6, i
        assert rel_l2(ws[i].grad, wr[i].grad) < 5e-6, i
    assert rel_l2(x0.grad, xr.grad) < 5e-6


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_scaler_chain_with_masked_segment_resize_matches_reference(H, gpu_device, p_drop):
    """The down-scaler's production combination (layers.py Interp2dEncoder.forward): scaler_conv_chain(grad_masked=True)
    -> bilinear_resize_seg(relu_input=True, act="relu"), i.e. the in_gate branch of resize_nhwc_bwd_kernel handing the
    chain a gradient that is already ReLU-masked, against conv2d x 3 + cat + F.interpolate(bilinear, align_corners) + ReLU
    in fp64 (reference layers.py:497-512) -- at the tolerance of the other down-scaler tests.  Also: the gradient autograd
    hands the chain is left untouched (retain_grad / hooks on the chain's output see the true gradient)."""
    from galerkin_transformer import ops
    dev = gpu_device
    B, Hh, Ww, C0, Ho, Wo = 3, 78, 78, 128, 43, 43
    widths = (42, 42, 44)
    x0 = rnd(B, Hh, Ww, C0, dev=dev, seed=451).requires_grad_(True)
    ws = [rnd(co, ci, 3, 3, dev=dev, seed=452 + i, scale=0.1).requires_grad_(True)
          for i, (co, ci) in enumerate(zip(widths, (C0,) + widths[:2]))]
    H.set_seed(79, dev)
    buf = ops.scaler_conv_chain(x0, *ws, p_drop=p_drop, training=True, grad_masked=True)
    buf.retain_grad()
    seen = []
    buf.register_hook(lambda gr: seen.append(gr.clone()))
    CP = buf.shape[-1] // 3
    y = ops.bilinear_resize_seg(buf, sum(widths), (Ho, Wo), widths[0], CP, act="relu", relu_input=True)
    cot = rnd(*y.shape, dev=dev, seed=459)
    y.backward(cot)
    torch.cuda.synchronize()
    assert len(seen) == 1 and torch.equal(buf.grad, seen[0])          # nobody wrote into the handed-over gradient
    got = [buf[..., i * CP:i * CP + widths[i]] for i in range(3)]
    xr = x0.detach().double().requires_grad_(True)
    wr = [w.detach().double().requires_grad_(True) for w in ws]
    scale = 1.0 / (1.0 - p_drop)
    cur, refs = xr, []
    for i in range(3):
        pre = torch.nn.functional.conv2d(cur.permute(0, 3, 1, 2), wr[i], padding=1).permute(0, 2, 3, 1)
        assert int(((got[i] > 0) & (pre < -1e-5)).sum()) == 0 and (p_drop > 0 or int(((got[i] <= 0) & (pre > 1e-5)).sum()) == 0)
        cur = pre * (got[i] > 0).double() * scale              # the run's own ReLU / dropout decisions, replayed
        refs.append(cur)
    rcat = torch.cat(refs, -1).permute(0, 3, 1, 2)
    ry = torch.relu(torch.nn.functional.interpolate(rcat, size=(Ho, Wo), mode="bilinear", align_corners=True)).permute(0, 2, 3, 1)
    ry.backward(cot.double())
    assert rel_l2(y, ry) < 3e-6
    for i in range(3):
        assert rel_l2(ws[i].grad, wr[i].grad) < 5e-6, i
    assert rel_l2(x0.grad, xr.grad) < 5e-6
    # the gradient handed over is the masked one: zero wherever the chain's output is not positive
    assert torch.equal(buf.grad[buf.detach() <= 0], torch.zeros_like(buf.grad[buf.detach() <= 0]))


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("B,Cin,Cout,n,size,p_drop", [(2, 1, 192, 141, 0.51, 0.05), (2, 1, 40, 29, (16, 16), 0.0),
                                                      (1, 3, 24, 9, (25, 21), 0.2), (2, 2, 8, 6, (1, 4), 0.0)])
def test_conv3x3_resize_silu(H, gpu_device, B, Cin, Cout, n, size, p_drop, nhwc):
    """gt_conv3x3_resize_* with act = GT_ACT_SILU (ABI v20; reference Interp2dEncoder with its default activation_type='silu',
    layers.py:446-456, 483-495 -- ex3's down-scaler): silu(resize(silu(dropout(conv3x3(x))))) in one pass and its weight
    gradient (both activations re-evaluated in the backward) against float64 torch with the dropout mask the stand-alone
    gt_dropout_apply draws for the same (seed, salt) on the channels-first convolution output."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    dev = gpu_device
    x = rnd(B, Cin, n, n + 2, dev=dev, seed=460)
    w = rnd(Cout, Cin, 3, 3, dev=dev, seed=461, scale=0.5)
    H.set_seed(778, dev)
    H._salt[0] = 11
    wg = w.clone().requires_grad_(True)
    y = ops.conv3x3_resize(x, wg, size, p_drop, True, out_nhwc=nhwc, act="silu")
    yc = y.permute(0, 3, 1, 2) if nhwc else y
    cot = rnd(*yc.shape, dev=dev, seed=462)
    yc.backward(cot)
    torch.cuda.synchronize()
    # the mask of the fused pass = what gt_dropout_apply gives a ones tensor of the conv output's shape with the same salt
    keep = torch.ones(B, Cout, n, n + 2, device=dev)
    if p_drop > 0:
        keep = H.dropout_apply(keep, H.dropout_desc(p_drop, 11, dev))
        assert abs(float((keep == 0).float().mean()) - p_drop) < 0.02
    xr, wr = x.double(), w.double().requires_grad_(True)
    y0 = F.silu(F.conv2d(xr, wr, padding=1) * keep.double())
    ref = F.silu(F.interpolate(y0, size=tuple(yc.shape[2:]), mode="bilinear", align_corners=True))
    (gw,) = torch.autograd.grad(ref, wr, cot.double())
    assert rel_l2(yc, ref) < 3e-6
    assert rel_l2(wg.grad, gw) < 1e-5


@pytest.mark.parametrize("p_drop", [0.0, 0.05])
@pytest.mark.parametrize("B,Hh,C0,widths,Ho", [(2, 71, 192, (64, 64, 64), 36), (3, 78, 128, (42, 42, 44), 43)])
def test_scaler_chain_silu_with_factor_resize_matches_reference(H, gpu_device, p_drop, B, Hh, C0, widths, Ho):
    """The SiLU form of the down-scaler's production combination (round 6; reference Interp2dEncoder.forward, layers.py:497-512,
    with activation_type='silu' -- ex3): scaler_conv_chain(act='silu', grad_masked=True) -> bilinear_resize_seg(act='silu',
    in_factor=fac), i.e. GT_ACT_DROP_SILU epilogues (dropout in front of the SiLU, keepscale * silu' left in `fac`), the
    GT_AUX_MUL data-gradient epilogues and the multiplicative in-gate of the segment resize, against conv2d x 3 + cat +
    F.interpolate + SiLU in float64 with the dropout masks the run drew (fac != 0)."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    dev = gpu_device
    Ww = Hh
    x0 = rnd(B, Hh, Ww, C0, dev=dev, seed=471).requires_grad_(True)
    ws = [rnd(co, ci, 3, 3, dev=dev, seed=472 + i, scale=0.1).requires_grad_(True)
          for i, (co, ci) in enumerate(zip(widths, (C0,) + widths[:2]))]
    H.set_seed(81, dev)
    buf, fac = ops.scaler_conv_chain(x0, *ws, p_drop=p_drop, training=True, grad_masked=True, act="silu")
    assert not fac.requires_grad
    buf.retain_grad()
    CP = buf.shape[-1] // 3
    y = ops.bilinear_resize_seg(buf, sum(widths), (Ho, Ho), widths[0], CP, act="silu", in_factor=fac)
    cot = rnd(*y.shape, dev=dev, seed=479)
    y.backward(cot)
    torch.cuda.synchronize()
    for i in range(3):          # padding columns: exact zeros in the buffer
        assert torch.equal(buf[..., i * CP + widths[i]:(i + 1) * CP], torch.zeros_like(buf[..., i * CP + widths[i]:(i + 1) * CP]))
    xr = x0.detach().double().requires_grad_(True)
    wr = [w.detach().double().requires_grad_(True) for w in ws]
    scale = 1.0 / (1.0 - p_drop)
    cur, refs = xr, []
    for i in range(3):
        keep = (fac[..., i * CP:i * CP + widths[i]] != 0).double()
        if p_drop > 0:
            assert abs(1.0 - float(keep.mean()) - p_drop) < 0.01
        else:
            assert bool(keep.all())
        pre = F.conv2d(cur.permute(0, 3, 1, 2), wr[i], padding=1).permute(0, 2, 3, 1)
        cur = F.silu(pre * keep * scale)
        refs.append(cur)
        assert rel_l2(buf[..., i * CP:i * CP + widths[i]], cur) < 3e-6, i
    rcat = torch.cat(refs, -1).permute(0, 3, 1, 2)
    ry = F.silu(F.interpolate(rcat, size=(Ho, Ho), mode="bilinear", align_corners=True)).permute(0, 2, 3, 1)
    ry.backward(cot.double())
    assert rel_l2(y, ry) < 4e-6                 # (f16x2: 1.9e-6; bf16x3, three chained convolutions: 3.0e-6)
    for i in range(3):
        assert rel_l2(ws[i].grad, wr[i].grad) < 5e-6, i
    assert rel_l2(x0.grad, xr.grad) < 5e-6


def test_scaler_chain_silu_unmasked_gradient(H, gpu_device):
    """scaler_conv_chain(act='silu') consumed directly (grad_masked=False): its backward applies the factor itself."""
    import torch.nn.functional as F
    from galerkin_transformer import ops
    dev = gpu_device
    B, Hh, C0, widths = 1, 40, 96, (32, 32, 32)
    x0 = rnd(B, Hh, Hh, C0, dev=dev, seed=481).requires_grad_(True)
    ws = [rnd(co, ci, 3, 3, dev=dev, seed=482 + i, scale=0.1).requires_grad_(True)
          for i, (co, ci) in enumerate(zip(widths, (C0,) + widths[:2]))]
    buf, fac = ops.scaler_conv_chain(x0, *ws, p_drop=0.0, training=True, act="silu")
    cot = rnd(*buf.shape, dev=dev, seed=489)
    buf.backward(cot)
    xr = x0.detach().double().requires_grad_(True)
    wr = [w.detach().double().requires_grad_(True) for w in ws]
    cur, refs = xr, []
    for i in range(3):
        cur = F.silu(F.conv2d(cur.permute(0, 3, 1, 2), wr[i], padding=1).permute(0, 2, 3, 1))
        refs.append(cur)
    rcat = torch.cat(refs, -1)
    rcat.backward(cot.double())
    assert rel_l2(buf, rcat) < 3e-6 and rel_l2(x0.grad, xr.grad) < 5e-6
    for i in range(3):
        assert rel_l2(ws[i].grad, wr[i].grad) < 5e-6, i


def test_resize_seg_equals_dense_resize(H, gpu_device):
    """gt_bilinear2d_seg_fwd/bwd (the last resize of the down-scaler reading the padded three-segment buffer) == the dense
    channels-last resize of the gathered real channels, forward and backward (padding columns of dx: zero)."""
    from galerkin_transformer import ops
    dev = gpu_device
    B, Hi, Wi, Ho, Wo, seg, segp, Cc = 2, 78, 78, 43, 43, 42, 48, 128
    buf = rnd(B, Hi, Wi, 3 * segp, dev=dev, seed=431)
    cols = list(range(0, 42)) + list(range(48, 90)) + list(range(96, 140))
    dense = buf[..., cols].contiguous().requires_grad_(True)
    bufg = buf.clone().requires_grad_(True)
    y1 = ops.bilinear_resize_seg(bufg, Cc, (Ho, Wo), seg, segp, act="relu")
    y2 = ops.bilinear_resize(dense, (Ho, Wo), in_nhwc=True, out_nhwc=True, act="relu")
    assert torch.equal(y1, y2)
    cot = rnd(B, Ho, Wo, Cc, dev=dev, seed=432)
    y1.backward(cot); y2.backward(cot)
    assert torch.equal(bufg.grad[..., cols], dense.grad)
    pad = [c for c in range(3 * segp) if c not in cols]
    assert torch.equal(bufg.grad[..., pad], torch.zeros_like(bufg.grad[..., pad]))


def test_conv3x3_resize_channels_last_output(H, gpu_device):
    """gt_conv3x3_resize_fwd_nhwc / _bwd_nhwc == the channels-first fused conv0 + resize, transposed (same dropout mask)."""
    from galerkin_transformer import ops
    dev = gpu_device
    x = rnd(3, 1, 141, 141, dev=dev, seed=441)
    res = []
    for nhwc in (False, True):
        w = rnd(128, 1, 3, 3, dev=dev, seed=442).requires_grad_(True)
        H.set_seed(5, dev)
        H._salt[0] = 11
        y = ops.conv3x3_resize(x, w, 0.555, p_drop=0.05, training=True, out_nhwc=nhwc)
        cot = rnd(3, 128, 78, 78, dev=dev, seed=443)
        y.backward(cot.permute(0, 2, 3, 1).contiguous() if nhwc else cot)
        res.append((y.permute(0, 3, 1, 2) if nhwc else y, w.grad))
    assert torch.equal(res[0][0], res[1][0])
    assert rel_l2(res[1][1], res[0][1]) < 1e-6


@pytest.mark.parametrize("Cin,p_drop,n,scale", [(1, 0.05, 141, 0.555), (1, 0.0, 141, 0.555), (2, 0.1, 64, 0.5), (3, 0.05, 33, 0.75)])
def test_conv3x3_resize_recorded_decisions(H, gpu_device, Cin, p_drop, n, scale):
    """relu_bits of gt_conv3x3_resize_*_nhwc: with the forward's decisions recorded (4 bits per output pixel and channel) the
    backward re-evaluates neither the convolution nor the dropout mask and does not read y; same forward bits, same weight
    gradient as the re-evaluating backward up to the round-off of one reassociated product (the re-evaluating path is held to
    the unfused operators and to fp64 by test_conv3x3_resize_fused_equals_unfused / _channels_last_output)."""
    from galerkin_transformer import ops
    dev = gpu_device
    x = rnd(2, Cin, n, n, dev=dev, seed=451)
    cot = rnd(2, int(n * scale), int(n * scale), 64, dev=dev, seed=453)
    cot[0, :5] = 0.0
    res = []
    old = ops._crb_bits[0]
    try:
        for bits in (True, False):
            ops._crb_bits[0] = bits
            w = rnd(64, Cin, 3, 3, dev=dev, seed=452).requires_grad_(True)
            H.set_seed(7, dev)
            H._salt[0] = 21
            y = ops.conv3x3_resize(x, w, scale, p_drop=p_drop, training=True, out_nhwc=True)
            y.backward(cot)
            res.append((y.detach(), w.grad.detach()))
    finally:
        ops._crb_bits[0] = old
    assert torch.equal(res[0][0], res[1][0])
    assert rel_l2(res[0][1], res[1][1]) < 1e-6
    assert float(res[0][1].abs().max()) > 0


@pytest.mark.parametrize("B,Hh,Ww,Cin,ldx,ldg,alpha", [
    (2, 77, 77, 128, 128, -128, 1.0),       # the up-scaler's 128 -> 128 convolution (Cout = 128: blocks of 64 x 32 channels)
    (3, 78, 78, 128, 128, 144, 1.0),        # conv1 of the down-scaler: dense 128-channel input, gy = a segment of [.., 144]
    (2, 78, 78, 48, 144, 96, 1.0 / 0.9),    # conv2 / conv3: both operands column segments (pitches 144 / 96), dropout scale
    (5, 9, 80, 16, 16, 48, 1.0),            # one input tile, the widest row the LDS rows hold, few image rows
    (2, 20, 37, 32, 36, 48, -2.0),          # odd width, pitch > channels
    (1, 3, 5, 48, 48, 48, 1.0),             # tiny image: every row and column touches the zero padding
    (2, 21, 114, 128, 128, 144, 1.0),       # C3 (211 x 211): the down-scaler's 114-pixel rows = two x-segments of 57
    (1, 17, 113, 128, 128, -128, 1.0),      # C3: the up-scaler's 113 x 113, 128 -> 128
    (1, 6, 243, 48, 48, 48, 1.0),           # four segments (61 pixels each), narrow chain
    (2, 9, 81, 16, 16, 48, 1.0),            # one pixel over a segment: 41 + 40
])
@pytest.mark.parametrize("prec", ["bf16x3", "f16x2"])
def test_conv3x3_wgrad_nhwc_matches_conv2d(H, gpu_device, B, Hh, Ww, Cin, ldx, ldg, alpha, prec):
    """gt_conv3x3_wgrad_nhwc (gt_convw.hip: operands split once per block into LDS planes, pixel-interleaved k, nine taps
    co-resident, sign-alternating accumulation) against the weight gradient of torch's conv2d in fp64 -- the reference's
    autograd path for Interp2dEncoder's conv1 / conv2 / conv3 (libs/layers.py:463-482, 88-150).  Operands are read in place
    out of wider channels-last buffers (pixel pitches ldx / ldg); columns beyond the used ones hold NaN-free garbage that
    must not enter."""
    dev = gpu_device
    Cout, T = (48, B * Hh * Ww) if ldg > 0 else (-ldg, B * Hh * Ww)
    ldg = abs(ldg)
    xbuf = rnd(T, ldx, dev=dev, seed=611)
    gbuf = rnd(T, ldg, dev=dev, seed=612)
    off_x, off_g = (ldx - Cin) // 4 * 4, (ldg - Cout) // 4 * 4      # 16-byte aligned column offsets inside the buffers
    xv, gv = xbuf[:, off_x:off_x + Cin], gbuf[:, off_g:off_g + Cout]
    # (the fp16 arithmetic keeps one running exponent per operand and block: a tenfold ramp over the image rows moves it)
    ramp = torch.logspace(0, 1, Hh, device=dev).repeat_interleave(Ww).repeat(B).unsqueeze(1)
    xbuf, gbuf = xbuf * ramp, gbuf * ramp.flip(0)
    xv, gv = xbuf[:, off_x:off_x + Cin], gbuf[:, off_g:off_g + Cout]
    dw = H.conv3x3_wgrad_nhwc(gv, ldg, xv, ldx, B, Hh, Ww, Cin, Cout, alpha=alpha, precision=prec)
    torch.cuda.synchronize()
    xr = xv.double().reshape(B, Hh, Ww, Cin).permute(0, 3, 1, 2).contiguous()
    gr = gv.double().reshape(B, Hh, Ww, Cout).permute(0, 3, 1, 2).contiguous()
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=dev, requires_grad=True)
    torch.nn.functional.conv2d(xr, w, padding=1).backward(gr)
    ref = alpha * w.grad
    assert dw.shape == ref.shape
    assert rel_l2(dw, ref) < KTOL, rel_l2(dw, ref)
    # every tap on its own (a transposed / mirrored tap order would pass a norm over all taps only by accident)
    for ky in range(3):
        for kx in range(3):
            assert rel_l2(dw[:, :, ky, kx], ref[:, :, ky, kx]) < 2 * KTOL, (ky, kx)
    # deterministic
    dw2 = H.conv3x3_wgrad_nhwc(gv, ldg, xv, ldx, B, Hh, Ww, Cin, Cout, alpha=alpha, precision=prec)
    assert torch.equal(dw, dw2)


def test_conv3x3_wgrad_nhwc_rejects_what_it_does_not_cover(H, gpu_device):
    dev = gpu_device
    x, g = rnd(2 * 8 * 8, 16, dev=dev, seed=621), rnd(2 * 8 * 8, 48, dev=dev, seed=622)
    with pytest.raises(H.GtNotSupported):
        H.conv3x3_wgrad_nhwc(g[:, :32], 48, x, 16, 2, 8, 8, 16, 32)          # Cout != 48
    with pytest.raises(H.GtNotSupported):
        H.conv3x3_wgrad_nhwc(g, 48, x[:, :8], 16, 2, 8, 8, 8, 48)            # Cin % 16
    xw, gw = rnd(1 * 2 * 96, 16, dev=dev, seed=623), rnd(1 * 2 * 96, 48, dev=dev, seed=624)
    dw = H.conv3x3_wgrad_nhwc(gw, 48, xw, 16, 1, 2, 96, 16, 48)              # W > 80: two x-segments since round 5
    assert tuple(dw.shape) == (48, 16, 3, 3) and bool(torch.isfinite(dw).all())


@pytest.mark.parametrize("N,K", [(128, 128), (256, 128), (128, 384), (384, 128)])
def test_gemm_f16x2_dynamic_row_scaling(H, gpu_device, N, K):
    """GT_PREC_F16X2 on the packed-B kernel (two fp16 terms per operand, three products, per-row running exponent on the
    activation side, per-tile exponent on the packed weight): rows spanning ten decades of magnitude, rows that grow or shrink
    a thousandfold along K (the accumulator is rescaled in flight), zero rows and a zero stage -- every ROW of the product must
    be fp32-class accurate relative to its own scale, and identical inputs give identical bits."""
    dev = gpu_device
    M = 20000                                  # >= 16384: the packed-B kernel
    g = torch.Generator().manual_seed(700 + N + K)
    A = torch.randn(M, K, generator=g)
    A *= 10.0 ** (torch.rand(M, 1, generator=g) * 10.0 - 6.0)                  # row magnitudes 1e-6 .. 1e4
    ramp = torch.logspace(0, 3, K).unsqueeze(0)
    A[1000:2000] *= ramp                                                       # growing along K: exponent drops in flight
    A[2000:3000] *= ramp.flip(1)                                               # shrinking along K
    A[3000:3100] = 0.0
    A[3100:3200, :16] = 0.0                                                    # an all-zero first stage
    A[3200:3300, 32:] = 0.0                                                    # nothing after the second stage
    B = torch.randn(N, K, generator=g) * 0.05
    B[:32] *= 1e-4                                                             # one fragment tile of tiny weights
    B[32:64] *= 1e3
    Ad, Bd = A.to(dev), B.to(dev)
    ref = A.double() @ B.double().t()
    scale = A.double().abs() @ B.double().abs().t()                           # the un-cancelled magnitude of every output
    C = torch.empty(M, N, device=dev)
    H.gemm(Ad, Bd, C, M, N, K, lda=K, ldb=K, ldc=N, precision="f16x2")
    torch.cuda.synchronize()
    assert "gemm_x3h_kernel" in H.gemm_kernel_name(Ad, Bd, M, N, K, lda=K, ldb=K, ldc=N, precision="f16x2")
    err = (C.double().cpu() - ref).abs() / scale.clamp_min(1e-300)
    err[scale == 0] = (C.double().cpu()[scale == 0]).abs()
    assert float(err.max()) < 2e-6, float(err.max())                          # every element, relative to sum |a||b|
    assert float(err.pow(2).mean().sqrt()) < 1e-7
    row_err = (C.double().cpu() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
    assert float(row_err[ref.norm(dim=1) > 0].max()) < 2e-6
    assert torch.equal(C[3000:3100], torch.zeros_like(C[3000:3100]))
    C2 = torch.empty(M, N, device=dev)
    H.gemm(Ad, Bd, C2, M, N, K, lda=K, ldb=K, ldc=N, precision="f16x2")
    assert torch.equal(C, C2)
    # the same product in the default arithmetic, for scale
    C3 = torch.empty(M, N, device=dev)
    H.gemm(Ad, Bd, C3, M, N, K, lda=K, ldb=K, ldc=N, precision="bf16x3")
    err3 = (C3.double().cpu() - ref).abs() / scale.clamp_min(1e-300)
    print("f16x2 rms %.2e max %.2e | bf16x3 rms %.2e max %.2e" % (float(err.pow(2).mean().sqrt()), float(err.max()),
                                                                    float(err3.pow(2).mean().sqrt()), float(err3.max())))


def test_gemm_f16x2_tiny_magnitudes_have_no_power_of_two_cliff(H, gpu_device):
    """the un-scale exponent -(row exponent + tile exponent) used to be clamped to [-126, 126]; with row amax x tile
    amax below ~2^-100 the result came out a power of two too large.  Rows at 1e-30, 1e-34 and 1e-37 against weights at 1e-3
    and 1e-6: every row fp32-class relative to its own scale (results down to ~1e-43 are subnormal: absolute bound there)."""
    dev = gpu_device
    M, N, K = 16384 + 256, 128, 128
    g = torch.Generator().manual_seed(4242)
    A = torch.randn(M, K, generator=g)
    A[:512] *= 1e-30
    A[512:1024] *= 1e-34
    A[1024:1536] *= 1e-37
    Bm = torch.randn(N, K, generator=g) * 1e-3
    Bm[:32] *= 1e-3
    Ad, Bd = A.to(dev), Bm.to(dev)
    ref = A.double() @ Bm.double().t()
    C = torch.empty(M, N, device=dev)
    H.gemm(Ad, Bd, C, M, N, K, lda=K, ldb=K, ldc=N, precision="f16x2")
    torch.cuda.synchronize()
    assert "gemm_x3h_kernel" in H.gemm_kernel_name(Ad, Bd, M, N, K, lda=K, ldb=K, ldc=N, precision="f16x2")
    got = C.double().cpu()
    for lo, hi in ((0, 512), (512, 1024), (1024, 1536), (1536, M)):
        r, c = ref[lo:hi], got[lo:hi]
        scale = A[lo:hi].double().abs() @ Bm.double().abs().t()    # un-cancelled magnitude of every output
        # fp32-class relative to sum |a||b|, plus a few subnormal steps (1.4e-45) where the result itself is subnormal
        assert bool(((c - r).abs() <= 2e-6 * scale + 6e-45).all()), (lo, hi, float(((c - r).abs() / scale.clamp_min(1e-300)).max()))
        if float(r.abs().max()) > 1e-36:                           # not a power of two off: the norms agree
            assert abs(float(c.norm() / r.norm()) - 1.0) < 1e-4, (lo, hi, float(c.norm() / r.norm()))


@pytest.mark.parametrize("kernel", ["gemm_x3w", "convw"])
def test_token_contracted_f16x2_per_column_dynamic_range(H, gpu_device, kernel):
    """ADVICE r4 / VERDICT r5 next-round 8: the per-COLUMN accuracy of the two-term fp16 weight-gradient kernels when the
    features of one 128-block span many decades (gemm_x3w_kernel: dW = dY^T X of nn.Linear, reference layers.py:811,823,964,976
    backwards; gt_conv3x3_wgrad_nhwc: conv2d weight backward, layers.py:463-482).  Both keep ONE power-of-two exponent per
    operand and block, so a feature q decades below its block's loudest keeps about 22 - 3.32 q significant bits -- this test
    PINS that documented bound ("Numerical guarantees ... and their limits") as the expected value:
        rel. error of column c  <=  4 * 2^-22 * max(1, amax(block) / amax(c))           (measured per decade, printed)
    i.e. columns within ~1 decade of the loudest are fp32-class on their own, quieter ones lose relative (never absolute)
    accuracy linearly with the ratio, and GT_PREC_BF16X3 on the same operands has no such dependence (every column < 2e-6)."""
    dev = gpu_device
    g = torch.Generator().manual_seed(77)
    decades = torch.arange(0, 10)                      # column group j: scaled by 10^-j
    if kernel == "gemm_x3w":
        M, N, K = 128, 128, 40000                      # dW [M, N] = A^T B over K tokens; columns of B in groups of 12
        A = torch.randn(K, M, generator=g)
        B = torch.randn(K, N, generator=g)
        colscale = torch.ones(N)
        for j in decades:
            colscale[12 * j:12 * j + 12] = 10.0 ** (-float(j))
        B = B * colscale
        Ad, Bd = A.to(dev), B.to(dev)

        def run(prec):
            C = torch.empty(M, N, device=dev)
            H.gemm(Ad, Bd, C, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=0, precision=prec)
            return C.double().cpu()
        assert "gemm_x3w_kernel" in H.gemm_kernel_name(Ad, Bd, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N,
                                                       split_k=0, precision="f16x2")
        ref = A.double().t() @ B.double()
        col_err = lambda C: ((C - ref).norm(dim=0) / ref.norm(dim=0))
    else:
        Bn, Hh, Ww, Cin, Cout = 4, 40, 40, 128, 64     # dw [Cout, Cin, 3, 3]; input channels in groups of 12
        x = torch.randn(Bn, Hh, Ww, Cin, generator=g)
        gy = torch.randn(Bn, Hh, Ww, Cout, generator=g)
        colscale = torch.ones(Cin)
        for j in decades:
            colscale[12 * j:12 * j + 12] = 10.0 ** (-float(j))
        x = x * colscale
        xd, gd = x.to(dev), gy.to(dev)

        def run(prec):
            return H.conv3x3_wgrad_nhwc(gd.reshape(-1, Cout), Cout, xd.reshape(-1, Cin), Cin, Bn, Hh, Ww, Cin, Cout,
                                        precision=prec).double().cpu()
        xr = x.double().permute(0, 3, 1, 2)
        wr = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(xr, wr, padding=1).backward(gy.double().permute(0, 3, 1, 2))
        ref = wr.grad
        col_err = lambda C: ((C - ref).permute(1, 0, 2, 3).reshape(Cin, -1).norm(dim=1)
                             / ref.permute(1, 0, 2, 3).reshape(Cin, -1).norm(dim=1))
    e16, e3 = col_err(run("f16x2")), col_err(run("bf16x3"))
    table = {int(j): (float(e16[12 * j:12 * j + 12].max()), float(e3[12 * j:12 * j + 12].max())) for j in decades}
    print(kernel, "per-column rel. error by decades below the block's loudest feature (f16x2, bf16x3):", table)
    for j in decades:
        bound = 4.0 * 2.0 ** -22 * 10.0 ** float(j)
        assert table[int(j)][0] < bound, (kernel, int(j), table[int(j)], bound)
        assert table[int(j)][1] < 2e-6, (kernel, int(j), table[int(j)])
    assert table[0][0] < 2e-6 and table[1][0] < 1e-5              # the loud decade(s): fp32-class on their own


@pytest.mark.parametrize("B,Hh", [(16, 32), (22, 32), (40, 48), (64, 80)])
def test_conv3x3_wgrad_nhwc_workspace_contract(H, gpu_device, B, Hh):
    """gt_conv3x3_wgrad_nhwc_ws_bytes planned with the bf16 channel blocks while the fp16 launch could use
    more row chunks (Cout = 48, Cin % 64 == 0) and wrote past the advertised size.  A workspace of EXACTLY ws_bytes with a
    canary behind it, in both arithmetics; one byte less is refused."""
    import ctypes as C
    dev = gpu_device
    Ww, Cin, Cout = 40, 128, 48
    T = B * Hh * Ww
    x, gy = rnd(T, Cin, dev=dev, seed=801), rnd(T, Cout, dev=dev, seed=802)
    L = H.lib()
    need = int(L.gt_conv3x3_wgrad_nhwc_ws_bytes(B, Hh, Ww, Cin, Cout))
    assert need > 0 and need % 4 == 0
    res = {}
    for prec in ("f16x2", "bf16x3"):
        buf = torch.full((need // 4 + 4096,), 12345.0, device=dev)
        dw = torch.empty(Cout, Cin, 3, 3, device=dev)
        rc = L.gt_conv3x3_wgrad_nhwc(gy.data_ptr(), Cout, x.data_ptr(), Cin, dw.data_ptr(), B, Hh, Ww, Cin, Cout, 1.0,
                                     H.PREC_CODE[prec], buf.data_ptr(), need, H.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (prec, rc)
        assert bool((buf[need // 4:] == 12345.0).all()), f"{prec}: wrote past gt_conv3x3_wgrad_nhwc_ws_bytes"
        res[prec] = dw
        rc = L.gt_conv3x3_wgrad_nhwc(gy.data_ptr(), Cout, x.data_ptr(), Cin, dw.data_ptr(), B, Hh, Ww, Cin, Cout, 1.0,
                                     H.PREC_CODE[prec], buf.data_ptr(), 1024, H.stream_ptr())
        assert rc == -3, (prec, rc)                                # GT_EWS
    assert rel_l2(res["f16x2"], res["bf16x3"].double()) < 5e-6


def test_conv3x3_f16x2_matches_conv2d(H, gpu_device):
    """The implicit 3x3 convolution (forward and data gradient) in GT_PREC_F16X2 against torch's conv2d in fp64."""
    from galerkin_transformer import ops
    dev = gpu_device
    old = H.set_precision("f16x2")
    try:
        x = rnd(4, 77, 77, 128, dev=dev, seed=801).requires_grad_(True)
        w = rnd(128, 128, 3, 3, dev=dev, seed=802, scale=0.05).requires_grad_(True)
        y = ops.conv3x3_nhwc(x, w)
        cot = rnd(*y.shape, dev=dev, seed=803)
        y.backward(cot)
        torch.cuda.synchronize()
    finally:
        H.set_precision(old)
    xr, wr = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr.permute(0, 3, 1, 2), wr, padding=1).permute(0, 2, 3, 1)
    yr.backward(cot.double())
    assert rel_l2(y, yr) < KTOL and rel_l2(x.grad, xr.grad) < KTOL and rel_l2(w.grad, wr.grad) < KTOL


@pytest.mark.parametrize("prec", ["bf16x3", "f16x2"])
def test_packed_gemm_repeat_launch_bitwise(H, gpu_device, prec):
    """The packed-B kernels order their loads with COUNTED waits (inline-asm fragment loads, vmcnt(N) + barrier): a miscount
    shows up as a few rows of one launch in several differing from run to run, not as a wrong mean.  Forty back-to-back
    launches of the three hot instances -- QKV + head-norm epilogue on plain tiles, a plain token product, the implicit 3x3
    convolution -- must all return the bits of the first one.  (Round 4: a refactoring of the kernel body made exactly the
    head-norm launch flicker, 16 rows of one head in one launch out of four, with an unchanged instruction stream around
    the waits; this test is what keeps that from coming back unnoticed.)"""
    dev = gpu_device
    B, n, d, h, p = 18, 1849, 128, 4, 2
    T, dk = B * n, d // h
    DP = H.round4(dk + p)
    x, pos = rnd(T, d, dev=dev, seed=901), rnd(T, p, dev=dev, seed=902)
    wq, bq = rnd(3 * d, d, dev=dev, seed=903, scale=0.1), rnd(3 * d, dev=dev, seed=904, scale=0.1)
    gamma, beta = torch.ones(2, h, dk, device=dev), torch.zeros(2, h, dk, device=dev)
    w2 = rnd(256, d, dev=dev, seed=905, scale=0.1)
    img, wc = rnd(6, 77, 77, 128, dev=dev, seed=906), rnd(128, 9 * 128, dev=dev, seed=907, scale=0.05)

    def launch():
        out3 = torch.empty(3, T, h, DP, device=dev)
        stats = torch.empty(2, T, h, 2, device=dev)
        H.gemm(x, wq, None, T, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=bq, precision=prec,
               hn=dict(gamma=gamma, beta=beta, pos=pos, out=out3, stats=stats, h=h, dk=dk, p=p, norm_mask=6, eps=1e-7,
                       skip_raw=7, plain=True))
        y = torch.empty(T, 256, device=dev)
        H.gemm(x, w2, y, T, 256, d, lda=d, ldb=d, ldc=256, precision=prec)
        c = torch.empty(6 * 77 * 77, 128, device=dev)
        H.gemm(img.reshape(-1, 128), wc, c, 6 * 77 * 77, 128, 9 * 128, lda=128, ldb=9 * 128, ldc=128, conv=(77, 77, 128),
               precision=prec)
        return out3, stats, y, c

    first = launch()
    for _ in range(40):
        again = launch()
        for a, b in zip(first, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,K", [(128, 256, 33282), (384, 128, 20000), (256, 128, 236672),
                                   (192, 192, 40000), (576, 192, 33000), (192, 384, 20001), (160, 96, 17000),    # round 5: partial tiles (ex3: d = 192)
                                   (192, 64, 262144), (64, 128, 40000), (128, 64, 33000), (64, 64, 17000), (32, 96, 20000)])   # round 6: narrow models (ex1: d = 64)
def test_gemm_f16x2_weight_gradient_kernel(H, gpu_device, M, N, K):
    """gemm_x3w_kernel (GT_PREC_F16X2 token-contracted weight gradient: a stage of 32 tokens split once into fp16 planes in LDS,
    one running exponent per operand and block with in-flight accumulator rescaling, split-K slabs + fixed-order reduce,
    the bias gradient riding on it as column sums of A): against fp64, with magnitudes that change a thousandfold along the
    token axis (early blocks see small values, late blocks large ones; inside a block the exponent drops as the ramp climbs)."""
    dev = gpu_device
    g = torch.Generator().manual_seed(1200 + M + N)
    A = torch.randn(K, M, generator=g)
    B = torch.randn(K, N, generator=g)
    A *= torch.logspace(-3, 0, K).unsqueeze(1)                 # gradient-like: grows along the tokens
    B[: K // 3] *= 50.0
    Ad, Bd = A.to(dev), B.to(dev)
    C = torch.empty(M, N, device=dev)
    cs = torch.empty(M, device=dev)
    H.gemm(Ad, Bd, C, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=0, a_colsum=cs, precision="f16x2")
    torch.cuda.synchronize()
    assert "gemm_x3w_kernel" in H.gemm_kernel_name(Ad, Bd, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=0,
                                                   precision="f16x2")
    ref = Ad.double().t() @ Bd.double()
    scale = Ad.double().abs().t() @ Bd.double().abs()
    err = ((C.double() - ref).abs() / scale)
    assert float(err.max()) < 1e-6 and float(err.pow(2).mean().sqrt()) < 5e-8, (float(err.max()), float(err.pow(2).mean().sqrt()))
    assert rel_l2(C, ref) < KTOL
    assert rel_l2(cs, Ad.double().sum(0)) < KTOL
    C2, cs2 = torch.empty(M, N, device=dev), torch.empty(M, device=dev)
    H.gemm(Ad, Bd, C2, M, N, K, layout_a=1, layout_b=1, lda=M, ldb=N, ldc=N, split_k=0, a_colsum=cs2, precision="f16x2")
    assert torch.equal(C, C2) and torch.equal(cs, cs2)


# ---- gt_gemm's refusals: one descriptor per return site of the descriptor layer, each with ONE defect (then six with two, which
# pin the order of the checks).  Every pointer that is not itself the defect is a real tensor big enough for the shapes
# (M, N <= 256, K <= 512), so a descriptor accepted by mistake would run a small valid product, not a wild access.
# Base: fp32, la = lb = 0, M = N = 128, K = 64, split_k = 1.
_EINVAL, _EWS, _ENOTSUP = -1, -3, -4
_HN = dict(ep_mode=3, N=96, hn_h=1, hn_dk=32, hn_out=True, hn_gamma=True, hn_beta=True, hn_stats=True, hn_norm_mask=3, precision=1)
_HEAD = dict(n_out=1, w2=True, ldw2=128, out2=True, g2=True, dw2=True)
_CONV = dict(cv_h=8, cv_w=16, cv_c=16, K=144, lda=16, ldb=144, precision=1)                       # 128 pixels, 16 channels
_CONVW = dict(cv_h=8, cv_w=16, cv_c=16, cv_wgrad=1, layout_a=1, layout_b=1, M=64, N=16, K=128, lda=64, ldb=16, ldc=16, batch0=9,
              c_bs0=64 * 16, split_k=0, precision=1)
_K2 = dict(K2=16, A2=True, B2=True, lda2=16, ldb2=16)
_SPLIT4 = dict(K=512, lda=512, ldb=512, split_k=4)
_GEMM_REFUSALS = [
    ("null-c", dict(C=None), _EINVAL),
    ("layout-2", dict(layout_a=2), _EINVAL),
    ("ep-mode-7", dict(ep_mode=7), _EINVAL),
    ("headnorm-la1", dict(_HN, layout_a=1), _ENOTSUP),
    ("headnorm-wrong-n", dict(_HN, N=128), _EINVAL),
    ("headnorm-mask-no-stats", dict(_HN, hn_stats=None), _EINVAL),
    ("headnorm-act", dict(_HN, act=1), _ENOTSUP),
    ("headnorm-f32", dict(_HN, precision=0), _ENOTSUP),
    ("rowdot-n160", dict(_HEAD, ep_mode=1, N=160, ldc=160, ldw2=160), _ENOTSUP),
    ("rowdot-no-out2", dict(_HEAD, ep_mode=1, out2=None), _EINVAL),
    ("rowdot-lb1", dict(_HEAD, ep_mode=1, layout_b=1, ldb=128), _ENOTSUP),
    ("mlp-bwd-no-ws", dict(_HEAD, ep_mode=2, ws=None), _EWS),
    ("conv-k", dict(_CONV, K=128), _EINVAL),
    ("conv-c8", dict(_CONV, cv_c=8, K=72, lda=8, ldb=72), _ENOTSUP),
    ("conv-f32", dict(_CONV, precision=0), _ENOTSUP),
    ("convw-batch", dict(_CONVW, batch0=1), _EINVAL),
    ("convw-w8", dict(_CONVW, cv_h=16, cv_w=8), _ENOTSUP),
    ("rp-9", dict(rp=9, rp_a=True, rp_b=True, rp_lda=9, rp_ldb=9), _EINVAL),
    ("rp-no-a", dict(rp=2, rp_b=True, rp_lda=2, rp_ldb=2), _EINVAL),
    ("drop-no-seed", dict(drop=(0.1, False)), _EINVAL),
    ("drop-p1", dict(drop=(1.0, True)), _EINVAL),
    ("split4-bias", dict(_SPLIT4, bias=True), _ENOTSUP),
    ("split4-small-ws", dict(_SPLIT4, ws=1024), _EWS),
    ("k2-no-a2", dict(_K2, A2=None), _ENOTSUP),
    ("colsum-la0", dict(a_colsum=True), _ENOTSUP),
    ("c-masked-batch2", dict(c_masked=True, ldc_masked=128, batch0=2, a_bs0=128 * 64, c_bs0=128 * 128), _ENOTSUP),
    ("c-mask-p1", dict(c_masked=True, ldc_masked=128, c_mask=(1.0, True)), _EINVAL),
    ("aux-op-no-aux", dict(aux_op=1), _EINVAL),
    ("b-packed-not-packed", dict(b_packed=True), _EINVAL),
    ("precision-7", dict(precision=7), _EINVAL),
    ("act-gelu", dict(act=3), _EINVAL),
    ("batch-90000", dict(M=16, N=16, K=16, lda=16, ldb=16, ldc=16, batch0=300, batch1=300), _EINVAL),
    # two defects: the first check in the order of the descriptor layer answers
    ("rp-9+split4-bias", dict(_SPLIT4, bias=True, rp=9, rp_a=True, rp_b=True, rp_lda=9, rp_ldb=9), _EINVAL),     # not ENOTSUP
    ("precision-7+rp-9", dict(precision=7, rp=9, rp_a=True, rp_b=True, rp_lda=9, rp_ldb=9), _EINVAL),
    ("k2-no-a2+split4-small-ws", dict(_SPLIT4, **dict(_K2, A2=None), ws=1024), _ENOTSUP),                        # the plan, not EWS
    ("null-c+colsum-la0", dict(C=None, a_colsum=True), _EINVAL),                                                 # not ENOTSUP
    ("mlp-bwd-no-ws+lb1", dict(_HEAD, ep_mode=2, layout_b=1, ldb=128, ws=None), _EWS),                           # not ENOTSUP
    ("split4-small-ws+b-packed", dict(_SPLIT4, ws=1024, b_packed=True), _EWS),                                   # not EINVAL
]
_GEMM_PTRS = ("A", "B", "C", "A2", "B2", "bias", "res", "add", "pre", "aux", "rp_a", "rp_b", "a_colsum", "c_masked", "b_packed", "w2",
              "b2", "out2", "g2", "dw2", "hn_gamma", "hn_beta", "hn_pos", "hn_out", "hn_stats")


def gemm_refusal_rc(H, dev, fields, pool):
    """gt_gemm's return code for the base product with `fields` laid over it.  pool: name -> tensor, filled on demand."""
    import ctypes as C

    def buf(name, dtype=torch.float32):
        if name not in pool:
            pool[name] = torch.zeros(256 * 512, dtype=dtype, device=dev)        # the largest operand any case describes
        return pool[name]
    L = H.lib()
    d = H.GtGemmDesc()
    L.gt_gemm_desc_init(C.byref(d))
    f = dict(M=128, N=128, K=64, lda=64, ldb=64, ldc=128, A=True, B=True, C=True, ws=1 << 20)
    f.update(fields)
    ws = f.pop("ws")
    for k, v in f.items():
        if k in ("drop", "a_drop", "c_mask"):
            g = getattr(d, k)
            g.p, g.salt, g.seed = v[0], 5, buf("seed", torch.int64).data_ptr() if v[1] else None
        elif k in _GEMM_PTRS:
            setattr(d, k, buf(k).data_ptr() if v else None)
        else:
            setattr(d, k, v)
    wsp = buf("ws").data_ptr() if ws else None                        # 512 KiB of real scratch; `ws` = the size we admit to
    return L.gt_gemm(C.byref(d), wsp, min(ws or 0, 4 * 256 * 512), H.stream_ptr())


@pytest.fixture(scope="module")
def refusal_pool():
    return {}


@pytest.mark.parametrize("name,fields,want", _GEMM_REFUSALS, ids=[c[0] for c in _GEMM_REFUSALS])
def test_gemm_refusal_codes(H, gpu_device, refusal_pool, name, fields, want):
    """The code gt_gemm refuses a descriptor with is behaviour (the Python side falls back on GT_ENOTSUP only), and with two
    defects the order of the checks decides it."""
    assert gemm_refusal_rc(H, gpu_device, fields, refusal_pool) == want
    torch.cuda.synchronize()
