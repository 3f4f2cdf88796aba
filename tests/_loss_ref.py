"""WeightedL2Loss2d per-sample terms restated in numpy (the formulas of include/gt_hip.h, gt_h1loss2d_*), the float64 torch
oracle of the HIP route (``_terms_torch`` on the CPU) and the shared inputs of test_loss_hip_cpu.py / test_loss_hip_gpu.py."""
import functools

import numpy as np
import torch


def terms_np(P, T, G=None, K=None, *, d=2, h, beta=1.0, gamma=0.1, eps=1e-10):
    """(loss [N], reg [N] or None, L2 [N], H1 [N]) in the dtype of the inputs.  K: N n n values or None."""
    N, n, _ = P.shape
    s, m, M = d // 2, n - d, n * n
    L2 = (T ** 2).sum(axis=(1, 2)) / M + eps
    loss = beta * (((P - T) ** 2).sum(axis=(1, 2)) / M) / L2
    if G is None:
        return loss, None, L2, np.ones_like(L2)
    Kk = np.ones_like(P) if K is None else K.reshape(N, n, n)
    H1 = (Kk[..., None] * G ** 2).sum(axis=(1, 2, 3)) / M + eps
    Dx = (P[:, d:, s:n - s] - P[:, :m, s:n - s]) / (d * h)
    Dy = (P[:, s:n - s, d:] - P[:, s:n - s, :m]) / (d * h)
    Ki, Gi = Kk[:, s:n - s, s:n - s], G[:, s:n - s, s:n - s]
    R = ((Ki * (Gi[..., 0] - Dx)) ** 2 + (Ki * (Gi[..., 1] - Dy)) ** 2).sum(axis=(1, 2))
    return loss, gamma * h * (R / (2 * m * m)) / H1, L2, H1


def dpreds_np(P, T, G, K, L2, H1, gl, gr, *, d=2, h, beta=1.0, gamma=0.1):
    """The backward gather: dP[i, j] from the upstream gradients gl, gr [N] of loss and reg, pixel by pixel --
        dP[i,j] = gl beta 2 / (M L2) (P - T)[i,j]
                + gr gamma h 2 / (2 m^2 H1) / (d h) (r_x[i-d,j-s] - r_x[i,j-s] + r_y[i-s,j-d] - r_y[i-s,j])
    with r_c = K^2 (D_c P - G_c) on the interior index range [0, m)^2 and zero outside it."""
    N, n, _ = P.shape
    s, m, M = d // 2, n - d, n * n
    dP = (gl * beta * 2 / (M * L2))[:, None, None] * (P - T)
    if G is None or gr is None:
        return dP
    Kk = np.ones_like(P) if K is None else K.reshape(N, n, n)
    rx, ry = np.zeros((N, m, m), P.dtype), np.zeros((N, m, m), P.dtype)
    for i in range(m):
        for j in range(m):
            k2 = Kk[:, i + s, j + s] ** 2
            rx[:, i, j] = k2 * ((P[:, i + d, j + s] - P[:, i, j + s]) / (d * h) - G[:, i + s, j + s, 0])
            ry[:, i, j] = k2 * ((P[:, i + s, j + d] - P[:, i + s, j]) / (d * h) - G[:, i + s, j + s, 1])

    def at(r, i, j):
        return r[:, i, j] if 0 <= i < m and 0 <= j < m else 0.0

    c2 = gr * gamma * h * 2 / (2 * m * m * H1) / (d * h)
    for i in range(n):
        for j in range(n):
            dP[:, i, j] += c2 * (at(rx, i - d, j - s) - at(rx, i, j - s) + at(ry, i - s, j - d) - at(ry, i - s, j))
    return dP


@functools.lru_cache(maxsize=None)
def inputs(N, n, seed=0):
    """float32 CPU tensors (P, T, G, K [N,n,n,1], gl, gr): a prediction near its target (relative error ~ 0.3), a
    coefficient in [0.5, 1.5], upstream gradients in [0.5, 1.5].  Cached: callers must not write to them."""
    g = torch.Generator().manual_seed(1000 * n + 10 * N + seed)
    T = torch.randn(N, n, n, generator=g)
    P = T + 0.3 * torch.randn(N, n, n, generator=g)
    G = torch.randn(N, n, n, 2, generator=g) * n
    K = torch.rand(N, n, n, 1, generator=g) + 0.5
    gl, gr = torch.rand(N, generator=g) + 0.5, torch.rand(N, generator=g) + 0.5
    return P, T, G, K, gl, gr


def oracle64(lf, P, T, G=None, K=None, gl=None, gr=None, **kw):
    """``lf._terms_torch`` in float64 on the CPU from the given (any device, float32) inputs: dict(loss, reg, L2, H1, dP);
    dP is the gradient of (loss gl).sum() + (reg gr).sum() (gl, gr default to ones)."""
    f64 = lambda t: None if t is None else t.detach().double().cpu()
    p = f64(P).clone().requires_grad_(True)
    loss, reg, norms = lf._terms_torch(p, f64(T), targets_prime=f64(G), K=f64(K), **{k: f64(v) for k, v in kw.items()})
    total = (loss * (1.0 if gl is None else f64(gl))).sum()
    if reg is not None:
        total = total + (reg * (1.0 if gr is None else f64(gr))).sum()
    (dP,) = torch.autograd.grad(total, p)
    H1 = norms["H1"]
    return dict(loss=loss.detach(), reg=None if reg is None else reg.detach(), L2=norms["L2"].detach(),
                H1=H1.detach() if torch.is_tensor(H1) else H1, dP=dP)
