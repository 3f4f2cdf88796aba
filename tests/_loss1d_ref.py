"""WeightedL2Loss (1-D) per-sample terms restated in numpy (the formulas of include/gt_hip.h, gt_h1loss1d_*), the float64
torch oracle of the HIP route (``_terms_torch`` on the CPU) and the shared inputs of test_loss1d_hip_cpu.py /
test_loss1d_hip_gpu.py."""
import functools

import numpy as np
import torch


def terms_np(P, T, G=None, *, d=2, h, beta=1.0, gamma_h=0.0):
    """(loss [N], reg [N] or None, L2 [N], H1 [N]) in the dtype of the inputs.  gamma_h: the regulariser's weight times h."""
    N, L = P.shape
    s = d // 2
    L2 = h * (T ** 2).sum(axis=1)
    loss = beta * h * ((P - T) ** 2).sum(axis=1) / L2
    if G is None:
        return loss, None, L2, np.ones_like(L2)
    H1 = h * (G ** 2).sum(axis=1)
    D = (P[:, d:] - P[:, :L - d]) / (d * h)
    R = ((G[:, s:L - s] - D) ** 2).sum(axis=1)
    return loss, gamma_h * h * R / H1, L2, H1


def dpreds_np(P, T, G, L2, H1, gl, gr, *, d=2, h, beta=1.0, gamma_h=0.0):
    """The backward gather: dP[i] from the upstream gradients gl, gr [N] of loss and reg, element by element --
        dP[i] = gl beta h 2 / L2 (P - T)[i] + gr gamma_h h 2 / H1 / (d h) (r[i-s] - r[i+s])
    with r[c] = D P[c] - G[c] on s <= c < L - s and zero outside it."""
    N, L = P.shape
    s = d // 2
    dP = (gl * beta * h * 2 / L2)[:, None] * (P - T)
    if G is None or gr is None:
        return dP

    def r(c):
        if c < s or c >= L - s:
            return 0.0
        return (P[:, c + s] - P[:, c - s]) / (d * h) - G[:, c]

    c2 = gr * gamma_h * h * 2 / H1 / (d * h)
    for i in range(L):
        dP[:, i] += c2 * (r(i - s) - r(i + s))
    return dP


@functools.lru_cache(maxsize=None)
def inputs(N, L, seed=0):
    """float32 CPU tensors (P, T, G, gl, gr): a prediction near its target (relative error ~ 0.3, so that no sum
    cancels), a target derivative of the size of the difference quotient at h = 1 / L, upstream gradients in [0.5, 1.5].
    Cached: callers must not write to them."""
    g = torch.Generator().manual_seed(1000 * L + 10 * N + seed)
    T = torch.randn(N, L, generator=g)
    P = T + 0.3 * torch.randn(N, L, generator=g)
    G = torch.randn(N, L, generator=g) * L
    gl, gr = torch.rand(N, generator=g) + 0.5, torch.rand(N, generator=g) + 0.5
    return P, T, G, gl, gr


def oracle64(lf, P, T, G=None, gl=None, gr=None):
    """``lf._terms_torch`` in float64 on the CPU from the given (any device, float32) inputs: dict(loss, reg, L2, H1, dP);
    dP is the gradient of (loss gl).sum() + (reg gr).sum() (gl, gr default to ones)."""
    f64 = lambda t: None if t is None else t.detach().double().cpu()
    p = f64(P).clone().requires_grad_(True)
    loss, reg, norms = lf._terms_torch(p, f64(T), targets_prime=f64(G))
    total = (loss * (1.0 if gl is None else f64(gl))).sum()
    if reg is not None:
        total = total + (reg * (1.0 if gr is None else f64(gr))).sum()
    (dP,) = torch.autograd.grad(total, p)
    H1 = norms["H1"]
    return dict(loss=loss.detach(), reg=None if reg is None else reg.detach(), L2=norms["L2"].detach(),
                H1=H1.detach() if torch.is_tensor(H1) else H1, dP=dP)
