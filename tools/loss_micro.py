#!/usr/bin/env python3
"""ft.WeightedL2Loss2d.terms + reduce + backward (regulariser on, K given: the call of train_batch_darcy and of
bench.py --loss weighted_l2) on the HIP operator (gt_h1loss2d_fwd / _final / _bwd) against the torch route (_terms_torch),
at the bench's shape (N, n) = (128, 141) and at the ex4 rollout's (16, 64).

    python tools/loss_micro.py --reps 20

Prints one JSON line per (shape, route): time of a whole call (forward, reduce, backward down to the gradient of the model's
[N, n, n, 1] output) between device events, profiler off; the bytes such a call has to move at the least -- forward P, T, G,
K once (20 B per pixel), backward the same and dP (24 B per pixel) -- and their ratio in TB/s; for the HIP route also the
time of its three launches alone (_hip.Profile)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "galerkin-transformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x141,16x64", help="comma list of NxN_GRID")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from galerkin_transformer import _hip
    from galerkin_transformer.ft import WeightedL2Loss2d
    if not torch.cuda.is_available():
        raise SystemExit("loss_micro.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for shape in a.shapes.split(","):
        N, n = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        T = torch.randn(N, n, n, device=dev)
        out = (T + 0.3 * torch.randn(N, n, n, device=dev))[..., None].contiguous().requires_grad_(True)
        G, K = torch.randn(N, n, n, 2, device=dev) * n, torch.rand(N, n, n, 1, device=dev) + 0.5
        lf = WeightedL2Loss2d(regularizer=True, h=1.0 / n, gamma=0.5)
        nbytes = 44.0 * N * n * n

        def call(terms):
            loss, reg, _ = terms(out[..., 0], T, targets_prime=G, K=K)
            return torch.autograd.grad(lf.reduce(loss) + lf.reduce(reg), out)[0]

        for route, terms in (("hip", lf.terms), ("torch", lf._terms_torch)):
            for _ in range(a.warmup):
                call(terms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                call(terms)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            rec = dict(route=route, N=N, n=n, ms=round(ms, 4), MB=round(nbytes / 1e6, 2), TB_per_s=round(nbytes / ms / 1e9, 3))
            if route == "hip":
                with _hip.Profile() as prof:
                    for _ in range(a.reps):
                        call(terms)
                torch.cuda.synchronize()
                rec["launch_us"] = {k: round(1e3 * r["ms"] / r["calls"], 2) for k, r in prof.table().items()}
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
