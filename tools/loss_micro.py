#!/usr/bin/env python3
"""The training objectives' terms + reduce + backward on the HIP operators against the torch route (_terms_torch).

--dim 2 (default): ft.WeightedL2Loss2d (regulariser on, K given: the call of train_batch_darcy and of bench.py --loss
weighted_l2) on gt_h1loss2d_fwd / _final / _bwd, at the bench's shape (N, n) = (128, 141) and at the ex4 rollout's (16, 64).
--dim 1: ft.WeightedL2Loss (regulariser on: the call of train_batch_burgers) on gt_h1loss1d_fwd / _final / _bwd, at the
bench's ex1 batch (N, L) = (32, 8192) and at the reference's (4, 2048).

    python tools/loss_micro.py --reps 20
    python tools/loss_micro.py --dim 1 --reps 200 --warmup 20 --out profiles/loss_micro.jsonl

Prints one JSON line per (shape, route): time of a whole call (forward, reduce, backward down to the gradient of the model's
[N, n, n, 1] / [N, L, 1] output) between device events, profiler off; the bytes such a call has to move at the least -- 2-D:
forward P, T, G, K once (20 B per pixel), backward the same and dP (24 B per pixel); 1-D: forward P, T, G (12 B per
element), backward the same and dP (16 B) -- and their ratio in TB/s; for the HIP route also the time of its three launches
alone (_hip.Profile).  The 1-D call moves at most a few MB: its time is launches, not bandwidth."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "galerkin-transformer_amd"))


def case(dim, N, n, dev):
    """(loss function, call(terms) -> gradient of the model output, bytes a call has to move) at one shape."""
    import torch
    from galerkin_transformer.ft import WeightedL2Loss, WeightedL2Loss2d
    torch.manual_seed(0)
    if dim == 2:
        T = torch.randn(N, n, n, device=dev)
        out = (T + 0.3 * torch.randn(N, n, n, device=dev))[..., None].contiguous().requires_grad_(True)
        kw = dict(targets_prime=torch.randn(N, n, n, 2, device=dev) * n, K=torch.rand(N, n, n, 1, device=dev) + 0.5)
        lf = WeightedL2Loss2d(regularizer=True, h=1.0 / n, gamma=0.5)
        nbytes = 44.0 * N * n * n
    else:
        T = torch.randn(N, n, device=dev)
        out = (T + 0.3 * torch.randn(N, n, device=dev))[..., None].contiguous().requires_grad_(True)
        kw = dict(targets_prime=torch.randn(N, n, device=dev) * n)
        lf = WeightedL2Loss(regularizer=True, h=1.0 / n, gamma=0.5)
        nbytes = 28.0 * N * n

    def call(terms):
        loss, reg, _ = terms(out[..., 0], T, **kw)
        return torch.autograd.grad(lf.reduce(loss) + lf.reduce(reg), out)[0]

    return lf, call, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, choices=(1, 2), default=2)
    ap.add_argument("--shapes", default=None, help="comma list of NxN_GRID (--dim 2: default 128x141,16x64) or NxL (--dim 1: "
                                                   "default 32x8192,4x2048)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the lines to this file too (profiles/loss_micro.jsonl)")
    a = ap.parse_args()
    import torch
    from galerkin_transformer import _hip
    if not torch.cuda.is_available():
        raise SystemExit("loss_micro.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for shape in (a.shapes or ("128x141,16x64" if a.dim == 2 else "32x8192,4x2048")).split(","):
        N, n = (int(v) for v in shape.split("x"))
        lf, call, nbytes = case(a.dim, N, n, dev)
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
            rec = dict(route=route, N=N, **({"n": n} if a.dim == 2 else {"dim": 1, "L": n}), ms=round(ms, 4),
                       MB=round(nbytes / 1e6, 2), TB_per_s=round(nbytes / ms / 1e9, 3))
            if route == "hip":
                with _hip.Profile() as prof:
                    for _ in range(a.reps):
                        call(terms)
                torch.cuda.synchronize()
                rec["launch_us"] = {k: round(1e3 * r["ms"] / r["calls"], 2) for k, r in prof.table().items()}
            print(json.dumps(rec), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
