#!/usr/bin/env python3
"""Causal linear attention, forward + backward: ops.causal_linear_attention (gt_causal_attn_*: chunked scan, linear in n)
against a plain-torch float32 composition of the tril closed form on the same device and tensors,
    A = tril(q (k / n)^T),  out = A v / (rowsum(A) + eps sum_d q),
which materialises the [B, h, n, n] matrix and its gradient.

    python tools/causal_micro.py [--shapes 4x4x8192x36,8x1x2048x100] [--rounds 5] [--seconds 1.0] [--out FILE]

Per shape B x h x n x D: `rounds` measurements of each route, alternating (HIP, torch, HIP, ...), each over as many calls as
fill seconds / rounds after a warm-up, between device events.  One JSON line per shape: the median time per call of both
routes, their run-to-run spread ((max - min) / median over the rounds), the allocator's peak above the resident tensors during
one call of each route, and the largest difference of the two routes' outputs over the largest output.  No threshold rests on
these figures."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "galerkin-transformer_amd"))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps          # ms per call


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def tril_torch(q, k, v, eps=1e-7):
    A = torch.tril(q @ (k / q.size(-2)).transpose(-1, -2))
    return (A @ v) / (A.sum(-1) + eps * q.sum(-1))[..., None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x4x8192x36,8x1x2048x100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from galerkin_transformer import ops
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes.split(","):
        B, h, n, D = (int(s) for s in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        q, k = (((torch.rand(B, h, n, D, generator=g) + 0.5).to(dev)).requires_grad_(True) for _ in range(2))
        v = torch.randn(B, h, n, D, generator=g).to(dev).requires_grad_(True)
        cot = torch.randn(B, h, n, D, generator=g).to(dev)
        routes = {"hip": lambda: torch.autograd.grad(ops.causal_linear_attention(q, k, v)[0], (q, k, v), cot),
                  "torch": lambda: torch.autograd.grad(tril_torch(q, k, v), (q, k, v), cot)}
        with torch.no_grad():
            o_hip, o_torch = ops.causal_linear_attention(q, k, v)[0], tril_torch(q, k, v)
            diff = float((o_hip - o_torch).abs().max() / o_torch.abs().max())
        reps, ms = {}, {name: [] for name in routes}
        for name, fn in routes.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[name] = max(3, int(a.seconds / a.rounds / (timed(fn, 3) * 1e-3)))
        for _ in range(a.rounds):
            for name, fn in routes.items():
                ms[name].append(timed(fn, reps[name]))
        rec = dict(tool="causal_micro", B=B, h=h, n=n, D=D, leg="fwd+bwd", out_maxdiff_over_max=diff)
        for name, fn in routes.items():
            med = statistics.median(ms[name])
            rec[name + "_ms"] = round(med, 4)
            rec[name + "_spread"] = round((max(ms[name]) - min(ms[name])) / med, 3)
            rec[name + "_peak_mib"] = round(peak_above_resident(fn) / 2 ** 20, 1)
        rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
