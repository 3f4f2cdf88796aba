#!/usr/bin/env python3
"""Random-feature attention ('rfa' / 'favor') on the gt_rfattn_* kernels (ops.random_feature_attention) against a plain-torch
float32 composition of the same formula on the same device and tensors: forward + backward time and peak memory.

    python tools/rfattn_micro.py [--shapes 8x2048x96,4x8192x96] [--rounds 5] [--seconds 1.0] [--out FILE]

Per shape B x n x d and kind: `rounds` measurements of each route, alternating (HIP, torch, HIP, ...), each over as many
calls as fill seconds / rounds after a warm-up, between device events.  One JSON line per shape and kind: the median time per
forward + backward of both routes, their run-to-run spread ((max - min) / median over the rounds), the allocator's peak above
the resident tensors during one call of each route, and the ratios torch / HIP."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def compare(routes, rounds, seconds):
    reps = {}
    for name, fn in routes.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(3, int(seconds / rounds / (timed(fn, 3) * 1e-3)))
    out = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            out[name].append(timed(fn, reps[name]))
    return out, reps


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def composition(x, pos, wqkv, bqkv, omega, wout, bout, kind, eps):
    d = x.shape[-1]
    qkv = F.linear(x, wqkv, bqkv)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]

    def fmap(z):
        zs = z * d ** -0.25
        u = zs @ omega
        if kind == "rfa":
            return math.sqrt(2.0 / d) * torch.cat([torch.cos(u), torch.sin(u)], dim=-1)
        c = 0.5 * (zs * zs).sum(-1, keepdim=True) + 0.5 * math.log(d)
        return torch.cat([torch.exp(u - c), torch.exp(-u - c)], dim=-1)
    pq, pk = fmap(q), fmap(k)
    den = pq @ pk.sum(1).unsqueeze(-1) + eps
    return F.linear(torch.cat([(pq @ (pk.transpose(1, 2) @ v)) / den, pos], dim=-1), wout, bout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x2048x96,4x8192x96")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from galerkin_transformer import ops
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes.split(","):
        B, n, d = (int(v) for v in shape.split("x"))
        for kind in ("rfa", "favor"):
            g = torch.Generator().manual_seed(1)
            x = (0.5 * torch.randn(B, n, d, generator=g)).to(dev).requires_grad_(True)
            pos = torch.rand(B, n, 1, generator=g).to(dev)
            wqkv = (0.05 * torch.randn(3 * d, d, generator=g)).to(dev).requires_grad_(True)
            bqkv = torch.zeros(3 * d, device=dev, requires_grad=True)
            omega = torch.randn(d, d // 2, generator=g).to(dev)
            wout = (0.1 * torch.randn(d, d + 1, generator=g)).to(dev).requires_grad_(True)
            bout = torch.zeros(d, device=dev, requires_grad=True)
            cot = torch.randn(B, n, d, generator=g).to(dev)
            leaves = (x, wqkv, bqkv, wout, bout)

            def step(fwd):
                def run():
                    torch.autograd.grad(fwd(), leaves, cot)
                return run
            routes = {"hip": step(lambda: ops.random_feature_attention(x, pos, wqkv, bqkv, omega, wout, bout, kind=kind,
                                                                       eps=1e-6)),
                      "torch": step(lambda: composition(x, pos, wqkv, bqkv, omega, wout, bout, kind, 1e-6))}
            ms, reps = compare(routes, a.rounds, a.seconds)
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = dict(shape=[B, n, d], kind=kind, leg="fwd+bwd", reps=reps,
                       hip_ms=med["hip"], torch_ms=med["torch"],
                       hip_spread=(max(ms["hip"]) - min(ms["hip"])) / med["hip"],
                       torch_spread=(max(ms["torch"]) - min(ms["torch"])) / med["torch"],
                       hip_peak_mib=peak_above_resident(routes["hip"]) / 2 ** 20,
                       torch_peak_mib=peak_above_resident(routes["torch"]) / 2 ** 20)
            rec["time_ratio_torch_over_hip"] = rec["torch_ms"] / rec["hip_ms"]
            rec["peak_ratio_torch_over_hip"] = rec["torch_peak_mib"] / rec["hip_peak_mib"]
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
