#!/usr/bin/env python3
"""One graph-attention layer on the gt_graphattn_* kernels (layers.GraphAttention -> ops.graph_attention_stack) against a
plain-torch float32 composition of the rank-1 form on the same device and tensors: forward, and forward + backward.

    python tools/graphattn_micro.py [--shapes 4x512x96,4x2048x96,2x8192x96] [--rounds 5] [--seconds 1.0] [--out FILE]

The torch route materialises the [B, n, n] scores, weights and their gradients (not the reference's [B, n, n, 2F] input of the
score product, which does not fit at these sizes); the HIP route holds one bit per pair.  Dropout is off on both routes (the
torch route would have to store its mask).  Per shape B x n x F and leg: `rounds` measurements of each route, alternating
(HIP, torch, HIP, ...), each over as many calls as fill seconds / rounds after a warm-up, between device events.  One JSON
line per shape and leg: the median time per call of both routes, their run-to-run spread ((max - min) / median over the
rounds), the allocator's peak above the resident tensors during one call of each route, and `hip_not_slower`: the HIP median
is below the torch median plus the larger of the two spreads."""
import argparse
import json
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
    """routes: {name: fn}.  Returns {name: [ms per call, one per round]}, the routes alternating within a round."""
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


def torch_layer(node, keep, W, a, alpha):
    Fd = W.shape[1]
    h = node @ W
    e = F.leaky_relu((h @ a[:Fd]) + (h @ a[Fd:]).transpose(1, 2), alpha)
    P = torch.softmax(torch.where(keep, e, torch.full_like(e, -9e15)), dim=-1)
    return F.elu(P @ h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x512x96,4x2048x96,2x8192x96")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--in-features", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import galerkin_transformer as GT
    dev = torch.device("cuda:0")
    for shape in a.shapes.split(","):
        B, n, Fd = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        layer = GT.GraphAttention(a.in_features, Fd, dropout=0.0).to(dev).train()
        node = torch.randn(B, n, a.in_features, device=dev, requires_grad=True)
        cot = torch.randn(B, n, Fd, device=dev)
        # a banded Laplacian-like adjacency, nine kept entries per row, plus a sprinkle of long-range ones
        i = torch.arange(n, device=dev)
        adj = ((i[:, None] - i[None, :]).abs() <= 4).float() * 0.5
        adj = (adj[None] + (torch.rand(B, n, n, device=dev) < 4.0 / n).float()).contiguous()
        keep = adj.abs() > layer.thresh
        params = [node, layer.W, layer.a]

        def hip_fwd():
            with torch.no_grad():
                return layer(node, adj)

        def torch_fwd():
            with torch.no_grad():
                return torch_layer(node, keep, layer.W, layer.a, layer.alpha)

        def hip_fb():
            return torch.autograd.grad(layer(node, adj), params, cot)

        def torch_fb():
            return torch.autograd.grad(torch_layer(node, keep, layer.W, layer.a, layer.alpha), params, cot)

        with torch.no_grad():
            err = float((hip_fwd() - torch_fwd()).norm() / torch_fwd().norm())
        for leg, routes in (("fwd", dict(hip=hip_fwd, torch=torch_fwd)), ("fwd_bwd", dict(hip=hip_fb, torch=torch_fb))):
            ms, reps = compare(routes, a.rounds, a.seconds)
            rec = dict(shape=[B, n, Fd], leg=leg, rounds=a.rounds, reps=reps, rel_l2_hip_vs_torch=err,
                       nn_float_bytes=4 * B * n * n)
            for route, v in ms.items():
                med = statistics.median(v)
                rec[route] = dict(ms=round(med, 4), spread=round((max(v) - min(v)) / med, 4),
                                  peak_bytes=peak_above_resident(routes[route]), ms_rounds=[round(x, 4) for x in v])
            slack = max(rec["hip"]["spread"], rec["torch"]["spread"]) * rec["torch"]["ms"]
            rec["hip_not_slower"] = rec["hip"]["ms"] <= rec["torch"]["ms"] + slack
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del adj, keep, node, cot, layer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
