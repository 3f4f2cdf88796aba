#!/usr/bin/env python3
"""The three graph-convolution kernels (gt_graphconv_fwd / _bwd_data / _bwd_edge) against the reference's formulation of the
same products, torch.matmul(E, s.unsqueeze(-1)) and its autograd backward, on the same tensors in the same process.

    python tools/graphconv_micro.py [--shapes 4x96x512,4x96x2048] [--rounds 5] [--seconds 1.0] [--out FILE]

Per shape B x C x n and product: `rounds` measurements of each route, alternating (HIP, torch, HIP, ...), each over as many
calls as fill seconds / rounds after a warm-up, between device events.  One JSON line per shape and product: the median time
per call of both routes, their run-to-run spread ((max - min) / median over the rounds), the bytes the product has to move
(4 B C n^2 for the edge tensor plus the vectors), TB/s and the share of the ~6.3 TB/s an MI355X sustains from HBM, and
`hip_not_slower`: the HIP median is below the torch median plus the larger of the two spreads."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "galerkin-transformer_amd"))

HBM_TBS = 6.3


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


def summarise(ms):
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x96x512,4x96x2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from galerkin_transformer import _hip
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for shape in a.shapes.split(","):
        B, Cc, n = (int(v) for v in shape.split("x"))
        E = torch.randn(B, Cc, n, n, device=dev)
        S, G = torch.randn(B, n, Cc, device=dev), torch.randn(B, n, Cc, device=dev)
        S2 = torch.randn(B, n, Cc, device=dev)
        s_t = S.permute(0, 2, 1).contiguous()                      # [B, C, n]: the reference's `support`
        g_t = G.permute(0, 2, 1).contiguous().unsqueeze(-1)        # the gradient of its [B, C, n, 1] product
        Y, dS, dE = torch.empty_like(S), torch.empty_like(S), torch.empty_like(E)

        s_req = s_t.clone().requires_grad_(True)
        y_s = torch.matmul(E, s_req.unsqueeze(-1))
        E_req = E.clone().requires_grad_(True)
        y_e = torch.matmul(E_req, s_t.unsqueeze(-1))
        edge_bytes, vec_bytes = 4.0 * B * Cc * n * n, 4.0 * B * Cc * n
        products = {
            "fwd": (edge_bytes + 2 * vec_bytes, {
                "hip": lambda: _hip.graphconv_fwd([E], S, None, B, n, Cc, Y=Y),
                "torch": lambda: torch.matmul(E, s_t.unsqueeze(-1))}),
            "bwd_data": (edge_bytes + 2 * vec_bytes, {
                "hip": lambda: _hip.graphconv_bwd_data([E], G, B, n, Cc, dS=dS),
                "torch": lambda: torch.autograd.grad(y_s, s_req, g_t, retain_graph=True)}),
            "bwd_edge": (edge_bytes + 2 * vec_bytes, {
                "hip": lambda: _hip.graphconv_bwd_edge([dE], [G], [S], B, n, Cc),
                "torch": lambda: torch.autograd.grad(y_e, E_req, g_t, retain_graph=True)}),
            "bwd_edge_p2": (edge_bytes + 4 * vec_bytes, {           # two layers' pairs in the one write (no torch twin)
                "hip": lambda: _hip.graphconv_bwd_edge([dE], [G, S2], [S, G], B, n, Cc)}),
        }
        for name, (nbytes, routes) in products.items():
            ms, reps = compare(routes, a.rounds, a.seconds)
            rec = dict(shape=[B, Cc, n], product=name, bytes=nbytes, rounds=a.rounds, reps=reps)
            for route, v in ms.items():
                med, spread = summarise(v)
                tbs = nbytes / (med * 1e-3) / 1e12
                rec[route] = dict(ms=round(med, 4), spread=round(spread, 4), tb_per_s=round(tbs, 3),
                                  hbm_share=round(tbs / HBM_TBS, 3), ms_rounds=[round(x, 4) for x in v])
            if "torch" in rec:
                slack = max(rec["hip"]["spread"], rec["torch"]["spread"]) * rec["torch"]["ms"]
                rec["hip_not_slower"] = rec["hip"]["ms"] <= rec["torch"]["ms"] + slack
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del E, dE, E_req, y_e, y_s, products
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
