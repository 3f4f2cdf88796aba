#!/usr/bin/env python3
"""One training step (forward + backward) of a single encoder layer at the ex2_darcy141 encoder shape (1 849 tokens,
d 128, 4 heads x (32 + 2)) for one attention type and norm type -- the workload behind profiles/linattn_*.txt and
profiles/tokennorm_*.txt.

    python tools/linattn_micro.py --attention-type linear --batch 128 --steps 20
    python tools/linattn_micro.py --attention-type galerkin --norm-type instance --kernels
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/linattn_micro.py --attention-type galerkin

Prints one JSON line: step time from device events over the timed steps (profiler off) and the bytes each softmax /
token-norm pass has to move (computed from the shape).  --kernels adds the time of every C-ABI launch of one more step
(events around each launch: _hip.Profile), with bytes / time for the token-norm pair."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "galerkin-transformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attention-type", default="linear")
    ap.add_argument("--norm-type", default="layer", choices=("layer", "instance"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import galerkin_transformer as gt
    if not torch.cuda.is_available():
        raise SystemExit("linattn_micro.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    B, n, d, h, p, f = a.batch, 43 * 43, 128, 4, 2, 256
    torch.manual_seed(0)
    layer = gt.SimpleTransformerEncoderLayer(d_model=d, pos_dim=p, n_head=h, dim_feedforward=f, layer_norm=False,
                                             attention_type=a.attention_type, attn_norm=True, norm_eps=1e-7,
                                             norm_type=a.norm_type, dropout=0.0, ffn_dropout=0.0).to(dev).train()
    x = torch.randn(B, n, d, device=dev, requires_grad=True)
    pos, cot = torch.rand(B, n, p, device=dev), torch.randn(B, n, d, device=dev)

    def step():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        layer(x, pos).backward(cot)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    tile = 4.0 * B * n * h * ((d // h + p + 3) // 4 * 4)         # bytes of one head-tile tensor [B*n, h, DP]
    res = dict(attention_type=a.attention_type, norm_type=a.norm_type, batch=B, tokens=n, steps=a.steps,
               step_ms=e0.elapsed_time(e1) / a.steps,
               softmax_bytes=dict(feature_fwd=2 * tile, feature_bwd=3 * tile, token_fwd=3 * tile, token_bwd=5 * tile),
               # per tile (the layer normalises two, K and V): forward reads X twice and writes Y, backward reads X and dY
               # twice and writes dX
               token_norm_bytes=dict(fwd=3 * tile, bwd=5 * tile))
    if a.kernels:
        from galerkin_transformer import _hip
        with _hip.Profile() as prof:
            for _ in range(3):
                step()
            torch.cuda.synchronize()
        tab = prof.table()
        res["launch_us"] = {k: round(1e3 * v["ms"] / v["calls"], 2) for k, v in sorted(tab.items())}
        res["launch_gbps"] = {k: round(v["bytes"] / v["ms"] / 1e6, 1) for k, v in sorted(tab.items())
                              if k.startswith("gt_token_norm") and v["ms"] > 0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
