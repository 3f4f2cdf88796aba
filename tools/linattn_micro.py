#!/usr/bin/env python3
"""One training step (forward + backward) of a single encoder layer at the ex2_darcy141 encoder shape (1 849 tokens,
d 128, 4 heads x (32 + 2)) for one attention type -- the workload behind profiles/linattn_*.txt.

    python tools/linattn_micro.py --attention-type linear --batch 128 --steps 20
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/linattn_micro.py --attention-type galerkin

Prints one JSON line: step time from device events over the timed steps (profiler off) and the bytes each softmax pass
has to move (computed from the shape)."""
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
                                             dropout=0.0, ffn_dropout=0.0).to(dev).train()
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
    print(json.dumps(dict(attention_type=a.attention_type, batch=B, tokens=n, steps=a.steps,
                          step_ms=e0.elapsed_time(e1) / a.steps,
                          softmax_bytes=dict(feature_fwd=2 * tile, feature_bwd=3 * tile, token_fwd=3 * tile,
                                             token_bwd=5 * tile))))


if __name__ == "__main__":
    main()
