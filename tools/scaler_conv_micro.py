#!/usr/bin/env python3
"""The 'conv' scaler modes against the same modules driven through PyTorch-ROCm's own layers.

UpScaler(upsample_mode='conv') and DownScaler(downsample_mode='conv'), forward + backward in training mode (dropout on), on
the HIP operators (gt_deconv3x3s2_*, gt_avgpool2_act_*) and with the modules' own nn.ConvTranspose2d / nn.AvgPool2d / nn.Dropout
members called directly; the down-scaler's convolutions are Conv2dResBlock on both routes.

    python tools/scaler_conv_micro.py --reps 30 --out profiles/scaler_conv_micro.jsonl

Prints one JSON line per module: the median (and min / max) time of a call between device events with the profiler off, the
two routes alternating, five calls per sample; how far the two routes' results are apart in eval mode (relative L2 of the
output and the input gradient); the number of C-ABI launches of one HIP call and its four largest symbols (_hip.Profile, in a
call of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "galerkin-transformer_amd")]
import galerkin_transformer as gt  # noqa: E402
from galerkin_transformer import _hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--channels", type=int, default=128)
ap.add_argument("--coarse", type=int, default=12, help="n_s of the up-scaler's input (12 -> 147)")
ap.add_argument("--fine", type=int, default=141, help="n of the down-scaler's input")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.manual_seed(0)


def torch_up(mod, x):
    x = x.permute(0, 3, 1, 2)
    for b in mod.upsample:
        x = b.activation(b.dropout(b.deconv0(x)))
        x = b.activation(b.deconv1(x))
    return x.permute(0, 2, 3, 1)


def torch_down(mod, x):
    b, n = x.size(0), x.size(1)
    x = x.reshape(b, 1, n, n)
    for e in mod.downsample:
        x = e.activation(e.pool0(e.conv0(x)))
        x1 = e.conv1(x)
        x2 = e.conv2(x1)
        x3 = e.conv3(x2)
        x = e.activation(e.pool1(torch.cat([x1, x2, x3], dim=1)))
    return x.permute(0, 2, 3, 1)


def fwd_bwd(fn, mod, x, cot):
    for p in mod.parameters():
        p.grad = None
    x.grad = None
    y = fn(mod, x)
    y.backward(cot)
    return y


def time_pair(name, mod, x, routes, reps=args.reps, warm=args.warmup):
    with torch.no_grad():
        shape = routes["hip"](mod.eval(), x).shape
    cot = torch.randn(shape, device=dev)
    # the two routes agree (eval mode: no dropout)
    mod.eval()
    outs = {}
    for k, fn in routes.items():
        y = fwd_bwd(fn, mod, x, cot)
        outs[k] = (y.detach().clone(), x.grad.clone())
    torch.cuda.synchronize()
    agree = [float((outs["hip"][i] - outs["torch"][i]).norm() / outs["torch"][i].norm()) for i in (0, 1)]
    mod.train()
    times = {k: [] for k in routes}
    for k, fn in routes.items():
        for _ in range(warm):
            fwd_bwd(fn, mod, x, cot)
    torch.cuda.synchronize()
    for _ in range(reps):                       # alternate the two routes
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fwd_bwd(fn, mod, x, cot)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / 5)
    with _hip.Profile() as prof:
        fwd_bwd(routes["hip"], mod, x, cot)
    torch.cuda.synchronize()
    tab = prof.table()
    top = sorted(tab.items(), key=lambda kv: -kv[1]["ms"])[:4]
    res = dict(name=name, out_shape=list(shape), agree_out_dx=agree,
               hip_ms=statistics.median(times["hip"]), torch_ms=statistics.median(times["torch"]),
               hip_minmax=[min(times["hip"]), max(times["hip"])], torch_minmax=[min(times["torch"]), max(times["torch"])],
               hip_launches=len(prof.records), profile_ms=sum(v["ms"] for v in tab.values()),
               top=[(k, v["calls"], round(v["ms"], 4)) for k, v in top])
    print(json.dumps(res), flush=True)
    return res


results = []
B, C = args.batch, args.channels
up = gt.UpScaler(C, C).to(dev)
x = torch.randn(B, args.coarse, args.coarse, C, device=dev, requires_grad=True)
results.append(time_pair(f"UpScaler('conv') B={B} C={C} n_s={args.coarse}", up, x, {"hip": lambda m, t: m(t), "torch": torch_up}))
down = gt.DownScaler(1, C).to(dev)
x = torch.randn(B, args.fine, args.fine, 1, device=dev, requires_grad=True)
results.append(time_pair(f"DownScaler('conv') B={B} 1->{C} n={args.fine}", down, x, {"hip": lambda m, t: m(t), "torch": torch_down}))
if args.out:
    with open(args.out, "a") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")
