#!/usr/bin/env python3
"""The workloads behind profiles/fourier16_wide_B*.txt: the two-term fp16 Fourier attention at the wide head tiles
(DP = 68, 100), device events, profiler off, warm, median of --reps runs; one JSON line per case.

    python tools/fourier16_wide_micro.py kernels   # pre-split, forward, dQ', dK' + dV' at ex1's shapes and (8, 3721, 2, 68),
                                                   # next to the 52- and 36-wide instances; the dual pass against two single passes
    python tools/fourier16_wide_micro.py attn      # SimpleAttention forward + backward, fused against materialising
    python tools/fourier16_wide_micro.py step      # one SimpleTransformer(**config.yml: ex1_burgers) training step
    python tools/fourier16_wide_micro.py step --root OTHER_CHECKOUT   # the same step on another (built) checkout, e.g. the parent commit
"""
import argparse
import json
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("kernels", "attn", "step"))
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=15)
a = ap.parse_args()
a.root = os.path.abspath(a.root)
sys.path.insert(0, a.root)
sys.path.insert(0, os.path.join(a.root, "galerkin-transformer_amd"))
import torch  # noqa: E402
import galerkin_transformer as gt  # noqa: E402
from galerkin_transformer import _hip as H  # noqa: E402

dev = torch.device("cuda:0")
H.lib()
PEAK = 2.5e15          # dense f16 MFMA peak, FLOP/s


def med(fn, reps=None, warm=3):
    reps = reps or a.reps
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def mfma_flop(B, n, h, DP, dual):
    """FLOP the MFMA pipe executes in one pass: per wave (32 owners) and stream tile 12 NS + 6 ND instructions of 16x16x32
    (x 2 in the dual pass), waves = B h ceil(n / 32) (dead waves of a partial block excluded)."""
    NS, ND, nt = DP // 32 + 1, (DP + 15) // 16, (n + 31) // 32
    return B * h * nt * nt * (12 * NS + 6 * ND) * (2 if dual else 1) * 16 * 16 * 32 * 2


def kernels():
    out = []
    for (B, n, h, DP) in [(8, 2048, 1, 100), (8, 2048, 1, 52), (4, 8192, 1, 100), (4, 8192, 1, 52), (8, 3721, 2, 68),
                          (8, 3721, 2, 52), (8, 3721, 4, 36)]:
        g = torch.Generator().manual_seed(1)
        Q, K, V, dO = (torch.randn(B * n, h, DP, generator=g).to(dev) for _ in range(4))
        scale = 1.0 / math.sqrt(DP) / n
        H.set_seed(5, dev)
        for mode, drop in (("plain", None), ("block p=0.5", H.dropout_desc(0.5, 3, dev))):
            imgs = H.fourier16_presplit((Q, K, V, dO), B, n, h, DP)
            iq, ik, iv, ido = imgs
            O1 = torch.empty(B * n, h, DP, device=dev)
            O2 = torch.empty_like(O1)
            t = {}
            t["presplit x4"] = med(lambda: H.fourier16_presplit((Q, K, V, dO), B, n, h, DP))
            t["forward"] = med(lambda: H.fourier16_attn(iq, None, ik, iv, B, n, h, DP, scale, None, drop, False, O1=O1))
            t["dQ"] = med(lambda: H.fourier16_attn(ido, None, iv, ik, B, n, h, DP, scale, None, drop, False, O1=O1))
            t["dual"] = med(lambda: H.fourier16_attn(ik, iv, iq, ido, B, n, h, DP, scale, None, drop, True, O1=O1, O2=O2))

            def two_single():      # the same two outputs by two single-output passes (owner = key)
                H.fourier16_attn(ik, None, iq, ido, B, n, h, DP, scale, None, drop, True, O1=O1)
                H.fourier16_attn(iv, None, ido, iq, B, n, h, DP, scale, None, drop, True, O1=O2)
            t["dual as 2 single"] = med(two_single)
            row = dict(B=B, n=n, h=h, DP=DP, mode=mode)
            for k, (m, lo, hi) in t.items():
                row[k + " ms"] = round(m, 4)
                row[k + " min/max"] = [round(lo, 4), round(hi, 4)]
                if k in ("forward", "dQ", "dual"):
                    row[k + " mfma share"] = round(mfma_flop(B, n, h, DP, k == "dual") / (m * 1e-3) / PEAK, 3)
            print(json.dumps(row), flush=True)
            out.append(row)
    # dual == two singles, bit for bit (what a split of the dual pass would compute)
    B, n, h, DP = 2, 300, 1, 100
    Q, K, V, dO = (torch.randn(B * n, h, DP, device=dev) for _ in range(4))
    iq, ik, iv, ido = H.fourier16_presplit((Q, K, V, dO), B, n, h, DP)
    dv, dk = H.fourier16_attn(ik, iv, iq, ido, B, n, h, DP, 1.0 / n, None, None, True)
    dv1 = H.fourier16_attn(ik, None, iq, ido, B, n, h, DP, 1.0 / n, None, None, True)
    dk1 = H.fourier16_attn(iv, None, ido, iq, B, n, h, DP, 1.0 / n, None, None, True)
    print(json.dumps({"dual equals two singles bitwise": bool(torch.equal(dv, dv1) and torch.equal(dk, dk1))}))


def attn():
    for (B, n, d, h, p) in [(8, 2048, 96, 1, 1), (4, 8192, 96, 1, 1), (8, 3721, 128, 2, 2)]:
        torch.manual_seed(1)
        m = gt.SimpleAttention(h, d, pos_dim=p, attention_type="fourier", norm=True, eps=1e-7, dropout=0.0).to(dev)
        x = torch.randn(B, n, d, device=dev, requires_grad=True)
        pos, cot = torch.rand(B, n, p, device=dev), torch.randn(B, n, d, device=dev)
        for dmode in ("reference", "off"):
            gt.set_attention_dropout(dmode)
            row = dict(B=B, n=n, d=d, h=h, p=p, attention_dropout=dmode)
            for need_w in (False, True):
                def step():
                    m.zero_grad(set_to_none=True)
                    x.grad = None
                    y, _ = m.fused_forward(x, pos, residual=x, need_weights=need_w)
                    y.backward(cot)
                torch.cuda.reset_peak_memory_stats(dev)
                t = med(step)
                k = "materialising" if need_w else "fused"
                row[k + " fwd+bwd ms"] = round(t[0], 3)
                row[k + " min/max"] = [round(t[1], 3), round(t[2], 3)]
                row[k + " peak MiB"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20)
            print(json.dumps(row), flush=True)
        gt.set_attention_dropout("reference")


def step():
    import yaml
    with open(os.path.join(a.root, "galerkin-transformer_amd", "config.yml")) as f:
        cfg = yaml.full_load(f)["ex1_burgers"]
    for (B, n) in [(8, 2048), (4, 8192)]:
        torch.manual_seed(0)
        model = gt.SimpleTransformer(**cfg).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        g = torch.Generator().manual_seed(0)
        pos = torch.linspace(0, 1, n)[None, :, None].repeat(B, 1, 1).to(dev)
        node, target = torch.randn(B, n, 1, generator=g).to(dev), torch.randn(B, n, 1, generator=g).to(dev)

        def one():
            opt.zero_grad(set_to_none=True)
            loss = ((model(node, None, pos, pos)["preds"][..., :1] - target) ** 2).mean()
            loss.backward()
            opt.step()
        torch.cuda.reset_peak_memory_stats(dev)
        t = med(one, warm=4)
        print(json.dumps(dict(root=a.root, B=B, n=n, step_ms=round(t[0], 3), min_max=[round(t[1], 3), round(t[2], 3)],
                              peak_MiB=round(torch.cuda.max_memory_allocated(dev) / 2 ** 20),
                              fourier16_dp=list(getattr(H, "FOURIER16_DP", H.FOURIER_DP)))), flush=True)


{"kernels": kernels, "attn": attn, "step": step}[a.what]()
