#!/usr/bin/env python3
"""gt_batchnorm_fwd / gt_batchnorm_bwd (batch_norm=True of FeedForward) on a [T, f] hidden matrix, by default the bench's:
T = 128 * 141^2 rows, f = 256 -- the workload behind profiles/batchnorm_B128.txt.

    python tools/batchnorm_micro.py --reps 10
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/batchnorm_micro.py --reps 3

Prints one JSON line per call kind: time from device events around the launches (profiler off; _hip.Profile), the bytes the
call has to move (the nbytes the binding hands to _launch, computed from the shape) and their ratio in TB/s."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "galerkin-transformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128 * 141 * 141)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from galerkin_transformer import _hip
    if not torch.cuda.is_available():
        raise SystemExit("batchnorm_micro.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    T, f = a.rows, a.width
    torch.manual_seed(0)
    x = torch.randn(T, f, device=dev).relu_()
    dz, pre = torch.randn(T, f, device=dev), torch.randn(T, f, device=dev)
    gamma, beta = torch.rand(f, device=dev) + 0.5, torch.randn(f, device=dev)
    rm, rv = torch.zeros(f, device=dev), torch.ones(f, device=dev)
    z, gh = torch.empty_like(x), torch.empty_like(x)
    drop = _hip.dropout_desc(0.1, 7, dev)
    _, stats, _ = _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True, out=z)
    relu, silu = (_hip.AUX_GT0, None, 1.0 / 0.9, None), (_hip.AUX_DSILU, pre, 1.0, drop)
    cases = {
        "fwd_train": lambda: _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True, out=z),
        "fwd_eval": lambda: _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, False, out=z),
        "bwd_train_relu": lambda: _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=relu, out=gh),
        "bwd_train_silu_drop": lambda: _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=silu, out=gh),
        "bwd_eval_relu": lambda: _hip.batchnorm_bwd(x, dz, gamma, stats, False, gate=relu, out=gh),
    }
    for name, fn in cases.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        with _hip.Profile() as prof:
            for _ in range(a.reps):
                fn()
        torch.cuda.synchronize()
        (r,) = prof.table().values()
        ms, nbytes = r["ms"] / r["calls"], r["bytes"] / r["calls"]
        print(json.dumps(dict(call=name, rows=T, width=f, ms=round(ms, 4), GB=round(nbytes / 1e9, 3),
                              TB_per_s=round(nbytes / ms / 1e9, 3))), flush=True)


if __name__ == "__main__":
    main()
