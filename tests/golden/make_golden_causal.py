#!/usr/bin/env python3
"""Golden fixtures for causal linear attention, recorded on the CPU from the REAL reference: its causal_linear_attn function
(imported through make_golden.import_reference(); nothing of its text is in this file) is run in float64 with F.dropout
patched to identity (the reference always drops the running state with p = 0.5).

Per case (B, h, n, D), without a mask and, where listed, with one whose first two keys are dropped (leading rows exactly 0):
  q, k, v, cot   float32 arrays whose values lie on a 1/256 grid (they compress, and float32 holds them exactly):
                 q, k in [0.5, 1.5] (positive: every denominator is a sum of positive terms), v, cot in [-2, 2]
  kv_mask        uint8, only in the masked cases
  out, dq, dk, dv float64, from the reference function on the float64 images of these inputs.  The function writes its key
                 and value arguments in place, so it gets clones.
  out32 .. dv32  float32, from the reference function run in float32 on the same inputs: its own rounding error, the
                 yardstick of the GPU bars.
A fixture is spread over <name>.npz, <name>_p1.npz, ... so that no file exceeds 200 KB (tests/_causal_ref.py: CausalGolden).

decoder_state_dict.json: names and shapes of GalerkinTransformerDecoderLayer(64, 2).state_dict() of the reference (the
constructor runs there; the forward does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_causal.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import json

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import AttnDropCtl, import_reference               # noqa: E402

OUT = os.path.join(HERE, "causal")
MAX_FILE = 190 * 1000
CASES = (("n1_d16", (2, 2, 1, 16), False), ("n65_d20", (2, 2, 65, 20), False), ("n65_d20_masked", (2, 2, 65, 20), True),
         ("n130_d36", (1, 2, 130, 36), False), ("n130_d36_masked", (1, 2, 130, 36), True))


def write(name, blob, meta):
    """<name>.npz (meta first), then <name>_p<i>.npz: greedy packing under MAX_FILE."""
    for f in os.listdir(OUT):
        if f == name + ".npz" or (f.startswith(name + "_p") and f.endswith(".npz")):
            os.remove(os.path.join(OUT, f))
    parts, cur, size = [], {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}, 0
    for k, v in blob.items():
        cost = v.nbytes // 2 if k in ("q", "k", "v", "cot", "kv_mask") else v.nbytes       # the gridded inputs compress
        if size and size + cost > MAX_FILE:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += cost
    parts.append(cur)
    total = 0
    for i, part in enumerate(parts):
        path = os.path.join(OUT, name + (".npz" if i == 0 else f"_p{i}.npz"))
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 200 * 1000, (path, os.path.getsize(path))
        total += os.path.getsize(path)
    return len(parts), total


def main():
    os.makedirs(OUT, exist_ok=True)
    L, M, _ = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261021)

    def grid(lo, hi, *shape):
        return (torch.randint(int(lo * 256), int(hi * 256) + 1, shape, generator=g).float() / 256)

    for name, (B, h, n, D), masked in CASES:
        q, k = grid(0.5, 1.5, B, h, n, D), grid(0.5, 1.5, B, h, n, D)
        v, cot = grid(-2, 2, B, h, n, D), grid(-2, 2, B, h, n, D)
        kv_mask = None
        if masked:
            kv_mask = torch.rand(B, n, generator=g) > 0.2
            kv_mask[:, :2] = False
            kv_mask[:, 2] = True
        q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
        with ctl.active(None):
            out, _ = L.causal_linear_attn(q64, k64.clone(), v64.clone(), kv_mask=kv_mask, dropout=torch.nn.Dropout(0.1))
        dq, dk, dv = torch.autograd.grad(out, (q64, k64, v64), cot.double())
        blob = dict(q=q.numpy(), k=k.numpy(), v=v.numpy(), cot=cot.numpy())
        if masked:
            blob["kv_mask"] = kv_mask.numpy().astype(np.uint8)
            assert float(out[:, :, :2].abs().max()) == 0.0
        blob.update(out=out.detach().numpy(), dq=dq.numpy(), dk=dk.numpy(), dv=dv.numpy())
        q32, k32, v32 = (t.clone().requires_grad_(True) for t in (q, k, v))
        with ctl.active(None):
            o32, _ = L.causal_linear_attn(q32, k32.clone(), v32.clone(), kv_mask=kv_mask, dropout=torch.nn.Dropout(0.1))
        g32 = torch.autograd.grad(o32, (q32, k32, v32), cot)
        blob.update(out32=o32.detach().numpy(), dq32=g32[0].numpy(), dk32=g32[1].numpy(), dv32=g32[2].numpy())
        nfiles, total = write(name, blob, dict(B=B, h=h, n=n, D=D, masked=masked, eps=1e-7))
        print(f"{name:18s} out{tuple(out.shape)} max|out|={float(out.detach().abs().max()):.4f}  {nfiles} file(s), {total / 1000:.0f} KB")

    dec = M.GalerkinTransformerDecoderLayer(64, 2)
    shapes = {k: list(v.shape) for k, v in dec.state_dict().items()}
    with open(os.path.join(OUT, "decoder_state_dict.json"), "w") as f:
        json.dump(shapes, f, indent=1)
        f.write("\n")
    print(f"decoder_state_dict.json: {len(shapes)} entries")


if __name__ == "__main__":
    main()
