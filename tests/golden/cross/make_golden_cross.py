#!/usr/bin/env python3
"""Golden fixtures for cross-attention through SimpleAttention.forward(query, key, value, pos) with the three not one tensor
(reference layers.py:829-899, 672-734), recorded from the REAL reference on the CPU with the machinery of
tests/golden/make_golden.py (imported, not copied).  The module under record is SimpleAttention itself: B 2, d_model 64, 4
heads (x_galerkin_nonorm: d_model 128), nn.Dropout off; the attention dropout is the identity or a replayed mask of 0 / 2.
meta["form"] names the tensors passed as (query, key, value): the same name twice is the same tensor.

  x_galerkin_nopos (+ _replay)  galerkin, norm; forward(q, mem, mem), pos None; n_q 50, n_kv 70; mask [B, h, 16, 16]
  x_galerkin_nopos_wide         the same form, n_q 130, n_kv 33
  x_linear_nopos                linear, norm; the same form, n_q 50, n_kv 70
  x_galerkin_inst_nopos         galerkin, norm_type='instance'; the same form, n_q 50, n_kv 70
  x_galerkin_pos                galerkin, norm; forward(q, k, v, pos), n 70, pos_dim 2
  x_linear_pos                  linear, norm; forward(q, q, v, pos) (query is key), n 70, pos_dim 2
  x_fourier_pos (+ _replay)     fourier, norm; forward(q, k, v, pos), n 70, pos_dim 2; mask [B, h, 70, 70]
  x_softmax_pos                 softmax, norm; forward(q, mem, mem, pos), n 70, pos_dim 2
  x_galerkin_nonorm             galerkin, norm=False; forward(q, mem, mem), pos None; n_q 50, n_kv 70; d_model 128 (d_k 32)

Every file holds the output, the returned weight (`attn`), a cotangent, and the gradients of every distinct input and of
every parameter.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/cross/make_golden_cross.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import AttnDropCtl, import_reference, perturb, record      # noqa: E402

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("cross/<name>") reads it
B, H = 2, 4


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261019)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def case(name, form, n_q, n_kv, attention_type, pos_dim=0, d_model=64, mask_shape=None, **kw):
        torch.manual_seed(1127802)
        attn = L.SimpleAttention(H, d_model, pos_dim=pos_dim, attention_type=attention_type, dropout=0.0, xavier_init=1e-2,
                                 diagonal_weight=1e-2, **kw)
        perturb(attn, g)
        rows = dict(zip(form, (n_q, n_kv, n_kv)))              # (a name given twice keeps its first role's rows: equal anyway)
        ins = {k: rn(B, r, d_model) for k, r in rows.items()}
        const = dict(pos=torch.rand(B, n_q, pos_dim, generator=g)) if pos_dim else {}
        meta = dict(kind="cross_attention", form=list(form), B=B, n_q=n_q, n_kv=n_kv, n_head=H, d_model=d_model,
                    pos_dim=pos_dim, attention_type=attention_type, norm=kw.get("norm", False),
                    norm_type=kw.get("norm_type", "layer"), eps=1e-5)

        def run(m, pos=None, **t):
            return m(*(t[k] for k in form), pos=pos)[0]

        def rec(nm, masks=None, base=None):
            record(SUB + nm, attn, ins, run, meta, ctl, masks=masks, const_inputs=const, base=base)
            with ctl.active(masks), torch.no_grad():
                w = attn(*(ins[k] for k in form), pos=const.get("pos"))[1]
            path = os.path.join(os.path.dirname(HERE), SUB + nm + ".npz")
            blob = dict(np.load(path))
            blob["attn"] = w.numpy()
            np.savez_compressed(path, **blob)
            assert os.path.getsize(path) < (1 << 20), (nm, os.path.getsize(path))

        rec(name)
        if mask_shape is not None:
            mask = (torch.rand(*mask_shape, generator=g) >= 0.5).float() * 2.0
            rec(name + "_replay", masks=[mask], base=SUB + name)

    mem = ("q", "mem", "mem")
    case("x_galerkin_nopos", mem, 50, 70, "galerkin", norm=True, mask_shape=(B, H, 16, 16))
    case("x_galerkin_nopos_wide", mem, 130, 33, "galerkin", norm=True)
    case("x_linear_nopos", mem, 50, 70, "linear", norm=True)
    case("x_galerkin_inst_nopos", mem, 50, 70, "galerkin", norm=True, norm_type="instance")
    case("x_galerkin_pos", ("q", "k", "v"), 70, 70, "galerkin", pos_dim=2, norm=True)
    case("x_linear_pos", ("q", "q", "v"), 70, 70, "linear", pos_dim=2, norm=True)
    case("x_fourier_pos", ("q", "k", "v"), 70, 70, "fourier", pos_dim=2, norm=True, mask_shape=(B, H, 70, 70))
    case("x_softmax_pos", mem, 70, 70, "softmax", pos_dim=2, norm=True)
    case("x_galerkin_nonorm", mem, 50, 70, "galerkin", d_model=128, norm=False)


if __name__ == "__main__":
    main()
