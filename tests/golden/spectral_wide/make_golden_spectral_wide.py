#!/usr/bin/env python3
"""Golden fixtures for spectral layers wider than the resident mode-mixing kernels take (Cin * Cout > 6144, or a weight
slice of one mode beyond 160 KiB of LDS), recorded from the REAL reference on the CPU with the machinery of
tests/golden/make_golden.py (imported, not copied), in the manner of tests/golden/softmax_wide/make_golden_softmax_wide.py.

  sconv2d_w96x80     SpectralConv2d(96, 80, modes=2), SiLU, x [2, 6, 6, 96]: the two corner blocks are two mode-mix calls of
                     Q = 4 at q_off 0 and 4; backward tiled, forward resident
  sconv1d_w128x64    SpectralConv1d(128, 64, modes=3), x [2, 16, 128]: the first decoder layer of n_hidden 128 / freq_dim 64
  sconv1d_w160x136   SpectralConv1d(160, 136, modes=2), x [2, 8, 160]: forward tiled as well
  sreg_w96           SpectralRegressor(in_dim 96, n_hidden 96, freq_dim 96, out_dim 1, modes 2, 2 spectral layers,
                     spacial_fc) on a 6 x 6 grid: the SiLU-gate hand-over between two wide layers

Weights and inputs of every case are in <name>_in (the `base` of the record: _util.Golden reads meta["base"]), for the 1 MiB
limit of a committed file.  The regressor's second spectral layer still does not fit: its weights are in sreg_w96_in2 and
their gradients in sreg_w96_d2 (tests/_spectral_wide_ref.py: wide_golden puts them together again).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/spectral_wide/make_golden_spectral_wide.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import json

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import AttnDropCtl, import_reference, perturb, record      # noqa: E402

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("spectral_wide/<name>") reads it
LIMIT = 1 << 20


def _save_base(base, module, inputs, meta):
    """Weights + inputs in a file of their own (the `base` of the record)."""
    blob = {"sd/" + k: v.detach().numpy() for k, v in module.state_dict().items()}
    blob.update({"in/" + k: v.numpy() for k, v in inputs.items()})
    blob["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(os.path.dirname(HERE), base + ".npz"), **blob)


def _split_off(name, part, prefix):
    """Move the arrays whose key starts with ``prefix`` from <name>.npz to <part>.npz."""
    root = os.path.dirname(HERE)
    blob = dict(np.load(os.path.join(root, name + ".npz")))
    moved = {k: blob.pop(k) for k in list(blob) if k.startswith(prefix)}
    assert moved and blob
    np.savez_compressed(os.path.join(root, name + ".npz"), **blob)
    np.savez_compressed(os.path.join(root, part + ".npz"), **moved)


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261020)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def case(name, module, inputs, run, meta, const=None):
        base = SUB + name + "_in"
        _save_base(base, module, dict(inputs, **(const or {})), meta)
        record(SUB + name, module, inputs, run, meta, ctl, const_inputs=const, base=base)

    torch.manual_seed(7)
    conv = L.SpectralConv2d(96, 80, 2, dropout=0.0, activation="silu")
    perturb(conv, g, 0.05)
    case("sconv2d_w96x80", conv, dict(x=rn(2, 6, 6, 96)), lambda m, x: m(x),
         dict(kind="spectral_conv2d", B=2, n=6, in_dim=96, out_dim=80, modes=2, activation="silu", flat=False))

    for cin, cout, modes, n in ((128, 64, 3, 16), (160, 136, 2, 8)):
        torch.manual_seed(7)
        conv = L.SpectralConv1d(cin, cout, modes, dropout=0.0)
        perturb(conv, g, 0.05)
        case(f"sconv1d_w{cin}x{cout}", conv, dict(x=rn(2, n, cin)), lambda m, x: m(x),
             dict(kind="spectral_conv1d", B=2, n=n, in_dim=cin, out_dim=cout, modes=modes))

    kw = dict(in_dim=96, n_hidden=96, freq_dim=96, out_dim=1, modes=2, num_spectral_layers=2, spacial_dim=2,
              spacial_fc=True, activation="silu")
    torch.manual_seed(3)
    reg = M.SpectralRegressor(dropout=0.0, **kw)
    perturb(reg, g, 0.05)
    x, grid = rn(2, 6, 6, 96), torch.rand(2, 6, 6, 2, generator=g)
    case("sreg_w96", reg, dict(x=x), lambda m, x, grid: m(x, grid=grid),
         dict(kind="spectral_regressor", last_activation=True, **kw), const=dict(grid=grid))
    _split_off(SUB + "sreg_w96_in", SUB + "sreg_w96_in2", "sd/spectral_conv.1.")
    _split_off(SUB + "sreg_w96", SUB + "sreg_w96_d2", "dparam/spectral_conv.1.")

    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            print(f"{f:44s} {size / 1024:7.0f} KiB")
            assert size < LIMIT, f


if __name__ == "__main__":
    main()
