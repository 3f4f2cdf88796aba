#!/usr/bin/env python3
"""Golden fixtures for the random-feature attention baselines ('rfa' / 'favor'), recorded on the CPU from the REAL reference:
the function and class definitions of its examples/ex1_burgers_random_fourier_features.py are loaded at run time (the file
is parsed and only its `def` / `class` statements and its `from math import` are executed, next to the library modules of
make_golden.import_reference(); its data loading and training script never run).  Nothing of its text is in this file.

Per kind:
  attn_<kind>    RandomFourierAttention          B 2, n 70,  d 32, pos_dim 1
  layer_<kind>   TransformerEncoderLayer         B 2, n 130, d 64, dim_feedforward 128, dropout 0
  model_<kind>   SimpleTransformer (the example's), B 2, n 128, d 96, 2 layers, every dropout 0

Each fixture: sd/ (float32 parameters and the omega buffer recorded per layer), in/ (float32 inputs), and from a float64 run
of the reference on exactly these values: out, the cotangent cot, din/ and dparam/ (float64).  meta["noise"][tensor] is the
relative L2 distance of the reference's own float32 run from that float64 run.  A fixture is spread over <name>.npz,
<name>_p1.npz, ... so that no file exceeds 1 MiB (tests/_rfa_ref.py: RfaGolden).

Conditioning: 'rfa' denominators can change sign.  For every attention call of every case the float64 denominators must
satisfy min |den| >= 0.1 * mean |den|, else the generator fails.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rfa.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import ast
import copy
import json
import math
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden                                              # noqa: E402
from make_golden import import_reference, perturb               # noqa: E402

OUT = os.path.join(HERE, "rfa")
EXAMPLE = os.path.join(os.path.dirname(make_golden.REF), "examples", "ex1_burgers_random_fourier_features.py")
MAX_FILE = 900 * 1024


def load_example():
    """Namespace with the example's functions and classes, resolved against the reference's library modules."""
    L, M, FT = import_reference()
    ns = {}
    for mod in (L, M):
        ns.update({k: v for k, v in vars(mod).items() if not k.startswith("__")})
    ns.update(torch=torch, nn=torch.nn, copy=copy, defaultdict=defaultdict, math=math)
    with open(EXAMPLE) as f:
        tree = ast.parse(f.read(), EXAMPLE)
    keep = [node for node in tree.body
            if isinstance(node, (ast.FunctionDef, ast.ClassDef))
            or (isinstance(node, ast.ImportFrom) and node.module == "math")]
    exec(compile(ast.Module(body=keep, type_ignores=[]), EXAMPLE, "exec"), ns)
    return ns


def rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def write(name, blob, meta):
    """<name>.npz (meta first), then <name>_p<i>.npz: greedy packing under MAX_FILE."""
    for f in os.listdir(OUT):
        if f == name + ".npz" or (f.startswith(name + "_p") and f.endswith(".npz")):
            os.remove(os.path.join(OUT, f))
    parts, cur, size = [], {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}, 0
    for k, v in blob.items():
        if cur and size + v.nbytes > MAX_FILE:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    total = 0
    for i, part in enumerate(parts):
        path = os.path.join(OUT, name + (".npz" if i == 0 else f"_p{i}.npz"))
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), path
        total += os.path.getsize(path)
    return len(parts), total


def record(name, module, xname, x, pos, run, meta):
    """module: float32, omega buffers already drawn.  The redraw is switched off: the recorded omega is what ran."""
    for m in module.modules():
        if hasattr(m, "new_feature_map"):
            m.new_feature_map = lambda device: None
    attns = [m for m in module.modules() if type(m).__name__ == "RandomFourierAttention"]
    m64 = copy.deepcopy(module).double()
    for m in m64.modules():
        if hasattr(m, "new_feature_map"):
            m.new_feature_map = lambda device: None
    # conditioning of every attention call, from the float64 run's own inputs
    worst = []

    def hook(mod, args, kwargs):
        q = mod.query_projection(args[0])
        k = mod.key_projection(args[1])
        den = torch.einsum("nld,nd->nl", mod.feature_map.forward(q), mod.feature_map.forward(k).sum(dim=1)) + mod.eps
        worst.append(float((den.abs().min() / den.abs().mean()).detach()))
    handles = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in m64.modules()
               if type(m).__name__ == "RandomFourierAttention"]
    x64 = x.double().requires_grad_(True)
    out64 = run(m64, x64, pos.double())
    for h in handles:
        h.remove()
    assert len(worst) == len(attns) and min(worst) >= 0.1, (name, worst)
    cot = torch.randn(out64.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64)
    names = [k for k, p in m64.named_parameters()]
    g64 = torch.autograd.grad(out64, [x64] + [p for _, p in m64.named_parameters()], cot)
    x32 = x.clone().requires_grad_(True)
    out32 = run(module, x32, pos)
    g32 = torch.autograd.grad(out32, [x32] + [p for _, p in module.named_parameters()], cot.float())
    noise = {"out": rel(out32.detach(), out64.detach()), "d" + xname: rel(g32[0], g64[0])}
    noise.update({k: rel(a, b) for k, a, b in zip(names, g32[1:], g64[1:])})
    blob = {"in/" + xname: x.numpy(), "in/pos": pos.numpy(), "out": out64.detach().numpy(), "cot": cot.numpy(),
            "din/" + xname: g64[0].numpy()}
    blob.update({"sd/" + k: v.detach().numpy() for k, v in module.state_dict().items()})
    blob.update({"dparam/" + k: g.numpy() for k, g in zip(names, g64[1:])})
    nfiles, total = write(name, blob, dict(meta, noise=noise, min_den_over_mean=min(worst)))
    print(f"{name:14s} out{tuple(out64.shape)} |out|={float(out64.norm()):.4f}  min|den|/mean|den|={min(worst):.3f}  "
          f"noise(out)={noise['out']:.2e} max noise={max(noise.values()):.2e}  {nfiles} file(s), {total / 1024:.0f} KiB")


def main():
    os.makedirs(OUT, exist_ok=True)
    ns = load_example()
    g = torch.Generator().manual_seed(20261020)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def draw(module):
        torch.manual_seed(4711)
        for m in module.modules():
            if hasattr(m, "new_feature_map"):
                m.new_feature_map(torch.device("cpu"))

    for kind in ("rfa", "favor"):
        B, n, d = 2, 70, 32
        torch.manual_seed(1127802)
        attn = ns["RandomFourierAttention"](d, 1, pos_dim=1, attention_type=kind, xavier_init=1e-2, diagonal_weight=1e-2)
        perturb(attn, g)
        draw(attn)
        x, pos = rn(B, n, d), torch.rand(B, n, 1, generator=g)
        record(f"attn_{kind}", attn, "x", x, pos, lambda m, x, pos: m(x, x, x, pos=pos),
               dict(what="attn", attention_type=kind, B=B, n=n, d_model=d, pos_dim=1, eps=attn.eps))

        B, n, d = 2, 130, 64
        torch.manual_seed(1127802)
        layer = ns["TransformerEncoderLayer"](d_model=d, n_head=1, dim_feedforward=128, attention_type=kind, dropout=0.0,
                                              ffn_dropout=0.0)
        perturb(layer, g)
        draw(layer)
        x, pos = rn(B, n, d), torch.rand(B, n, 1, generator=g)
        record(f"layer_{kind}", layer, "x", x, pos, lambda m, x, pos: m(x, pos),
               dict(what="layer", attention_type=kind, B=B, n=n, d_model=d, n_head=1, dim_feedforward=128, dropout=0.0,
                    ffn_dropout=0.0))

        B, n = 2, 128
        cfg = dict(node_feats=2, pos_dim=1, n_targets=1, n_hidden=96, num_feat_layers=0, num_encoder_layers=2, n_head=1,
                   dim_feedforward=96, attention_type=kind, xavier_init=0.01, diagonal_weight=0.0, layer_norm=True,
                   attn_norm=False, return_attn_weight=False, return_latent=False, decoder_type="ifft", freq_dim=16,
                   num_regressor_layers=2, fourier_modes=8, spacial_dim=1, spacial_fc=False, dropout=0.0,
                   encoder_dropout=0.0, decoder_dropout=0.0, debug=False)
        torch.manual_seed(13)
        net = ns["SimpleTransformer"](**defaultdict(lambda: None, cfg))
        perturb(net, g)
        draw(net)
        node, pos = rn(B, n, 1), torch.linspace(0, 1, n)[None, :, None].repeat(B, 1, 1)
        record(f"model_{kind}", net, "node", node, pos, lambda m, node, pos: m(node, None, pos)["preds"],
               dict(what="model", attention_type=kind, B=B, n=n, config=cfg))


if __name__ == "__main__":
    main()
