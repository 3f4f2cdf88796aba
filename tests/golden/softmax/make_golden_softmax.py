#!/usr/bin/env python3
"""Golden fixtures for attention_type 'softmax' (scaled dot-product attention, reference layers.py:672-705), recorded from
the REAL reference on the CPU with the machinery of tests/golden/make_golden.py (imported, not copied).  Every nn.Dropout is
off; the attention dropout, which the reference applies to the softmax OUTPUT (layers.py:700-701), is the identity or a
replayed [B, h, n, n] mask of 0 / 2.

  enc_softmax_c2 (+ _replay)      B 2, n 150, d 128, 4 heads x (32 + 2), attn_norm, norm_eps 1e-7; weights / inputs in _in
  enc_softmax_c1                  n 300, d 64, 4 heads x (16 + 1), residual_type='minus'
  enc_softmax_c4_ln (+ _replay)   d 96, 2 heads x (48 + 2): DP = 52, layer_norm=True, attn_norm=False; weights / inputs in _in
  enc_softmax_weights             n 70, attn_weight=True: `attn` holds the returned softmax(S) .* mask
  model_burgers_softmax_small     SimpleTransformer, two layers, as model_burgers_linear_small

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/softmax/make_golden_softmax.py
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

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("softmax/<name>") reads it


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261018)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def enc_case(name, B, n, replay=False, split=False, **kw):
        torch.manual_seed(1127802)
        layer = M.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, **kw)
        # the reference forces dropout = 0.1 for 'softmax' (model.py:65-66) whatever the argument says
        for m in layer.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        perturb(layer, g)
        p = kw.get("pos_dim", 1)
        x, pos = rn(B, n, kw["d_model"]), torch.rand(B, n, p, generator=g)
        meta = dict(kind="encoder_layer", B=B, n=n, **kw)
        want_w = bool(kw.get("attn_weight"))
        run = (lambda m, x, pos: m(x, pos)[0]) if want_w else (lambda m, x, pos: m(x, pos))
        const = dict(pos=pos)
        base = None
        if split:
            # weights + inputs in a file of their own (the `base` of both records): keeps every file under 1 MiB
            base = SUB + name + "_in"
            blob = {"sd/" + k: v.detach().numpy() for k, v in layer.state_dict().items()}
            blob.update({"in/x": x.numpy(), "in/pos": pos.numpy(),
                         "meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)})
            np.savez_compressed(os.path.join(os.path.dirname(HERE), base + ".npz"), **blob)
        record(SUB + name, layer, dict(x=x), run, meta, ctl, const_inputs=const, base=base)
        if want_w:
            with ctl.active(None), torch.no_grad():
                w = layer(x, pos)[1]
            path = os.path.join(os.path.dirname(HERE), SUB + name + ".npz")
            blob = dict(np.load(path))
            blob["attn"] = w.numpy()
            np.savez_compressed(path, **blob)
        if replay:
            mask = (torch.rand(B, kw["n_head"], n, n, generator=g) >= 0.5).float() * 2.0
            record(SUB + name + "_replay", layer, dict(x=x), run, meta, ctl, masks=[mask], const_inputs=const,
                   base=base or SUB + name)

    enc_case("enc_softmax_c2", 2, 150, replay=True, split=True, d_model=128, pos_dim=2, n_head=4, dim_feedforward=256,
             attention_type="softmax", layer_norm=False, attn_norm=True, norm_eps=1e-7, xavier_init=1e-2,
             diagonal_weight=1e-2)
    enc_case("enc_softmax_c1", 2, 300, d_model=64, pos_dim=1, n_head=4, dim_feedforward=128, attention_type="softmax",
             layer_norm=False, attn_norm=True, residual_type="minus")
    enc_case("enc_softmax_c4_ln", 1, 144, replay=True, split=True, d_model=96, pos_dim=2, n_head=2, dim_feedforward=192,
             attention_type="softmax", layer_norm=True, attn_norm=False)
    enc_case("enc_softmax_weights", 2, 70, d_model=64, pos_dim=2, n_head=4, dim_feedforward=128, attention_type="softmax",
             layer_norm=False, attn_norm=True, attn_weight=True)

    import yaml
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "config.yml")) as f:
        cfgs = yaml.full_load(f)
    cfg = dict(cfgs["ex1_burgers"])
    cfg.update(attention_type="softmax", n_hidden=32, n_head=2, dim_feedforward=64, num_encoder_layers=2, freq_dim=16,
               fourier_modes=8)
    torch.manual_seed(13)
    model = M.SimpleTransformer(**cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    perturb(model, g, 0.02)
    node, pos = rn(2, 256, 1), torch.linspace(0, 1, 256)[None, :, None].repeat(2, 1, 1)
    record(SUB + "model_burgers_softmax_small", model, dict(node=node), lambda m, node, pos: m(node, None, pos)["preds"],
           dict(kind="simple_transformer", config=cfg), ctl, const_inputs=dict(pos=pos))


if __name__ == "__main__":
    main()
