#!/usr/bin/env python3
"""Golden fixtures for attention_type 'official': the classic post-LN Transformer encoder layer around nn.MultiheadAttention
(reference model.py:244-373, `_TransformerEncoderLayer` / `TransformerEncoderWrapper`) and the SimpleTransformer built on it
(model.py:888-895), recorded from the REAL reference on the CPU with the machinery of tests/golden/make_golden.py (imported,
not copied).  Every dropout is off (the layer is built with dropout=0.0), every parameter perturbed.

  enc_official_d64h4              B 2, n 150, d 64, 4 heads of 16, dim_feedforward 128, layer_norm
  enc_official_d128h4             B 2, n 150, d 128, 4 heads of 32, dim_feedforward 256, layer_norm; weights / inputs in _in
  enc_official_d96h2_pos          B 1, n 144, src 94 wide + pos 2 wide = d 96, 2 heads of 48, layer_norm=False
  enc_official_d64h1              B 2, n 130, d 64, 1 head
  enc_official_d96h1              B 2, n 130, d 96, 1 head
  enc_official_weights            B 2, n 70, d 64, 4 heads, attn_weight=True: `attn` holds the returned [B, n, n]
  wrapper_official_2              TransformerEncoderWrapper of two layers with a final nn.LayerNorm, d 64, 4 heads, n 70
  model_burgers_official_small    SimpleTransformer, ex1_burgers with attention_type='official', two layers, pos=None

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/official/make_golden_official.py
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

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("official/<name>") reads it


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261020)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def split_base(name, module, meta, **tensors):
        """Weights + inputs in a file of their own (the `base` of the record): keeps every file under 1 MiB."""
        base = SUB + name + "_in"
        blob = {"sd/" + k: v.detach().numpy() for k, v in module.state_dict().items()}
        blob.update({"in/" + k: v.numpy() for k, v in tensors.items()})
        blob["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(os.path.dirname(HERE), base + ".npz"), **blob)
        return base

    def enc_case(name, B, n, d_model, nhead, dim_feedforward, layer_norm=True, attn_weight=False, pos_dim=0, split=False):
        torch.manual_seed(1127802)
        layer = M._TransformerEncoderLayer(d_model, nhead, dim_feedforward=dim_feedforward, dropout=0.0,
                                           layer_norm=layer_norm, attn_weight=attn_weight)
        perturb(layer, g)
        x = rn(B, n, d_model - pos_dim)
        meta = dict(kind="official_layer", B=B, n=n, d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward,
                    layer_norm=layer_norm, attn_weight=attn_weight)
        const = dict(pos=torch.rand(B, n, pos_dim, generator=g)) if pos_dim else {}
        if attn_weight:
            run = lambda m, x, **c: m(x, **c)[0]
        else:
            run = lambda m, x, **c: m(x, **c)
        base = split_base(name, layer, meta, x=x, **const) if split else None
        record(SUB + name, layer, dict(x=x), run, meta, ctl, const_inputs=const, base=base)
        if attn_weight:
            with torch.no_grad():
                w = layer(x, **const)[1]
            path = os.path.join(os.path.dirname(HERE), SUB + name + ".npz")
            blob = dict(np.load(path))
            blob["attn"] = w.numpy()
            np.savez_compressed(path, **blob)

    enc_case("enc_official_d64h4", 2, 150, 64, 4, 128)
    enc_case("enc_official_d128h4", 2, 150, 128, 4, 256, split=True)
    enc_case("enc_official_d96h2_pos", 1, 144, 96, 2, 192, layer_norm=False, pos_dim=2)
    enc_case("enc_official_d64h1", 2, 130, 64, 1, 128)
    enc_case("enc_official_d96h1", 2, 130, 96, 1, 192)
    enc_case("enc_official_weights", 2, 70, 64, 4, 128, attn_weight=True)

    torch.manual_seed(1127802)
    layer = M._TransformerEncoderLayer(64, 4, dim_feedforward=128, dropout=0.0)
    wrap = M.TransformerEncoderWrapper(layer, 2, norm=torch.nn.LayerNorm(64))
    perturb(wrap, g)
    record(SUB + "wrapper_official_2", wrap, dict(x=rn(2, 70, 64)), lambda m, x: m(x),
           dict(kind="official_wrapper", B=2, n=70, d_model=64, nhead=4, dim_feedforward=128, layer_norm=True, num_layers=2),
           ctl)

    import yaml
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "config.yml")) as f:
        cfgs = yaml.full_load(f)
    cfg = dict(cfgs["ex1_burgers"])
    cfg.update(attention_type="official", n_hidden=32, n_head=2, dim_feedforward=64, num_encoder_layers=2, freq_dim=16,
               fourier_modes=8)
    torch.manual_seed(13)
    model = M.SimpleTransformer(**cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    perturb(model, g, 0.02)
    record(SUB + "model_burgers_official_small", model, dict(node=rn(2, 256, 1)),
           lambda m, node: m(node, None, None)["preds"], dict(kind="simple_transformer", config=cfg), ctl)


if __name__ == "__main__":
    main()
