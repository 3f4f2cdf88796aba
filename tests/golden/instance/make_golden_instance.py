#!/usr/bin/env python3
"""Golden fixtures for norm_type='instance' of the Galerkin family (K, V normalised over the tokens, one mean and variance
per (sample, head, channel); reference layers.py:842-854, 917-923), recorded from the REAL reference on the CPU with the
machinery of tests/golden/make_golden.py (imported, not copied).  They live in this subdirectory because the Galerkin-only
checks parametrise over every *.npz directly inside tests/golden/.

  enc_galerkin_inst_c2 (+ _replay)   B 2, n 150, d 128, 4 heads x (32 + 2), norm_eps=1e-7; weights and inputs in ..._c2_in
  enc_galerkin_inst_c1               n 300, d 64, 4 heads x (16 + 1), residual_type='minus'
  enc_linear_inst_c2                 attention_type='linear' at the c2 shape; weights and inputs in ..._c2_in
  enc_global_inst_c5                 attention_type='global', 1 head x (48 + 2), layer_norm=True, attn_norm=True
  enc_galerkin_inst_nopos            forward(x, pos=None): no coordinate columns, no `fc`
  enc_galerkin_inst_c4               d 96, 2 heads: Dr = 50, DP = 52
  model_burgers_galerkin_inst_small  SimpleTransformer, two layers, as model_burgers_linear_small

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/instance/make_golden_instance.py
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

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("instance/<name>") reads it


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261016)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def enc_case(name, B, n, masks_shape=None, nopos=False, split=False, **kw):
        torch.manual_seed(1127802)
        layer = M.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, norm_type="instance", **kw)
        # the reference forces dropout = 0.1 for 'linear' (model.py:65-66) whatever the argument says
        for m in layer.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        perturb(layer, g)
        p = kw.get("pos_dim", 1)
        x, pos = rn(B, n, kw["d_model"]), torch.rand(B, n, p, generator=g)
        meta = dict(kind="encoder_layer", B=B, n=n, norm_type="instance", **kw)
        if nopos:
            meta["nopos"] = True
            run, const = (lambda m, x: m(x, None)), {}
        else:
            run, const = (lambda m, x, pos: m(x, pos)), dict(pos=pos)
        base = None
        if split:
            # weights + inputs in a file of their own (the `base` of the records): keeps every file under 1 MiB
            base = SUB + name + "_in"
            blob = {"sd/" + k: v.detach().numpy() for k, v in layer.state_dict().items()}
            blob.update({"in/x": x.numpy(), "in/pos": pos.numpy(),
                         "meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)})
            np.savez_compressed(os.path.join(os.path.dirname(HERE), base + ".npz"), **blob)
        record(SUB + name, layer, dict(x=x), run, meta, ctl, const_inputs=const, base=base)
        base = base or SUB + name
        if masks_shape is not None:
            mask = (torch.rand(*masks_shape, generator=g) >= 0.5).float() * 2.0
            record(SUB + name + "_replay", layer, dict(x=x), run, meta, ctl, masks=[mask], const_inputs=const,
                   base=base)

    c2 = dict(d_model=128, pos_dim=2, n_head=4, dim_feedforward=256, layer_norm=False, attn_norm=True, norm_eps=1e-7,
              xavier_init=1e-2, diagonal_weight=1e-2)
    enc_case("enc_galerkin_inst_c2", 2, 150, masks_shape=(2, 4, 34, 34), split=True, attention_type="galerkin", **c2)
    enc_case("enc_galerkin_inst_c1", 2, 300, d_model=64, pos_dim=1, n_head=4, dim_feedforward=128,
             attention_type="galerkin", layer_norm=False, attn_norm=True, residual_type="minus")
    enc_case("enc_linear_inst_c2", 2, 150, split=True, attention_type="linear", **c2)
    enc_case("enc_global_inst_c5", 2, 256, d_model=48, pos_dim=2, n_head=1, dim_feedforward=96, attention_type="global",
             layer_norm=True, attn_norm=True)
    enc_case("enc_galerkin_inst_nopos", 2, 140, nopos=True, d_model=64, pos_dim=2, n_head=4, dim_feedforward=128,
             attention_type="galerkin", layer_norm=False, attn_norm=True, norm_eps=1e-7)
    enc_case("enc_galerkin_inst_c4", 1, 144, d_model=96, pos_dim=2, n_head=2, dim_feedforward=192,
             attention_type="galerkin", layer_norm=False, attn_norm=True, norm_eps=1e-7)

    import yaml
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "config.yml")) as f:
        cfgs = yaml.full_load(f)
    cfg = dict(cfgs["ex1_burgers"])
    cfg.update(attention_type="galerkin", norm_type="instance", n_hidden=32, n_head=2, dim_feedforward=64,
               num_encoder_layers=2, freq_dim=16, fourier_modes=8)
    torch.manual_seed(13)
    model = M.SimpleTransformer(**cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    perturb(model, g, 0.02)
    node, pos = rn(2, 256, 1), torch.linspace(0, 1, 256)[None, :, None].repeat(2, 1, 1)
    record(SUB + "model_burgers_galerkin_inst_small", model, dict(node=node),
           lambda m, node, pos: m(node, None, pos)["preds"], dict(kind="simple_transformer", config=cfg), ctl,
           const_inputs=dict(pos=pos))


if __name__ == "__main__":
    main()
