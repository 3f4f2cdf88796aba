#!/usr/bin/env python3
"""Golden fixtures for batch_norm=True of FeedForward / SimpleTransformerEncoderLayer (nn.BatchNorm1d(dim_feedforward) on
the transposed hidden tensor, reference layers.py:979-987), recorded from the REAL reference on the CPU with the machinery
of tests/golden/make_golden.py (imported, not copied).  Every dropout p is forced to 0.  They live in this subdirectory
because the Galerkin-only checks parametrise over every *.npz directly inside tests/golden/.

Every case <name> is three files:
  <name>_in     weights, inputs and the buffers BEFORE the call (`sd/`, `in/`): bn.weight / bn.bias perturbed, running_mean,
                running_var and num_batches_tracked set to non-trivial values; meta lists the state_dict keys
  <name>_eval   module.eval(): output and gradients from those buffers (asserted here: the call leaves them unchanged)
  <name>        module.train(): output, gradients, and under `buf1/` the three buffers of every norm AFTER the call

  ff_bn_relu              bare FeedForward(128, 256, batch_norm=True), x [2, 150, 128]
  ff_bn_silu              activation='silu', d 96 / f 192 (the Burgers sizes), x [2, 33, 96]
  enc_galerkin_bn_c2      the encoder layer at the c2 shape of tests/golden/instance with batch_norm=True
  model_burgers_bn_small  SimpleTransformer, two layers, batch_norm: true

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/batchnorm/make_golden_batchnorm.py
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

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("batchnorm/<name>") reads it
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261018)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def prepare(module):
        """p = 0 everywhere, every parameter perturbed, the norms' affine pair and buffers well away from (1, 0, 0, 1, 0)."""
        for m in module.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        perturb(module, g)
        norms = [m for m in module.modules() if isinstance(m, torch.nn.BatchNorm1d)]
        assert norms
        with torch.no_grad():
            for m in norms:
                m.weight.add_(0.2 * rn(*m.weight.shape))
                m.bias.add_(0.2 * rn(*m.bias.shape))
                m.running_mean.copy_(0.1 * rn(*m.running_mean.shape))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                m.num_batches_tracked.fill_(3)

    def case(name, module, inputs, run, meta, const=None):
        const = const or {}
        prepare(module)
        before = {k: v.clone() for k, v in module.state_dict().items()}
        meta = dict(meta, state_dict_keys=list(before))
        base = SUB + name + "_in"
        blob = {"sd/" + k: v.numpy() for k, v in before.items()}
        blob.update({"in/" + k: v.numpy() for k, v in list(inputs.items()) + list(const.items())})
        blob["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(os.path.dirname(HERE), base + ".npz"), **blob)
        module.eval()
        record(SUB + name + "_eval", module, inputs, run, dict(meta, training=False), ctl, const_inputs=const, base=base)
        assert all(torch.equal(v, before[k]) for k, v in module.state_dict().items())
        module.train()
        record(SUB + name, module, inputs, run, dict(meta, training=True), ctl, const_inputs=const, base=base)
        after = module.state_dict()
        path = os.path.join(os.path.dirname(HERE), SUB + name + ".npz")
        blob = dict(np.load(path))
        for k, v in after.items():
            if k.rsplit(".", 1)[-1] in BUFFERS:
                assert not torch.equal(v, before[k]), k
                blob["buf1/" + k] = v.numpy()
            else:
                assert torch.equal(v, before[k]), k
        np.savez_compressed(path, **blob)
        print(f"{name:34s} {os.path.getsize(path) / 1024:.0f} KiB with buf1/")

    torch.manual_seed(1127802)
    case("ff_bn_relu", L.FeedForward(128, 256, batch_norm=True, activation="relu", dropout=0.0), dict(x=rn(2, 150, 128)),
         lambda m, x: m(x), dict(kind="feed_forward", in_dim=128, dim_feedforward=256, activation="relu", B=2, n=150))
    torch.manual_seed(1127802)
    case("ff_bn_silu", L.FeedForward(96, 192, batch_norm=True, activation="silu", dropout=0.0), dict(x=rn(2, 33, 96)),
         lambda m, x: m(x), dict(kind="feed_forward", in_dim=96, dim_feedforward=192, activation="silu", B=2, n=33))

    c2 = dict(d_model=128, pos_dim=2, n_head=4, dim_feedforward=256, layer_norm=False, attn_norm=True, norm_eps=1e-7,
              xavier_init=1e-2, diagonal_weight=1e-2, attention_type="galerkin", batch_norm=True)
    torch.manual_seed(1127802)
    layer = M.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, **c2)
    case("enc_galerkin_bn_c2", layer, dict(x=rn(2, 150, 128)), lambda m, x, pos: m(x, pos),
         dict(kind="encoder_layer", B=2, n=150, **c2), const=dict(pos=torch.rand(2, 150, 2, generator=g)))

    import yaml
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "config.yml")) as f:
        cfgs = yaml.full_load(f)
    cfg = dict(cfgs["ex1_burgers"])
    cfg.update(attention_type="galerkin", batch_norm=True, n_hidden=32, n_head=2, dim_feedforward=64,
               num_encoder_layers=2, freq_dim=16, fourier_modes=8)
    torch.manual_seed(13)
    model = M.SimpleTransformer(**cfg)
    node, pos = rn(2, 256, 1), torch.linspace(0, 1, 256)[None, :, None].repeat(2, 1, 1)
    case("model_burgers_bn_small", model, dict(node=node), lambda m, node, pos: m(node, None, pos)["preds"],
         dict(kind="simple_transformer", config=cfg), const=dict(pos=pos))


if __name__ == "__main__":
    main()
