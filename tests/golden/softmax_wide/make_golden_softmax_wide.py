#!/usr/bin/env python3
"""Golden fixtures for attention_type 'softmax' at the 64- and 96-wide heads (head tiles DP = round4(d_k + pos_dim) = 68 and
100), recorded from the REAL reference on the CPU with the machinery of tests/golden/make_golden.py (imported, not copied),
in the manner of tests/golden/softmax/make_golden_softmax.py: every nn.Dropout is off; the attention dropout, which the
reference applies to the softmax OUTPUT (layers.py:700-701), is the identity or a replayed [B, h, n, n] mask of 0 / 2.

  enc_softmax_w100 (+ _replay)    B 2, n 65, d 96, 1 head x (96 + 1): DP = 100, the encoder layer of config.yml: ex1_burgers
  enc_softmax_w68 (+ _replay)     B 2, n 65, d 128, 2 heads x (64 + 2): DP = 68; weights / inputs in _in
  enc_softmax_w68_weights         the same layer and inputs with attn_weight=True: `attn` holds the returned softmax(S) .* mask
  model_burgers_softmax_ex1       SimpleTransformer(**config.yml: ex1_burgers) with attention_type='softmax', B 2, n 128: the
                                  full widths on a short grid.  num_encoder_layers is 2, not the shipped 4, for the 1 MiB
                                  limit of a committed file; even so the weights take 1.4 MiB (0.9 of it the spectral
                                  regressor's), so they and their gradients are split: the encoder's weights and the
                                  inputs in _in, `sd/regressor.*` in _in2, `dparam/regressor.*` in _d2
                                  (tests/_softmax_wide_ref.py: wide_golden puts them together again).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/softmax_wide/make_golden_softmax_wide.py
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

SUB = os.path.basename(HERE) + "/"           # record() writes tests/golden/<name>.npz; Golden("softmax_wide/<name>") reads it
LIMIT = 1 << 20


def _no_dropout(mod):
    # the reference forces dropout = 0.1 for 'softmax' (model.py:65-66) whatever the argument says
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def _save_base(base, module, inputs, meta):
    """Weights + inputs in a file of their own (the `base` of the records that share them): keeps every file under 1 MiB."""
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
    g = torch.Generator().manual_seed(20261019)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def enc_case(name, B, n, replay=False, split=False, weights_twin=False, **kw):
        torch.manual_seed(1127802)
        layer = _no_dropout(M.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, **kw))
        perturb(layer, g)
        p = kw["pos_dim"]
        x, pos = rn(B, n, kw["d_model"]), torch.rand(B, n, p, generator=g)
        meta = dict(kind="encoder_layer", B=B, n=n, **kw)
        const = dict(pos=pos)
        base = None
        if split:
            base = SUB + name + "_in"
            _save_base(base, layer, dict(x=x, pos=pos), meta)
        record(SUB + name, layer, dict(x=x), lambda m, x, pos: m(x, pos), meta, ctl, const_inputs=const, base=base)
        if replay:
            mask = (torch.rand(B, kw["n_head"], n, n, generator=g) >= 0.5).float() * 2.0
            record(SUB + name + "_replay", layer, dict(x=x), lambda m, x, pos: m(x, pos), meta, ctl, masks=[mask],
                   const_inputs=const, base=base or SUB + name)
        if weights_twin:
            kww = dict(kw, attn_weight=True)
            twin = _no_dropout(M.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, **kww))
            twin.load_state_dict(layer.state_dict(), strict=True)
            record(SUB + name + "_weights", twin, dict(x=x), lambda m, x, pos: m(x, pos)[0],
                   dict(kind="encoder_layer", B=B, n=n, **kww), ctl, const_inputs=const, base=base)
            with ctl.active(None), torch.no_grad():
                w = twin(x, pos)[1]
            path = os.path.join(os.path.dirname(HERE), SUB + name + "_weights.npz")
            blob = dict(np.load(path))
            blob["attn"] = w.numpy()
            np.savez_compressed(path, **blob)

    enc_case("enc_softmax_w100", 2, 65, replay=True, d_model=96, pos_dim=1, n_head=1, dim_feedforward=192,
             attention_type="softmax", layer_norm=False, attn_norm=True, xavier_init=1e-3, diagonal_weight=1e-2)
    enc_case("enc_softmax_w68", 2, 65, replay=True, split=True, weights_twin=True, d_model=128, pos_dim=2, n_head=2,
             dim_feedforward=256, attention_type="softmax", layer_norm=False, attn_norm=True)

    import yaml
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "config.yml")) as f:
        cfgs = yaml.full_load(f)
    cfg = dict(cfgs["ex1_burgers"])
    cfg.update(attention_type="softmax", num_encoder_layers=2)      # 2 of the shipped 4 layers: the file size limit (above)
    torch.manual_seed(13)
    model = _no_dropout(M.SimpleTransformer(**cfg))
    perturb(model, g, 0.02)
    node, pos = rn(2, 128, 1), torch.linspace(0, 1, 128)[None, :, None].repeat(2, 1, 1)
    name = "model_burgers_softmax_ex1"
    meta = dict(kind="simple_transformer", config=cfg)
    _save_base(SUB + name + "_in", model, dict(node=node, pos=pos), meta)
    record(SUB + name, model, dict(node=node), lambda m, node, pos: m(node, None, pos)["preds"], meta, ctl,
           const_inputs=dict(pos=pos), base=SUB + name + "_in")
    _split_off(SUB + name + "_in", SUB + name + "_in2", "sd/regressor.")
    _split_off(SUB + name, SUB + name + "_d2", "dparam/regressor.")

    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            print(f"{f:44s} {size / 1024:7.0f} KiB")
            assert size < LIMIT, f


if __name__ == "__main__":
    main()
