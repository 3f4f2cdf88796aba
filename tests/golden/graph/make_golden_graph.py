#!/usr/bin/env python3
"""Golden fixtures for the graph feature extractor (reference GCN, model.py:376-427; GraphConvolution and EdgeEncoder,
layers.py:153-198, 260-281; the edge features of BurgersDataset, ft.py:289-318), recorded from the REAL reference on the CPU
with the machinery of tests/golden/make_golden.py (imported, not copied).  Every nn.Dropout.p is set to 0 after construction
and the parameters are perturbed.

  g_gcn_l2         GCN, node_feats 1, C 32, L 2, F 6, B 2, n 33 (no activation: two layers have none)
  g_gcn_l4_raw     GCN, node_feats 2, C 16, L 4, F 3, raw_laplacian, B 2, n 35 (ReLU behind two layers)
  g_gcn_noact      GCN, L 3, activation=False, C 8, F 4, n 34
  g_gcn_n70        GCN, C 12, L 3, F 2, n 70
  g_gconv_layer    one GraphConvolution(5 -> 8), B 2, n 34: x as [B, n, in] (out, dx) and as [B, in, n] (out_t, dx_t)
  g_model1d_gcn    SimpleTransformer, galerkin, n_hidden 32, 2 heads, 'ifft' decoder, n 33, F 4
  g_model2d_gcn    FourierTransformer2D without scalers, n_s 7, n_hidden 32, F 3, 'ifft2', modes 3
  g_burgers_edge   edge / mass of BurgersDataset.get_edge at n_grid 17: default; renormalization; smoother='jacobi';
                   n_krylov 3 with mass features
  g_init_hashes.json   sha256 of every parameter of GCN(1, 32, 2, 6) built under torch.manual_seed(1127802)

Every module file holds the output, a cotangent, d(x) (d(node)), d(edge) and every parameter gradient.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/graph/make_golden_graph.py
"""
import hashlib
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import AttnDropCtl, import_reference, perturb, record      # noqa: E402

SUB = os.path.basename(HERE) + "/"
SEED = 1127802


def no_dropout(mod):
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def small(name):
    path = os.path.join(HERE, name)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))


def main():
    L, M, FT = import_reference()
    ctl = AttnDropCtl()
    g = torch.Generator().manual_seed(20261020)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def edge_like(B, n, F):
        """Edge features of the size the dataset hands out: O(1) near the diagonal, decaying away from it."""
        i = torch.arange(n, dtype=torch.float32)
        decay = torch.exp(-(i[:, None] - i[None, :]).abs() / 4.0)
        return (rn(B, n, n, F) * decay[None, :, :, None] / 3.0).contiguous()

    def gcn_case(name, B, n, node_feats, C, nl, F, **kw):
        torch.manual_seed(SEED)
        gcn = no_dropout(M.GCN(node_feats=node_feats, out_features=C, num_gcn_layers=nl, edge_feats=F, **kw))
        perturb(gcn, g)
        meta = dict(kind="gcn", B=B, n=n, node_feats=node_feats, out_features=C, num_gcn_layers=nl, edge_feats=F,
                    activation=kw.get("activation", True), raw_laplacian=bool(kw.get("raw_laplacian", False)))
        record(SUB + name, gcn, dict(x=rn(B, n, node_feats), edge=edge_like(B, n, F)), lambda m, x, edge: m(x, edge),
               meta, ctl)
        small(name + ".npz")

    gcn_case("g_gcn_l2", 2, 33, 1, 32, 2, 6)
    gcn_case("g_gcn_l4_raw", 2, 35, 2, 16, 4, 3, raw_laplacian=True)
    gcn_case("g_gcn_noact", 2, 34, 1, 8, 3, 4, activation=False)
    gcn_case("g_gcn_n70", 2, 70, 1, 12, 3, 2)

    # one layer, both input layouts
    B, n, cin, cout = 2, 34, 5, 8
    torch.manual_seed(SEED)
    layer = L.GraphConvolution(cin, cout)
    perturb(layer, g)
    x, e = rn(B, n, cin), (rn(B, cout, n, n) / 6.0).contiguous()
    meta = dict(kind="graph_convolution", B=B, n=n, in_features=cin, out_features=cout)
    record(SUB + "g_gconv_layer", layer, dict(x=x, edge=e), lambda m, x, edge: m(x, edge), meta, ctl)
    xt = x.transpose(1, 2).contiguous().requires_grad_(True)
    ee = e.clone().requires_grad_(True)
    out_t = layer(xt, ee)
    blob = dict(np.load(os.path.join(HERE, "g_gconv_layer.npz")))
    gs = torch.autograd.grad(out_t, [xt, ee], torch.from_numpy(blob["cot"]))
    blob.update(out_t=out_t.detach().numpy(), dx_t=gs[0].numpy(), dedge_t=gs[1].numpy())
    np.savez_compressed(os.path.join(HERE, "g_gconv_layer.npz"), **blob)
    small("g_gconv_layer.npz")

    # whole models
    import yaml
    with open("/root/reference/config.yml") as f:
        cfgs = yaml.full_load(f)
    cfg = dict(cfgs["ex1_burgers"])
    cfg.update(attention_type="galerkin", n_hidden=32, n_head=2, dim_feedforward=64, num_encoder_layers=2, freq_dim=16,
               fourier_modes=8, feat_extract_type="gcn", num_feat_layers=2, edge_feats=4, graph_activation=True,
               raw_laplacian=False)
    torch.manual_seed(13)
    model = no_dropout(M.SimpleTransformer(**cfg))
    perturb(model, torch.Generator().manual_seed(20261021), 0.02)      # (a generator of its own: see the envelope test)
    B, n = 2, 33
    node, pos = rn(B, n, 1), torch.linspace(0, 1, n)[None, :, None].repeat(B, 1, 1)
    record(SUB + "g_model1d_gcn", model, dict(node=node, edge=edge_like(B, n, 4)),
           lambda m, node, edge, pos: m(node, edge, pos)["preds"], dict(kind="simple_transformer_gcn", config=cfg), ctl,
           const_inputs=dict(pos=pos))
    small("g_model1d_gcn.npz")

    cfg = dict(cfgs["ex2_darcy"])
    cfg.update(n_hidden=32, n_head=2, dim_feedforward=64, num_encoder_layers=2, freq_dim=16, fourier_modes=3,
               downscaler_size=None, upscaler_size=None, feat_extract_type="gcn", num_feat_layers=2, edge_feats=3,
               graph_activation=True, raw_laplacian=False, dropout=0.0, downscaler_dropout=0.0, upscaler_dropout=0.0,
               ffn_dropout=0.0, encoder_dropout=0.0, decoder_dropout=0.0)
    torch.manual_seed(14)
    model = no_dropout(M.FourierTransformer2D(**cfg))
    perturb(model, torch.Generator().manual_seed(20261024), 0.02)
    B, ns = 2, 7
    node, pos, grid = rn(B, ns, ns, 1), torch.rand(B, ns * ns, 2, generator=g), torch.rand(B, ns, ns, 2, generator=g)
    record(SUB + "g_model2d_gcn", model, dict(node=node, edge=edge_like(B, ns * ns, 3)),
           lambda m, node, edge, pos, grid: m(node, edge, pos, grid)["preds"],
           dict(kind="fourier_transformer_2d_gcn", config=cfg, n_s=ns), ctl, const_inputs=dict(pos=pos, grid=grid))
    small("g_model2d_gcn.npz")

    # the dataset's edge machinery on a uniform grid of 17 points: get_edge reads these attributes of self and nothing else
    grid = np.linspace(0, 1, 17)
    blob = {}
    variants = dict(default=dict(), renorm=dict(renormalization=True), jacobi=dict(smoother="jacobi"),
                    krylov3_mass=dict(n_krylov=3, return_mass_features=True))
    for tag, kw in variants.items():
        ds = types.SimpleNamespace(n_grid=17, renormalization=False, smoother=None, n_krylov=2,
                                   return_distance_features=True, return_mass_features=False)
        ds.__dict__.update(kw)
        edges, mass = FT.BurgersDataset.get_edge(ds, grid)
        blob[tag + "/edge"] = np.asarray(edges, dtype=np.float32)
        blob[tag + "/mass"] = np.asarray(mass, dtype=np.float32)
        print(f"g_burgers_edge {tag:14s} edge{blob[tag + '/edge'].shape} mass{blob[tag + '/mass'].shape}")
    blob["meta"] = np.frombuffer(json.dumps(dict(n_grid=17, variants=variants)).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g_burgers_edge.npz"), **blob)
    small("g_burgers_edge.npz")

    # init inventory
    torch.manual_seed(SEED)
    gcn = M.GCN(1, 32, 2, 6)
    inv = {k: dict(shape=list(v.shape), sha256=hashlib.sha256(v.detach().numpy().tobytes()).hexdigest())
           for k, v in gcn.state_dict().items()}
    with open(os.path.join(HERE, "g_init_hashes.json"), "w") as f:
        json.dump(dict(seed=SEED, args=[1, 32, 2, 6], params=inv), f, indent=0)
    print("g_init_hashes:", list(inv))


if __name__ == "__main__":
    main()
