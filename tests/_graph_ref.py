"""Plain-torch restatement of the graph feature extractor (reference GCN, model.py:376-427; GraphConvolution and EdgeEncoder,
layers.py:153-198, 260-281) in any dtype and on any device, and of the two models that carry it, on the oracle's pieces.
Pinned against the fixtures of tests/golden/graph/ by test_graph_conv_cpu.py.

    E  = cat([E0?, silu(conv3x3(E0, w1)), silu(conv3x3(E1, w2))], 1),   E0 = edge.permute(0, 3, 1, 2)
    h0 = x;  h_{l+1}[b,i,c] = sum_j E[b,c,i,j] (h_l W_l)[b,j,c] + bias_l[c];  ReLU behind the layers 1 .. L-2 if `activation`

The formula holds for every B and n here (the reference's B = 1 and n == C accidents are not restated)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from _util import GOLDEN, rel_l2
from oracle import galerkin_oracle as O

GCN_GOLDEN = ("g_gcn_l2", "g_gcn_l4_raw", "g_gcn_noact", "g_gcn_n70")
MODEL_GOLDEN = ("g_model1d_gcn", "g_model2d_gcn")
GRAPH_GOLDEN = GCN_GOLDEN + ("g_gconv_layer",) + MODEL_GOLDEN


def edge_encoder(sd, e0, raw_laplacian=False):
    """The channel groups of the encoded edge tensor; e0 [B, F, n, n]."""
    e1 = F.silu(F.conv2d(e0, sd["lap_conv1.conv.0.weight"], padding=1))
    e2 = F.silu(F.conv2d(e1, sd["lap_conv2.conv.0.weight"], padding=1))
    return (e0, e1, e2) if raw_laplacian else (e1, e2)


def graph_conv(h, E, weight, bias):
    """h [B, n, in], E [B, C, n, n] -> [B, n, C]."""
    y = torch.einsum("bcij,bjc->bic", E, h @ weight)
    return y if bias is None else y + bias


def gcn(sd, x, edge, *, num_gcn_layers, activation=True, raw_laplacian=False):
    E = torch.cat(edge_encoder(O._sub(sd, "edge_learner."), edge.permute(0, 3, 1, 2), raw_laplacian), dim=1)
    L = num_gcn_layers
    h = x
    for l in range(L):
        p = "gcn_layer0." if l == 0 else f"gcn_layers.{l - 1}."
        h = graph_conv(h, E, sd[p + "weight"], sd.get(p + "bias"))
        if activation and 0 < l < L - 1:
            h = F.relu(h)
    return h


def _gcn_of_cfg(sd, cfg, x, edge):
    return gcn(O._sub(sd, "feat_extract."), x, edge, num_gcn_layers=cfg["num_feat_layers"],
               activation=cfg.get("graph_activation"), raw_laplacian=bool(cfg.get("raw_laplacian")))


def simple_transformer_gcn(sd, cfg, node, edge, pos):
    """SimpleTransformer.forward with the GCN in front (model.py:760-807)."""
    x = _gcn_of_cfg(sd, cfg, node, edge)
    ek = O._enc_kwargs(cfg)
    ek["residual_type"] = cfg.get("residual_type")
    ek["activation_type"] = cfg.get("attn_activation") or "relu"
    for li in range(cfg["num_encoder_layers"]):
        x = O.encoder_layer(O._sub(sd, f"encoder_layers.{li}."), x, pos, attn_drop=None, **ek)
    return O.spectral_regressor(O._sub(sd, "regressor."), x, None, modes=cfg["fourier_modes"],
                                num_spectral_layers=cfg["num_regressor_layers"],
                                spacial_dim=cfg.get("spacial_dim") or cfg["pos_dim"],
                                spacial_fc=bool(cfg.get("spacial_fc")), activation=cfg.get("regressor_activation"))


def fourier_transformer_2d_gcn(sd, cfg, node, edge, pos, grid):
    """FourierTransformer2D.forward without scalers, the GCN between the input Linear and the encoders (model.py:953-1017)."""
    B = node.shape[0]
    ns = int(round(pos.shape[1] ** 0.5))
    x = torch.cat([node, pos.reshape(B, ns, ns, -1)], dim=-1)
    x = F.linear(x, sd["downscaler.id.weight"], sd["downscaler.id.bias"]).reshape(B, -1, cfg["n_hidden"])
    x = _gcn_of_cfg(sd, cfg, x, edge)
    ek = O._enc_kwargs(cfg)
    for li in range(cfg["num_encoder_layers"]):
        x = O.encoder_layer(O._sub(sd, f"encoder_layers.{li}."), x, pos, attn_drop=None, **ek)
    x = x.reshape(B, ns, ns, cfg["n_hidden"])
    x = O.spectral_regressor(O._sub(sd, "regressor."), x, grid, modes=cfg["fourier_modes"],
                             num_spectral_layers=cfg["num_regressor_layers"], spacial_dim=cfg["spacial_dim"],
                             spacial_fc=cfg["spacial_fc"], activation=cfg.get("regressor_activation"),
                             last_activation=bool(cfg.get("last_activation")))
    if cfg.get("boundary_condition") == "dirichlet":
        x = F.pad(x[:, 1:-1, 1:-1], (0, 0, 1, 1, 1, 1))
    return x


def run_ref(g, sd, ins):
    """The restatement of fixture g on the state dict sd and the inputs ins (its dtype and device)."""
    kind, m = g.meta["kind"], g.meta
    if kind == "gcn":
        return gcn(sd, ins["x"], ins["edge"], num_gcn_layers=m["num_gcn_layers"], activation=m["activation"],
                   raw_laplacian=m["raw_laplacian"])
    if kind == "graph_convolution":
        return graph_conv(ins["x"], ins["edge"], sd["weight"], sd["bias"]).permute(0, 2, 1)
    if kind == "simple_transformer_gcn":
        return simple_transformer_gcn(sd, m["config"], ins["node"], ins["edge"], ins["pos"])
    if kind == "fourier_transformer_2d_gcn":
        return fourier_transformer_2d_gcn(sd, m["config"], ins["node"], ins["edge"], ins["pos"], ins["grid"])
    raise KeyError(kind)


def ref_grads(g, dtype):
    """(out, {input: grad}, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    ins = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    out = run_ref(g, sd, ins)
    names = list(g.dparam)
    grads = torch.autograd.grad(out, [ins[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    nin = len(g.din)
    return out.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:]))


def all_errors(out, din, dparam, ref_out, ref_din, ref_dparam):
    errs = {"out": rel_l2(out, ref_out)}
    errs.update({"d" + k: rel_l2(din[k], v) for k, v in ref_din.items()})
    errs.update({"dW:" + k: rel_l2(dparam[k], v) for k, v in ref_dparam.items()})
    return errs


def extra(name, key):
    """An array a graph fixture holds beside the Golden fields (g_gconv_layer: out_t, dx_t, dedge_t)."""
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "graph", name + ".npz"))[key])


def burgers_edge():
    z = np.load(os.path.join(GOLDEN, "graph", "g_burgers_edge.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def init_hashes():
    with open(os.path.join(GOLDEN, "graph", "g_init_hashes.json")) as f:
        return json.load(f)
