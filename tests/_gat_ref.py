"""Plain-torch restatement of the graph-attention feature extractor (reference GraphAttention, layers.py:201-257; GAT,
model.py:430-469) in any dtype and on any device, written from the rank-1 form of the scores, and of the 1-D model that
carries it.  Pinned against the fixtures of tests/golden/gat/ by test_graph_attention_cpu.py.

    h = node W;  s = h a[:F];  t = h a[F:]
    keep_ij = |adj_ij| > thresh if graph_lap else adj_ij > 0
    e_ij = LeakyReLU_alpha(s_i + t_j) where keep_ij, else -9e15;  P = softmax_j(e);  Pm = P * mask;  U = Pm h
    out = ELU(U) if concat else U

It forms [B, n, n] tensors, never the reference's [B, n, n, 2F] one."""
import json
import os

import torch
import torch.nn.functional as F

from _util import GOLDEN, rel_l2
from oracle import galerkin_oracle as O

LAYER_GOLDEN = ("a_layer", "a_layer_noconcat")
GAT_GOLDEN = ("a_gat_l2", "a_gat_l4_act", "a_gat_n70")
MODEL_GOLDEN = ("a_model1d_gat",)
ALL_GOLDEN = LAYER_GOLDEN + GAT_GOLDEN + MODEL_GOLDEN


def keep_of(adj, graph_lap=True, thresh=1e-6):
    """The keep predicate, decided in adj's own dtype as the reference does (a float32 adj against float32(thresh))."""
    return adj.abs() > thresh if graph_lap else adj > 0


def attention_core(h, s, t, keep, *, alpha=1e-2, concat=True, relu=False, mask=None):
    """(out, U, L, Pm) from h [B, n, F], s, t [B, n] and the boolean keep [B, n, n]; mask: the dropout multipliers (0 or
    1/(1-p)) or None.  L is the logsumexp of the kept scores of a row, log n for a row that keeps nothing."""
    e = F.leaky_relu(s[:, :, None] + t[:, None, :], alpha)
    e = torch.where(keep, e, torch.full_like(e, -9e15))
    P = torch.softmax(e, dim=-1)
    Pm = P if mask is None else P * mask
    U = Pm @ h
    out = F.elu(U) if concat else U
    if relu:
        out = F.relu(out)
    n = h.shape[1]
    ez = torch.where(keep, e, torch.full_like(e, float("-inf")))
    L = torch.where(keep.any(-1), torch.logsumexp(ez, dim=-1).nan_to_num(neginf=0.0),
                    torch.full_like(s, float(torch.log(torch.tensor(float(n), dtype=torch.float64)))))
    return out, U, L, Pm


def graph_attention(node, adj_keep, W, a, *, alpha=1e-2, concat=True, relu=False, mask=None):
    Fd = W.shape[1]
    h = node @ W
    s, t = (h @ a[:Fd]).squeeze(-1), (h @ a[Fd:]).squeeze(-1)
    return attention_core(h, s, t, adj_keep, alpha=alpha, concat=concat, relu=relu, mask=mask)[0]


def gat(sd, x, keep, *, num_gcn_layers, activation=False, masks=None, alpha=1e-2):
    L = num_gcn_layers
    h = x
    for l in range(L):
        p = "gat_layer0." if l == 0 else f"gat_layers.{l - 1}."
        h = graph_attention(h, keep, sd[p + "W"], sd[p + "a"], alpha=alpha, relu=bool(activation) and 0 < l < L - 1,
                            mask=None if masks is None else masks[l])
    return h


def simple_transformer_gat(sd, cfg, node, keep, pos):
    """SimpleTransformer.forward with the GAT in front (model.py:760-807)."""
    x = gat(O._sub(sd, "feat_extract."), node, keep, num_gcn_layers=cfg["num_feat_layers"],
            activation=cfg.get("graph_activation"))
    ek = O._enc_kwargs(cfg)
    ek["residual_type"] = cfg.get("residual_type")
    ek["activation_type"] = cfg.get("attn_activation") or "relu"
    for li in range(cfg["num_encoder_layers"]):
        x = O.encoder_layer(O._sub(sd, f"encoder_layers.{li}."), x, pos, attn_drop=None, **ek)
    return O.spectral_regressor(O._sub(sd, "regressor."), x, None, modes=cfg["fourier_modes"],
                                num_spectral_layers=cfg["num_regressor_layers"],
                                spacial_dim=cfg.get("spacial_dim") or cfg["pos_dim"],
                                spacial_fc=bool(cfg.get("spacial_fc")), activation=cfg.get("regressor_activation"))


def fixture_keep(g):
    """The keep predicate of fixture g, decided on its float32 adjacency."""
    m = g.meta
    if m["kind"] == "graph_attention":
        return keep_of(g.inputs["adj"], m["graph_lap"], m["thresh"])
    return keep_of(g.inputs["edge"][..., 0])


def run_ref(g, sd, ins, keep):
    kind, m = g.meta["kind"], g.meta
    if kind == "graph_attention":
        return graph_attention(ins["node"], keep, sd["W"], sd["a"], alpha=m["alpha"], concat=m["concat"])
    if kind == "gat":
        return gat(sd, ins["x"], keep, num_gcn_layers=m["num_gcn_layers"], activation=m["activation"])
    if kind == "simple_transformer_gat":
        return simple_transformer_gat(sd, m["config"], ins["node"], keep, ins["pos"])
    raise KeyError(kind)


def ref_grads(g, dtype):
    """(out, {input: grad}, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    ins = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    out = run_ref(g, sd, ins, fixture_keep(g))
    names = list(g.dparam)
    grads = torch.autograd.grad(out, [ins[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    nin = len(g.din)
    return out.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:]))


def all_errors(out, din, dparam, ref_out, ref_din, ref_dparam):
    errs = {"out": rel_l2(out, ref_out)}
    errs.update({"d" + k: rel_l2(din[k], v) for k, v in ref_din.items()})
    errs.update({"dW:" + k: rel_l2(dparam[k], v) for k, v in ref_dparam.items()})
    return errs


def init_hashes():
    with open(os.path.join(GOLDEN, "gat", "a_init_hashes.json")) as f:
        return json.load(f)


def unpack_bits(words, n):
    """int64 words [B, n, ceil(n/64)] -> bool [B, n, n]: bit (j mod 64) of word (b, i, j // 64)."""
    j = torch.arange(n, device=words.device)
    w = words[:, :, j // 64]
    return ((w >> (j % 64)) & 1).bool()
