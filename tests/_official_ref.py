"""Plain-torch restatement of attention_type='official': the classic post-LN Transformer encoder layer around
nn.MultiheadAttention (reference model.py:244-373), its wrapper and the SimpleTransformer built on it, in any dtype and on
any device.  The formulas are the ones the modules document:

    [q, k, v] = src in_proj_weight^T + in_proj_bias, heads of d_k = d / h;  P = softmax(q k^T / sqrt(d_k));  Pm = P .* m
    a = out_proj(merge_heads(Pm v));  src = [norm1](src + a);  src = [norm2](src + linear2(relu(linear1(src))))
    w = mean over the heads of Pm

(every nn.Dropout the identity; m: an explicit [B, h, n, n] mask standing in for the dropout on P).  Pinned against the
fixtures of tests/golden/official/ by test_official_cpu.py; builders and runners of the package's modules for those fixtures
live here too, shared by the CPU and the GPU tests."""
import math

import torch
import torch.nn.functional as F

from oracle import galerkin_oracle as O

OFFICIAL_GOLDEN = ("enc_official_d64h4", "enc_official_d128h4", "enc_official_d96h2_pos", "enc_official_d64h1",
                   "enc_official_d96h1", "enc_official_weights", "wrapper_official_2", "model_burgers_official_small")
SUB = "official/"


def attention(sd, x, n_head, m=None):
    """(out_proj(merge_heads(Pm v)), Pm [B, h, n, n]) from the keys self_attn.* of ``sd``."""
    B, n, d = x.shape
    dk = d // n_head
    qkv = F.linear(x, sd["self_attn.in_proj_weight"], sd["self_attn.in_proj_bias"])
    q, k, v = (t.reshape(B, n, n_head, dk).permute(0, 2, 1, 3) for t in qkv.split(d, dim=-1))
    p = (torch.einsum("bhnd,bhmd->bhnm", q, k) / math.sqrt(dk)).softmax(dim=-1)
    pm = p if m is None else p * m.to(p.dtype)
    o = torch.einsum("bhnm,bhmd->bhnd", pm, v).permute(0, 2, 1, 3).reshape(B, n, d)
    return F.linear(o, sd["self_attn.out_proj.weight"], sd["self_attn.out_proj.bias"]), pm


def encoder_layer(sd, src, pos=None, *, n_head, layer_norm=True, m=None, return_attn=False, eps=1e-5):
    if pos is not None:
        src = torch.cat([pos.to(src.dtype), src], dim=-1)
    d = src.shape[-1]
    a, pm = attention(sd, src, n_head, m)
    src = src + a
    if layer_norm:
        src = F.layer_norm(src, (d,), sd["norm1.weight"], sd["norm1.bias"], eps)
    f = F.linear(F.relu(F.linear(src, sd["linear1.weight"], sd["linear1.bias"])), sd["linear2.weight"], sd["linear2.bias"])
    src = src + f
    if layer_norm:
        src = F.layer_norm(src, (d,), sd["norm2.weight"], sd["norm2.bias"], eps)
    return (src, pm.mean(dim=1)) if return_attn else src


def wrapper(sd, src, *, n_head, num_layers, layer_norm=True, final_norm=True):
    for i in range(num_layers):
        src = encoder_layer(O._sub(sd, f"layers.{i}."), src, n_head=n_head, layer_norm=layer_norm)
    if final_norm:
        src = F.layer_norm(src, (src.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-5)
    return src


def simple_transformer(sd, cfg, node):
    """SimpleTransformer(attention_type='official') called as model(node, None, None): the oracle's 1-D model with this
    file's layer in the encoder's place (pos=None: nothing is concatenated, the regressor gets no grid)."""
    def layer(lsd, x, pos, attn_drop=None, **_kw):
        return encoder_layer(lsd, x, None, n_head=cfg["n_head"], layer_norm=bool(cfg["layer_norm"]))
    orig = O.encoder_layer
    O.encoder_layer = layer
    try:
        return O.simple_transformer_1d(sd, cfg, node, None)
    finally:
        O.encoder_layer = orig


def run_ref(g, sd, inputs, return_attn=False, m=None):
    """The restatement on one fixture of tests/golden/official/ (sd / inputs in any dtype)."""
    meta = g.meta
    if meta["kind"] == "official_layer":
        return encoder_layer(sd, inputs["x"], inputs.get("pos"), n_head=meta["nhead"], layer_norm=meta["layer_norm"], m=m,
                             return_attn=return_attn)
    if meta["kind"] == "official_wrapper":
        return wrapper(sd, inputs["x"], n_head=meta["nhead"], num_layers=meta["num_layers"], layer_norm=meta["layer_norm"])
    assert meta["kind"] == "simple_transformer"
    return simple_transformer(sd, meta["config"], inputs["node"])


def ref_grads(g, dtype, m=None):
    """(out, {input: grad}, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    inputs = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    out = run_ref(g, sd, inputs, m=m)
    names = list(g.dparam)
    grads = torch.autograd.grad(out, [inputs[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    nin = len(g.din)
    return out.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:]))


def build_module(gt, g, dropout=0.0):
    """The package's module for one fixture (parameters not loaded)."""
    meta = g.meta
    if meta["kind"] in ("official_layer", "official_wrapper"):
        layer = gt._TransformerEncoderLayer(meta["d_model"], meta["nhead"], dim_feedforward=meta["dim_feedforward"],
                                            dropout=dropout, layer_norm=meta["layer_norm"],
                                            attn_weight=bool(meta.get("attn_weight")))
        if meta["kind"] == "official_layer":
            return layer
        return gt.TransformerEncoderWrapper(layer, meta["num_layers"], norm=torch.nn.LayerNorm(meta["d_model"]))
    return gt.SimpleTransformer(**meta["config"])


def run_module(mod, g, ins):
    """The module's call as the fixture recorded it: (out, w or None)."""
    kind = g.meta["kind"]
    if kind == "official_layer":
        out = mod(ins["x"], ins.get("pos"))
    elif kind == "official_wrapper":
        out = mod(ins["x"])
    else:
        out = mod(ins["node"], None, None)["preds"]
    return out if isinstance(out, tuple) else (out, None)
