"""Plain-torch restatement of attention_type='softmax' (scaled dot-product attention, reference layers.py:672-705,
829-899) and of the encoder layer / SimpleTransformer around it, in any dtype and on any device.  The CPU oracle
(oracle/galerkin_oracle.py) covers the softmax-free types only; this file restates the softmax branch for the tests, pinned
against the fixtures of tests/golden/softmax/ by test_softmax_attention_cpu.py, and reuses the oracle's unchanged pieces."""
import contextlib
import math

import torch
import torch.nn.functional as F

from _linear_ref import enc_kwargs, grad_errors, zero_grad_params      # noqa: F401  (the same zero-gradient biases: see below)
from oracle import galerkin_oracle as O

SOFTMAX_GOLDEN = ("enc_softmax_c2", "enc_softmax_c2_replay", "enc_softmax_c1", "enc_softmax_c4_ln",
                  "enc_softmax_c4_ln_replay", "enc_softmax_weights", "model_burgers_softmax_small")
# zero_grad_params: a constant added to every key (the last bias in front of K': norm_K.*.bias with attn_norm, linears.1.bias
# without) shifts each score row uniformly, so the softmax over the keys is unchanged and that bias has a vanishing gradient
# -- the same names _linear_ref.zero_grad_params picks for the token softmax of the linear family.


def core(q, k, v, scale, m=None):
    """softmax attention on head tiles [..., n, D]: returns (O, Pm, L) with Pm = softmax(q k^T scale) .* m."""
    s = torch.einsum("...nd,...md->...nm", q, k) * scale
    p = s.softmax(dim=-1)
    pm = p if m is None else p * m.to(p.dtype)
    return torch.einsum("...nm,...md->...nd", pm, v), pm, torch.logsumexp(s, dim=-1)


def softmax_attention(sd, x, pos, *, n_head, norm=True, eps=1e-5, attn_drop=None):
    """Projections, per-head LayerNorm on Q and K, [pos, X] per head, P = softmax(Q' K'^T / sqrt(d_k + pos_dim)) over the
    keys, the attention dropout on P (layers.py:700-701), heads merged, fc."""
    B, n, d = x.shape
    dk = d // n_head
    q, k, v = (F.linear(x, sd[f"linears.{i}.weight"], sd[f"linears.{i}.bias"])
               .reshape(B, n, n_head, dk).permute(0, 2, 1, 3) for i in range(3))
    if norm:
        k = O.head_layernorm(k, *O._stack_norm(sd, "norm_K", n_head), eps)
        q = O.head_layernorm(q, *O._stack_norm(sd, "norm_Q", n_head), eps)
    use_pos = pos is not None and pos.shape[-1] > 0
    if use_pos:
        pp = pos[:, None].expand(B, n_head, n, pos.shape[-1]).to(x.dtype)
        q, k, v = (torch.cat([pp, t], dim=-1) for t in (q, k, v))
    p = (torch.einsum("bhnd,bhmd->bhnm", q, k) / math.sqrt(q.shape[-1])).softmax(dim=-1)
    p = O._apply_attn_drop(p, attn_drop)
    o = torch.einsum("bhnm,bhmd->bhnd", p, v).permute(0, 2, 1, 3).reshape(B, n, -1)
    if use_pos:
        o = F.linear(o, sd["fc.weight"], sd["fc.bias"])
    return o, p


def encoder_layer(sd, x, pos, *, n_head, attention_type="softmax", layer_norm=False, attn_norm=None, norm_eps=1e-5,
                  residual_type="add", activation_type="relu", attn_drop=None, return_attn=False, relu_mask=None):
    """The oracle's encoder_layer (every nn.Dropout the identity) around softmax_attention."""
    assert attention_type == "softmax", attention_type
    if attn_norm is None:
        attn_norm = not layer_norm
    if (not layer_norm) and (not attn_norm):
        attn_norm = True
    att, m = softmax_attention(O._sub(sd, "attn."), x, pos, n_head=n_head, norm=attn_norm, eps=norm_eps,
                               attn_drop=attn_drop)
    x = x + att if (residual_type in ("add", "plus") or residual_type is None) else x - att
    d = x.shape[-1]
    if layer_norm:
        x = F.layer_norm(x, (d,), sd["layer_norm1.weight"], sd["layer_norm1.bias"], norm_eps)
    x = x + O.feed_forward(O._sub(sd, "ff."), x, activation_type,
                           relu_mask=None if relu_mask is None else relu_mask.reshape(x.shape[0], x.shape[1], -1))
    if layer_norm:
        x = F.layer_norm(x, (d,), sd["layer_norm2.weight"], sd["layer_norm2.bias"], norm_eps)
    return (x, m) if return_attn else x


@contextlib.contextmanager
def _softmax_layers():
    """The oracle's whole-model functions call its module-level encoder_layer: route it here for the duration."""
    orig = O.encoder_layer
    O.encoder_layer = encoder_layer
    try:
        yield
    finally:
        O.encoder_layer = orig


def run_ref(g, sd, inputs, return_attn=False):
    """The restatement on one fixture of tests/golden/softmax/ (sd / inputs in any dtype; masks follow sd's dtype)."""
    drops = g.masks if g.masks else None
    if g.meta["kind"] == "encoder_layer":
        return encoder_layer(sd, inputs["x"], inputs.get("pos"), attn_drop=drops[0] if drops else None,
                             return_attn=return_attn, **enc_kwargs(g.meta))
    assert g.meta["kind"] == "simple_transformer"
    with _softmax_layers():
        return O.simple_transformer_1d(sd, g.meta["config"], inputs["node"], inputs["pos"], attn_drops=drops)


def ref_grads(g, dtype):
    """(out, {"dx"/"dnode": grad}, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    inputs = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    out = run_ref(g, sd, inputs)
    names = list(g.dparam)
    grads = torch.autograd.grad(out, [inputs[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    nin = len(g.din)
    return out.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:]))
