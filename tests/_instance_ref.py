"""Plain-torch restatement of norm_type='instance' for the Galerkin family (reference layers.py:842-854, 917-923: one
nn.InstanceNorm1d(d_k, affine=True) per head on the transposed K and V) and of the encoder layer / SimpleTransformer
around it, in any dtype and on any device.  The CPU oracle covers per-head LayerNorm only; this file restates the token-axis
norm for the tests, pinned against the fixtures of tests/golden/instance/ by test_instance_norm_cpu.py, and reuses the
oracle's and _linear_ref's unchanged pieces."""
import contextlib

import torch
import torch.nn.functional as F

from _linear_ref import enc_kwargs
from oracle import galerkin_oracle as O

INSTANCE_GOLDEN = ("enc_galerkin_inst_c2", "enc_galerkin_inst_c2_replay", "enc_galerkin_inst_c1", "enc_linear_inst_c2",
                   "enc_global_inst_c5", "enc_galerkin_inst_nopos", "enc_galerkin_inst_c4",
                   "model_burgers_galerkin_inst_small")
SHARED_INPUTS = ("enc_galerkin_inst_c2_in", "enc_linear_inst_c2_in")
FAMILY = ("galerkin", "linear", "global")


def head_tokennorm(t, gamma, beta, eps):
    """t: (B, h, n, dk); gamma / beta: (h, dk).  Per (sample, head, channel): mean and BIASED variance over the n tokens."""
    mu = t.mean(dim=2, keepdim=True)
    var = ((t - mu) ** 2).mean(dim=2, keepdim=True)
    return (t - mu) / torch.sqrt(var + eps) * gamma[None, :, None, :] + beta[None, :, None, :]


def instance_attention(sd, x, pos, *, n_head, attention_type="galerkin", norm=True, eps=1e-5, attn_drop=None):
    """Projections, token-axis norm of K and V, [pos, X] per head (after the norm: the coordinates are not normalised),
    for 'linear' / 'global' the softmax of Q over the head's columns and of K over the tokens, M = dropout(K^T V / n),
    out = Q M, heads merged, fc (skipped without coordinates)."""
    assert attention_type in FAMILY, attention_type
    B, n, d = x.shape
    dk = d // n_head
    q, k, v = (F.linear(x, sd[f"linears.{i}.weight"], sd[f"linears.{i}.bias"])
               .reshape(B, n, n_head, dk).permute(0, 2, 1, 3) for i in range(3))
    if norm:
        k = head_tokennorm(k, *O._stack_norm(sd, "norm_K", n_head), eps)
        v = head_tokennorm(v, *O._stack_norm(sd, "norm_V", n_head), eps)
    use_pos = pos is not None and pos.shape[-1] > 0
    if use_pos:
        pp = pos[:, None].expand(B, n_head, n, pos.shape[-1]).to(x.dtype)
        q, k, v = (torch.cat([pp, t], dim=-1) for t in (q, k, v))
    if attention_type != "galerkin":
        q = q.softmax(dim=-1)
        k = k.softmax(dim=-2)
    m = torch.einsum("bhnd,bhne->bhde", k, v) / n
    m = O._apply_attn_drop(m, attn_drop)
    o = torch.einsum("bhnd,bhde->bhne", q, m).permute(0, 2, 1, 3).reshape(B, n, -1)
    if use_pos:
        o = F.linear(o, sd["fc.weight"], sd["fc.bias"])
    return o, m


def encoder_layer(sd, x, pos, *, n_head, attention_type="galerkin", layer_norm=False, attn_norm=None, norm_eps=1e-5,
                  residual_type="add", activation_type="relu", attn_drop=None, return_attn=False, relu_mask=None):
    """The oracle's encoder_layer (every nn.Dropout the identity) around instance_attention."""
    if attn_norm is None:
        attn_norm = not layer_norm
    if (not layer_norm) and (not attn_norm):
        attn_norm = True
    att, m = instance_attention(O._sub(sd, "attn."), x, pos, n_head=n_head, attention_type=attention_type, norm=attn_norm,
                                eps=norm_eps, attn_drop=attn_drop)
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
def _instance_layers():
    """The oracle's whole-model functions call its module-level encoder_layer: route it here for the duration."""
    orig = O.encoder_layer
    O.encoder_layer = encoder_layer
    try:
        yield
    finally:
        O.encoder_layer = orig


def attention_type_of(g):
    return g.meta.get("attention_type") or g.meta["config"]["attention_type"]


def run_ref(g, sd, inputs):
    """The restatement on one fixture of tests/golden/instance/ (sd / inputs in any dtype; masks follow sd's dtype)."""
    drops = g.masks if g.masks else None
    if g.meta["kind"] == "encoder_layer":
        return encoder_layer(sd, inputs["x"], inputs.get("pos"), attn_drop=drops[0] if drops else None,
                             **enc_kwargs(g.meta))
    assert g.meta["kind"] == "simple_transformer"
    with _instance_layers():
        return O.simple_transformer_1d(sd, g.meta["config"], inputs["node"], inputs["pos"], attn_drops=drops)


def zero_grad_params(sd, attention_type):
    """Parameters whose gradient is ZERO in exact arithmetic with the token-axis norm on K and V: a constant added to a whole
    column does not survive the subtraction of the token mean, so the K and V projection biases (linears.1.bias,
    linears.2.bias) get sum_t dX[t, c] = 0.  For 'linear' / 'global' the token softmax behind the norm removes a constant
    per column once more: norm_K.*.bias too (the reasoning of _linear_ref.zero_grad_params).  Every float32 evaluation, the
    reference's included, returns round-off there, so a RELATIVE error of such a tensor means nothing."""
    names = set()
    for k in sd:
        if k.endswith("linears.1.bias") or k.endswith("linears.2.bias"):
            if any(j.startswith(k[:-len("linears.1.bias")] + "norm_K.") for j in sd):
                names.add(k)
        if attention_type != "galerkin" and ".norm_K." in "." + k and k.endswith(".bias"):
            names.add(k)
    return names


def grad_errors(got, ref, sd, attention_type):
    """_linear_ref.grad_errors with the name set of zero_grad_params above: relative L2, except for those parameters, whose
    ABSOLUTE error is taken relative to the size the same sum has without the cancellation -- the gradient of the sibling
    weight (for a Linear: per input feature, |dW| / sqrt(fan_in)).  The same bars then apply to both kinds."""
    zero = zero_grad_params(sd, attention_type)
    errs = {}
    for k, r in ref.items():
        a, r = got[k].detach().double().cpu(), r.detach().double().cpu()
        if k in zero:
            w = ref[k[:-len("bias")] + "weight"].detach().double()
            scale = float(w.norm()) / (w.shape[1] ** 0.5 if w.dim() == 2 else 1.0)
            errs[k] = float((a - r).norm()) / scale
        else:
            errs[k] = float((a - r).norm()) / (float(r.norm()) or 1.0)
    return errs


def ref_grads(g, dtype):
    """(out, {"dx"/"dnode": grad}, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    inputs = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    out = run_ref(g, sd, inputs)
    names = list(g.dparam)
    grads = torch.autograd.grad(out, [inputs[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    nin = len(g.din)
    return out.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:]))
