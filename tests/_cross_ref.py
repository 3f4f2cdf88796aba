"""Plain-torch restatement of cross-attention through SimpleAttention.forward(query, key, value, pos) with the three not one
tensor (reference layers.py:829-899, 672-734), in any dtype and on any device: every attention type of the HIP path, both
head norms.  Pinned against the fixtures of tests/golden/cross/ by test_cross_attention_cpu.py; reuses the oracle's pieces
and those of _linear_ref / _instance_ref where they fit."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from _instance_ref import grad_errors as instance_grad_errors
from _instance_ref import head_tokennorm
from _linear_ref import grad_errors
from _util import GOLDEN, rel_l2
from oracle import galerkin_oracle as O

CROSS_GOLDEN = ("x_galerkin_nopos", "x_galerkin_nopos_replay", "x_galerkin_nopos_wide", "x_linear_nopos",
                "x_galerkin_inst_nopos", "x_galerkin_pos", "x_linear_pos", "x_fourier_pos", "x_fourier_pos_replay",
                "x_softmax_pos", "x_galerkin_nonorm")
FAMILY = ("galerkin", "linear", "global")


def cross_attention(sd, query, key, value, pos, *, n_head, attention_type, norm=True, norm_type="layer", eps=1e-5,
                    attn_drop=None, galerkin_divisor="n_q"):
    """Q = linears[0](query), K = linears[1](key), V = linears[2](value); per-head LayerNorm (or the token-axis norm) on K, V
    for the Galerkin family, LayerNorm on Q, K otherwise; [pos, X] per head; the core; heads merged; fc (skipped without
    coordinates).  Galerkin family: M = dropout(K'^T V' / n_q) -- the sum over the n_kv memory tokens, the divisor the
    QUERY count (layers.py:719, 728); ``galerkin_divisor="n_kv"`` is the other reading, kept to pin the difference."""
    B, n_q, d = query.shape
    n_kv = key.shape[1]
    dk = d // n_head
    q, k, v = (F.linear(x, sd[f"linears.{i}.weight"], sd[f"linears.{i}.bias"])
               .reshape(B, x.shape[1], n_head, dk).permute(0, 2, 1, 3) for i, x in enumerate((query, key, value)))
    if norm and attention_type in FAMILY:
        hn = head_tokennorm if norm_type == "instance" else O.head_layernorm
        k = hn(k, *O._stack_norm(sd, "norm_K", n_head), eps)
        v = hn(v, *O._stack_norm(sd, "norm_V", n_head), eps)
    elif norm:
        k = O.head_layernorm(k, *O._stack_norm(sd, "norm_K", n_head), eps)
        q = O.head_layernorm(q, *O._stack_norm(sd, "norm_Q", n_head), eps)
    use_pos = pos is not None and pos.shape[-1] > 0
    if use_pos:
        pp = pos[:, None].expand(B, n_head, pos.shape[1], pos.shape[-1]).to(query.dtype)
        q, k, v = (torch.cat([pp, t], dim=-1) for t in (q, k, v))
    if attention_type in FAMILY:
        if attention_type != "galerkin":
            q = q.softmax(dim=-1)
            k = k.softmax(dim=-2)
        m = torch.einsum("bhnd,bhne->bhde", k, v) / dict(n_q=n_q, n_kv=n_kv)[galerkin_divisor]
        m = O._apply_attn_drop(m, attn_drop)
        o = torch.einsum("bhnd,bhde->bhne", q, m)
    else:
        s = torch.einsum("bhnd,bhmd->bhnm", q, k) / math.sqrt(q.shape[-1])
        m = s.softmax(dim=-1) if attention_type == "softmax" else s / n_kv
        m = O._apply_attn_drop(m, attn_drop)
        o = torch.einsum("bhnm,bhmd->bhnd", m, v)
    o = o.permute(0, 2, 1, 3).reshape(B, n_q, -1)
    if use_pos:
        o = F.linear(o, sd["fc.weight"], sd["fc.bias"])
    return o, m


def attn_kwargs(meta):
    return dict(n_head=meta["n_head"], attention_type=meta["attention_type"], norm=meta["norm"],
                norm_type=meta["norm_type"], eps=meta["eps"])


def golden_weight(name):
    """The attention weight the reference returned for tests/golden/cross/<name>."""
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "cross", name + ".npz"))["attn"])


def ref_grads(g, dtype, **kw):
    """(out, weight, {input: grad}, {param: grad}) of the restatement in ``dtype`` with the fixture's cotangent."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in g.sd.items()}
    ins = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    out, w = cross_attention(sd, *(ins[k] for k in g.meta["form"]), ins.get("pos"),
                             attn_drop=g.masks[0] if g.masks else None, **attn_kwargs(g.meta), **kw)
    names = [k for k in g.dparam]
    grads = torch.autograd.grad(out, [ins[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    nin = len(g.din)
    return out.detach(), w.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:]))


def param_errors(got, ref, g):
    """{name: error} of the parameter gradients.  Under a token softmax of K' ('linear' / 'global') or a softmax over the
    keys the bias in front of K' has a vanishing gradient (_linear_ref.zero_grad_params), and so have the K and V
    projection biases under the token-axis norm (_instance_ref.zero_grad_params): measured absolutely there, as the
    grad_errors of those files do; relative L2 everywhere else."""
    if g.meta["norm"] and g.meta["norm_type"] == "instance":
        return instance_grad_errors(got, ref, g.sd, g.meta["attention_type"])
    if g.meta["attention_type"] in ("linear", "global", "softmax"):
        return grad_errors(got, ref, g.sd)
    return {k: rel_l2(got[k], r) for k, r in ref.items()}


def all_errors(out, w, din, dparam, ref_out, ref_w, ref_din, ref_dparam, g):
    errs = {"out": rel_l2(out, ref_out), "attn": rel_l2(w, ref_w)}
    errs.update({"d" + k: rel_l2(din[k], v) for k, v in ref_din.items()})
    errs.update({"dW:" + k: v for k, v in param_errors(dparam, ref_dparam, g).items()})
    return errs
