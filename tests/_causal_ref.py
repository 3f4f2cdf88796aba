"""Plain-torch restatement of causal linear attention (reference layers.py:736-762) and of the decoder layer built on it
(reference model.py:142-241), for the causal tests.  Runs in whatever dtype its inputs have (float64 for the reference
values, float32 on the CPU for the yardstick of the GPU bars).

Closed form of the function: with keep = kv_mask (True = keep) or all ones, k^ = keep k / n, v^ = keep v,
    A = tril(q k^^T),   out = A v^ / (rowsum(A) + eps sum_d q).
The same function in the reference's own formulation, causal_ref_scan: the running states S_i = cumsum of k^_j v^_j^T and
z_i = cumsum of k^_j, out_i = S_i^T q_i / ((z_i + eps) . q_i).  In float64 the two agree to rounding; in float32 they do not
round alike (the scan form cancels S_i g_i against c_i z_i in the backward, as the reference function and the HIP kernels
do), so the float32 yardstick of the GPU bars is taken from both, and the scan form stands in for "the reference function run
in float32" where the reference does not exist: test_causal_attention_cpu pins its float32 error to the reference function's
recorded float32 results.
The module wiring carries the three repairs of INTEGRATION.md: ``mask`` of the causal type is the core's kv_mask [B, n_kv]
(not unsqueezed), the decoder's self-attention is called with mask=tgt_mask, and no dropout is drawn on the running state.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
CAUSAL_DIR = os.path.join(HERE, "golden", "causal")
CASES = ("n1_d16", "n65_d20", "n65_d20_masked", "n130_d36", "n130_d36_masked")
EPS = 1e-7


def _hats(k, v, kv_mask):
    n = k.shape[-2]
    kh = k / n
    if kv_mask is None:
        return kh, v
    keep = kv_mask[:, None, :, None]
    return kh.masked_fill(~keep, 0.0), v.masked_fill(~keep, 0.0)


def causal_ref(q, k, v, kv_mask=None, eps=EPS):
    """q, k, v [B, h, n, D]; kv_mask torch.bool [B, n] or None."""
    kh, vh = _hats(k, v, kv_mask)
    A = torch.tril(q @ kh.transpose(-1, -2))
    den = A.sum(-1) + eps * q.sum(-1)
    return (A @ vh) / den[..., None]


def causal_ref_scan(q, k, v, kv_mask=None, eps=EPS):
    """The running-state formulation (memory O(n D^2): test sizes only)."""
    kh, vh = _hats(k, v, kv_mask)
    S = (kh.unsqueeze(-1) * vh.unsqueeze(-2)).cumsum(-3)
    dinv = 1.0 / ((kh.cumsum(-2) + eps) * q).sum(-1)
    return torch.einsum("bhnd,bhnde,bhn->bhne", q, S, dinv)


FORMS = {"tril": causal_ref, "scan": causal_ref_scan}


def condition(q, k, kv_mask=None, eps=EPS):
    """max_i sum_d |(z_i[d] + eps) q_i[d]| / |den_i|: 1 for positive q, k; the tests' inputs keep it <= 2."""
    kh, _ = _hats(k, k, kv_mask)
    t = (kh.cumsum(-2) + eps) * q
    return float((t.abs().sum(-1) / t.sum(-1).abs()).max())


def causal_grads(q, k, v, kv_mask, cot, dtype, eps=EPS, form="tril"):
    """(out, dq, dk, dv) of causal_ref (or causal_ref_scan) in ``dtype`` on the CPU."""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    out = FORMS[form](q, k, v, kv_mask, eps)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), cot.to(dtype))


def causal_yardstick(q, k, v, kv_mask, cot, ref64, names=("out", "dq", "dk", "dv")):
    """Per tensor, the larger float32 error of the two formulations against the float64 values ref64 (a dict)."""
    e = {}
    for form in FORMS:
        for k_, t in zip(names, causal_grads(q, k, v, kv_mask, cot, torch.float32, form=form)):
            if float(ref64[k_].abs().max()) > 0.0:
                e[k_] = max(e.get(k_, 0.0), err(t, ref64[k_]))
    return e


class CausalGolden:
    """One fixture of tests/golden/causal: <name>.npz and, where it was split to keep files small, <name>_p<i>.npz."""

    def __init__(self, name):
        z = {}
        i = 0
        while True:
            path = os.path.join(CAUSAL_DIR, name + (".npz" if i == 0 else f"_p{i}.npz"))
            if not os.path.exists(path):
                break
            with np.load(path, allow_pickle=False) as f:
                z.update({k: f[k] for k in f.files})
            i += 1
        self.files = i
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.q, self.k, self.v, self.cot = (torch.from_numpy(z[k]).double() for k in ("q", "k", "v", "cot"))
        self.kv_mask = torch.from_numpy(z["kv_mask"]).bool() if "kv_mask" in z else None
        self.out, self.dq, self.dk, self.dv = (torch.from_numpy(z[k]) for k in ("out", "dq", "dk", "dv"))
        # the reference function's own float32 run on the same inputs
        self.f32 = {k: torch.from_numpy(z[k + "32"]) for k in ("out", "dq", "dk", "dv")}


def decoder_state_dict_shapes():
    with open(os.path.join(CAUSAL_DIR, "decoder_state_dict.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------- modules
def _heads(x, h):
    B, n, d = x.shape
    return x.view(B, n, h, d // h).transpose(1, 2)


def _head_norm(sd, prefix, x, eps):
    return torch.stack([F.layer_norm(x[:, i], x.shape[-1:], sd[f"{prefix}.{i}.weight"], sd[f"{prefix}.{i}.bias"], eps)
                        for i in range(x.shape[1])], dim=1)


def simple_attention_ref(sd, prefix, query, key, value, *, n_head, attention_type, norm, eps=1e-5, pos=None, mask=None,
                         probe=None, form="tril"):
    """SimpleAttention.forward (layers.py:829-899) for 'galerkin' and 'causal', attention dropout off.  ``probe``: a list
    that receives (q, k, mask) of every causal call, for the conditioning check."""
    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    q, k, v = (_heads(F.linear(x, sd[f"linears.{i}.weight"], sd[f"linears.{i}.bias"]), n_head)
               for i, x in enumerate((query, key, value)))
    if norm:
        if attention_type == "galerkin":
            k, v = _head_norm(sd, "norm_K", k, eps), _head_norm(sd, "norm_V", v, eps)
        else:
            k, q = _head_norm(sd, "norm_K", k, eps), _head_norm(sd, "norm_Q", q, eps)
    if pos is not None:
        pp = pos.unsqueeze(1).repeat(1, n_head, 1, 1)
        q, k, v = (torch.cat([pp, x], dim=-1) for x in (q, k, v))
    if attention_type == "galerkin":
        assert mask is None
        x = q @ (k.transpose(-1, -2) @ v / q.size(-2))
    else:
        assert attention_type == "causal"
        if probe is not None:
            probe.append((q.detach(), k.detach(), mask))
        x = FORMS[form](q, k, v, mask)
    B, _, n, D = x.shape
    x = x.transpose(1, 2).reshape(B, n, n_head * D)
    if pos is not None:
        x = F.linear(x, sd["fc.weight"], sd["fc.bias"])
    return x


def decoder_layer_ref(sd, x, memory, *, nhead, layer_norm, attn_norm, norm_eps=1e-5, memory_mask=None, probe=None,
                      form="tril"):
    """GalerkinTransformerDecoderLayer.forward in eval mode, self_attn of the default 'galerkin' type, tgt_mask None."""
    d = x.shape[-1]

    def ln(i, t):
        return F.layer_norm(t, (d,), sd[f"norm{i}.weight"], sd[f"norm{i}.bias"], norm_eps) if layer_norm else t
    kw = dict(n_head=nhead, norm=attn_norm, eps=norm_eps)
    x = ln(1, x + simple_attention_ref(sd, "self_attn.", x, x, x, attention_type="galerkin", **kw))
    x = ln(2, x + simple_attention_ref(sd, "multihead_attn.", x, memory, memory, attention_type="causal", mask=memory_mask,
                                       probe=probe, form=form, **kw))
    y = F.linear(F.relu(F.linear(x, sd["ff.lr1.weight"], sd["ff.lr1.bias"])), sd["ff.lr2.weight"], sd["ff.lr2.bias"])
    return ln(3, x + y)


def ref_and_yardstick(fn, sd, inputs, cot):
    """fn(sd, form=..., **inputs) -> out.  Returns (names, float64 results, yardstick): out, d(inputs)..., d(parameters
    used)... from autograd on the CPU in float64 (tril form), and per tensor the larger float32 error of the two
    formulations against them; parameters that take no gradient are left out."""
    def run(dtype, form):
        p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
        ins = {k: v.detach().to(dtype).requires_grad_(True) for k, v in inputs.items()}
        out = fn(p, form=form, **ins)
        leaves = list(ins.items()) + list(p.items())
        grads = torch.autograd.grad(out, [t for _, t in leaves], cot.to(dtype), allow_unused=True)
        res = {"out": out.detach()}
        res.update({"d:" + k: g for (k, _), g in zip(leaves, grads) if g is not None})
        return res
    ref64 = run(torch.float64, "tril")
    yard = {}
    for form in FORMS:
        r32 = run(torch.float32, form)
        for k, r in ref64.items():
            if float(r.abs().max()) > 0.0:
                yard[k] = max(yard.get(k, 0.0), err(r32[k], r))
    return list(ref64), ref64, yard


def err(a, ref):
    """max-abs error over max-abs of the reference."""
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())
