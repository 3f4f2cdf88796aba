"""Random-feature attention ('rfa' / 'favor') restated from its formulas in plain torch, any dtype (the tests use float64):
the oracle for shapes without a fixture, itself held to the fixtures of tests/golden/rfa/ at 1e-12 (test_rfattn_cpu.py).

With d = d_model, m = d features, Om [d, m/2], s = d^(-1/4), per sample:
    u(z) = (s z) Om;   rfa: phi = sqrt(2/m) [cos u, sin u];   favor: phi = [exp(u - c), exp(-u - c)], c = s^2 |z|^2 / 2 + log(m) / 2
    KV = phi(k)^T v,  ksum = sum_tokens phi(k),  den = phi(q) . ksum + eps,  out = phi(q) KV / den
    y = [out, pos] Wout^T + bout
"""
import glob
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import galerkin_oracle as O

RFA_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfa")


def phi(z, omega, kind):
    d = z.shape[-1]
    m = 2 * omega.shape[-1]
    zs = z * d ** -0.25
    u = zs @ omega
    if kind == "rfa":
        return math.sqrt(2.0 / m) * torch.cat([torch.cos(u), torch.sin(u)], dim=-1)
    assert kind == "favor", kind
    c = 0.5 * (zs * zs).sum(-1, keepdim=True) + 0.5 * math.log(m)
    return torch.cat([torch.exp(u - c), torch.exp(-u - c)], dim=-1)


def kva(k, v, omega, kind):
    """[B, m, d + 4]: KV, the column sums of phi(k), three zero columns -- the layout of gt_rfattn_kv."""
    pk = phi(k, omega, kind)
    B, _, d = v.shape
    va = torch.cat([v, torch.ones_like(v[..., :1]), torch.zeros(B, v.shape[1], 3, dtype=v.dtype)], dim=-1)
    return pk.transpose(1, 2) @ va


def core(q, k, v, omega, kind, eps=1e-6):
    """(out [B, n, d], den [B, n], KVa [B, m, d + 4]) for q, k, v [B, n, d]."""
    d = q.shape[-1]
    M = kva(k, v, omega, kind)
    pq = phi(q, omega, kind)
    den = (pq @ M[:, :, d].unsqueeze(-1)).squeeze(-1) + eps
    return (pq @ M[:, :, :d]) / den.unsqueeze(-1), den, M


def core_grads(q, k, v, omega, kind, dout, eps=1e-6):
    """dQ, dK, dV of sum(out * dout), and dKVa = phi(q)^T [dout / den, -(dout . out) / den, 0, 0, 0]."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out, den, _ = core(q, k, v, omega, kind, eps)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout)
    out, den = out.detach(), den.detach()
    g = torch.cat([dout / den.unsqueeze(-1), -((dout * out).sum(-1) / den).unsqueeze(-1),
                   torch.zeros(*dout.shape[:2], 3, dtype=dout.dtype)], dim=-1)
    dkva = phi(q.detach(), omega, kind).transpose(1, 2) @ g
    return dq, dk, dv, dkva


def attention(sd, x, pos, kind, eps=1e-6, return_den=False):
    """RandomFourierAttention from its state dict (query / key / value / out_projection.*, feature_map.omega)."""
    q = F.linear(x, sd["query_projection.weight"], sd["query_projection.bias"])
    k = F.linear(x, sd["key_projection.weight"], sd["key_projection.bias"])
    v = F.linear(x, sd["value_projection.weight"], sd["value_projection.bias"])
    out, den, _ = core(q, k, v, sd["feature_map.omega"], kind, eps)
    y = F.linear(torch.cat([out, pos.to(out.dtype)], dim=-1), sd["out_projection.weight"], sd["out_projection.bias"])
    return (y, den) if return_den else y


def encoder_layer(sd, x, pos, kind, norm_eps=1e-5, activation="relu"):
    """Post-norm: x = LN1(x + attn(x, pos)); x = LN2(x + ff(x)), every nn.Dropout the identity."""
    d = x.shape[-1]
    x = x + attention(O._sub(sd, "attn."), x, pos, kind)
    x = F.layer_norm(x, (d,), sd["layer_norm1.weight"], sd["layer_norm1.bias"], norm_eps)
    x = x + O.feed_forward(O._sub(sd, "ff."), x, activation)
    return F.layer_norm(x, (d,), sd["layer_norm2.weight"], sd["layer_norm2.bias"], norm_eps)


def model(sd, cfg, node, pos):
    x = torch.cat([node, pos.to(node.dtype)], dim=-1)
    x = F.linear(x, sd["feat_extract.id.weight"], sd["feat_extract.id.bias"])
    for i in range(cfg["num_encoder_layers"]):
        x = encoder_layer(O._sub(sd, f"encoder_layers.{i}."), x, pos, cfg["attention_type"])
    return O.spectral_regressor(O._sub(sd, "regressor."), x, None, modes=cfg["fourier_modes"],
                                num_spectral_layers=cfg["num_regressor_layers"], spacial_dim=cfg.get("spacial_dim") or 1,
                                spacial_fc=False, activation=cfg.get("regressor_activation"))


# ------------------------------------------------------------------------------------------------- fixtures
FIXTURES = tuple(f"{what}_{kind}" for what in ("attn", "layer", "model") for kind in ("rfa", "favor"))


class RfaGolden:
    """One fixture of tests/golden/make_golden_rfa.py: <name>.npz and its continuation files <name>_p<i>.npz (a file stays
    under 1 MiB).  sd (float32 parameters and the recorded omega buffers), inputs (float32), out / cot / din / dparam
    (float64), meta with the per-tensor ``noise`` of the reference's own float32 run."""

    def __init__(self, name):
        files = [os.path.join(RFA_GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(RFA_GOLDEN, name + "_p[0-9]*.npz")))
        z = {}
        for f in files:
            with np.load(f) as part:
                z.update({k: part[k] for k in part.files})
        t = lambda a: torch.from_numpy(np.array(a))
        self.name = name
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.kind = self.meta["attention_type"]
        self.sd = {k[3:]: t(v) for k, v in z.items() if k.startswith("sd/")}
        self.inputs = {k[3:]: t(v) for k, v in z.items() if k.startswith("in/")}
        self.out, self.cot = t(z["out"]), t(z["cot"])
        self.din = {k[4:]: t(v) for k, v in z.items() if k.startswith("din/")}
        self.dparam = {k[7:]: t(v) for k, v in z.items() if k.startswith("dparam/")}
        self.noise = self.meta["noise"]

    def run(self, sd, x, pos):
        """The restatement on this fixture's kind of module; x is the differentiable input (``x`` or ``node``)."""
        what = self.meta["what"]
        if what == "attn":
            return attention(sd, x, pos, self.kind, self.meta["eps"])
        if what == "layer":
            return encoder_layer(sd, x, pos, self.kind)
        return model(sd, self.meta["config"], x, pos)

    def restated(self, dtype=torch.float64):
        """(out, dx, {param: grad}) of the restatement in ``dtype`` on the fixture's inputs and cotangent."""
        sd = {k: v.to(dtype) for k, v in self.sd.items()}
        names = [k for k in sd if k in self.dparam]
        for k in names:
            sd[k].requires_grad_(True)
        xname = "node" if self.meta["what"] == "model" else "x"
        x = self.inputs[xname].to(dtype).requires_grad_(True)
        out = self.run(sd, x, self.inputs["pos"].to(dtype))
        grads = torch.autograd.grad(out, [x] + [sd[k] for k in names], self.cot.to(dtype))
        return out.detach(), grads[0], dict(zip(names, grads[1:]))
