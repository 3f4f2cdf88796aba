"""Plain-torch restatement of batch_norm=True of FeedForward (reference layers.py:979-987: nn.BatchNorm1d(dim_feedforward)
on the transposed hidden tensor, behind the hidden dropout) -- forward, gradients (through autograd) and the buffer updates --
and of the encoder layer / SimpleTransformer around it, in any dtype and on any device.  The CPU oracle has no such norm;
this file restates it for the tests, pinned against the fixtures of tests/golden/batchnorm/ by test_batchnorm_cpu.py, and
reuses the oracle's unchanged pieces (its encoder_layer and whole-model functions call its module-level feed_forward, which
is routed here for the duration of a run)."""
import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

from _linear_ref import enc_kwargs
from _util import GOLDEN
from oracle import galerkin_oracle as O

BATCHNORM_CASES = ("ff_bn_relu", "ff_bn_silu", "enc_galerkin_bn_c2", "model_burgers_bn_small")
BATCHNORM_GOLDEN = tuple(c + s for c in BATCHNORM_CASES for s in ("", "_eval"))      # <case>: train(), <case>_eval: eval()
SHARED_INPUTS = tuple(c + "_in" for c in BATCHNORM_CASES)
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
MOMENTUM, EPS = 0.1, 1e-5           # nn.BatchNorm1d's defaults: the reference's constructor passes neither


def batch_norm_rows(h, weight, bias, running_mean, running_var, training, momentum=MOMENTUM, eps=EPS):
    """h [..., f]: one mean and one BIASED variance per channel over every other axis.  Returns (z, (new running_mean, new
    running_var)) -- the second is None in eval mode, where the running buffers are the statistics."""
    f = h.shape[-1]
    new = None
    if training:
        rows = h.reshape(-1, f)
        T = rows.shape[0]
        mean = rows.mean(dim=0)
        var = ((rows - mean) ** 2).mean(dim=0)
        with torch.no_grad():
            new = ((1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var * T / (T - 1))
    else:
        mean, var = running_mean, running_var
    return (h - mean) / torch.sqrt(var + eps) * weight + bias, new


def feed_forward_bn(sd, x, activation="relu", training=True, momentum=MOMENTUM, eps=EPS, drop_mask=None, updates=None):
    """lr1 -> act -> [* drop_mask] -> BatchNorm1d -> lr2 on the state_dict of one FeedForward.  drop_mask: the hidden
    dropout's multiplicative mask (0 or 1 / (1 - p)), in FRONT of the norm.  updates: a list that receives
    (running_mean, running_var) after a training-mode call."""
    h = O._act(activation, "relu")(F.linear(x, sd["lr1.weight"], sd["lr1.bias"]))
    if drop_mask is not None:
        h = h * drop_mask.to(h.dtype).reshape(h.shape)
    z, new = batch_norm_rows(h, sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"], training,
                             momentum, eps)
    if new is not None and updates is not None:
        updates.append(new)
    return F.linear(z, sd["lr2.weight"], sd["lr2.bias"])


@contextlib.contextmanager
def _bn_layers(training, updates):
    orig = O.feed_forward

    def ff(sd, x, activation="relu", relu_mask=None):
        assert relu_mask is None and "bn.weight" in sd
        return feed_forward_bn(sd, x, activation, training, updates=updates)

    O.feed_forward = ff
    try:
        yield
    finally:
        O.feed_forward = orig


def bn_prefixes(sd):
    """'...bn.' of every norm in state_dict order, which is the order the layers run in."""
    return [k[:-len("running_mean")] for k in sd if k.endswith("bn.running_mean")]


def run_ref(g, sd, inputs, updates=None):
    """The restatement on one fixture of tests/golden/batchnorm/ (sd / inputs in any dtype)."""
    training, kind = g.meta["training"], g.meta["kind"]
    if kind == "feed_forward":
        return feed_forward_bn(sd, inputs["x"], g.meta["activation"], training, updates=updates)
    with _bn_layers(training, updates):
        if kind == "encoder_layer":
            return O.encoder_layer(sd, inputs["x"], inputs.get("pos"), **enc_kwargs(g.meta))
        assert kind == "simple_transformer"
        return O.simple_transformer_1d(sd, g.meta["config"], inputs["node"], inputs["pos"])


def ref_grads(g, dtype):
    """(out, {"x" / "node": grad}, {param: grad}, {buffer: value after the call}) of the restatement in ``dtype`` with the
    fixture's cotangent.  The buffers come back for every norm; in eval mode they are the ones that went in."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in g.sd.items()}
    names = list(g.dparam)
    for k in names:
        sd[k].requires_grad_(True)
    inputs = {k: (v.to(dtype).clone().requires_grad_(True) if k in g.din else v.to(dtype)) for k, v in g.inputs.items()}
    updates = []
    out = run_ref(g, sd, inputs, updates)
    grads = torch.autograd.grad(out, [inputs[k] for k in g.din] + [sd[k] for k in names], g.cot.to(dtype))
    bufs = {k: v.detach().clone() for k, v in sd.items() if k.rsplit(".", 1)[-1] in BUFFERS}
    pre = bn_prefixes(sd)
    assert len(updates) == (len(pre) if g.meta["training"] else 0)
    for p, (rm, rv) in zip(pre, updates):
        bufs[p + "running_mean"], bufs[p + "running_var"] = rm, rv
        bufs[p + "num_batches_tracked"] = sd[p + "num_batches_tracked"] + 1
    nin = len(g.din)
    return out.detach(), dict(zip(g.din, grads[:nin])), dict(zip(names, grads[nin:])), bufs


def buffers_after(name):
    """The buffers the reference held after its training-mode call (`buf1/` of the train fixture)."""
    z = np.load(os.path.join(GOLDEN, "batchnorm", name + ".npz"))
    return {k[5:]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith("buf1/")}


def grad_errors(got, ref):
    """Relative L2 per parameter.  No gradient vanishes here: the activation sits between lr1 and the norm."""
    return {k: float((got[k].detach().double().cpu() - r.detach().double().cpu()).norm()) / (float(r.double().norm()) or 1.0)
            for k, r in ref.items()}
