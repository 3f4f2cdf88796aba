"""Module state that one operator leaves for the next: the parity sinks, the masked twins of data gradients and the
SiLU gates.  Everything here is advisory; the operators that use it live in the family modules.
"""
from __future__ import annotations

import os


# ReLU mask capture for parity runs: with a list installed, every FeedForward forward (ReLU, no hidden dropout) appends
# the boolean mask hidden > 0 it will differentiate with.  At bench sizes (~1e7 pre-activations per layer) some lie within
# fp32 rounding of the kink, where the derivative is decided by the last bit of the accumulation; the checker replays
# these decisions in its float64 model instead of comparing coin flips.
_relu_mask_sink = [None]


def set_relu_mask_sink(sink):
    """sink: a list to append the FeedForward ReLU masks to (in call order), or None to switch the capture off."""
    _relu_mask_sink[0] = sink


_scaler_mask_sink = [None]


def set_scaler_mask_sink(sink):
    """sink: a list that every scaler_conv_chain forward appends its three ReLU masks to ([B, H, W, width_i] booleans:
    output > 0, i.e. kept by the dropout and positive), or None.  Parity runs replay them in the checker, like
    set_relu_mask_sink's."""
    _scaler_mask_sink[0] = sink


# ----------------------------------------------------------------------------------- masked twins of data gradients
# A block of the encoder layer ends in  out = res + dropout(y)  (model.py:125, 132); its backward needs the incoming gradient
# twice: as it is (residual branch) and under that dropout's mask (three contractions).  The masked copy used to be one
# elementwise gt_dropout_apply pass per block and backward (12 per step at six layers).  Now the block that CONSUMES `out`
# produces it: its forward finds the mask parameters of its input registered here (keyed by the tensor's address), and the
# product of its backward that writes d(out) writes the masked copy too (gt_gemm_desc.c_masked).  Everything is advisory: a
# consumer that finds no twin for exactly its (tensor address, p, salt) -- another op in between, a gradient autograd
# accumulated from two consumers, a hook that replaced it -- runs the elementwise pass as before.
_fold_masks = [os.environ.get("GT_FOLD_MASKS", "1") != "0"]
_mask_hints = {}                # out.data_ptr() -> (p, salt, numel): "the gradient w.r.t. this tensor is wanted under this mask too"
_masked_twins = {}              # dx.data_ptr()  -> (masked copy, p, salt, dx, dx._version at the offer)


_fold_seq = [0]                 # forward blocks that use this registry, in call order


def _hint_output_mask(out, p: float, salt: int):
    """Called at the END of a block's forward.  A hint is only honoured by the very next block's forward (an address that
    the allocator hands out again later must not resurrect it), and any forward activity drops leftover twins of an earlier
    backward."""
    _masked_twins.clear()
    _mask_hints.clear()
    if _fold_masks[0] and p > 0:
        _mask_hints[out.data_ptr()] = (float(p), int(salt), out.numel(), _fold_seq[0])


def _wanted_mask(x):
    """Called at the START of a block's forward: (p, salt) under which the producer of x wants d(x) once more, or None."""
    _fold_seq[0] += 1
    e = _mask_hints.pop(x.data_ptr(), None) if _fold_masks[0] else None
    return (e[0], e[1]) if e is not None and e[2] == x.numel() and e[3] == _fold_seq[0] - 1 else None


def _offer_twin(dx, dxm, p: float, salt: int):
    """dxm = dx .* mask(p, salt), written next to dx by the product that formed dx.  The entry keeps dx itself alive until it
    is taken or dropped: a tensor that something else still refers to is never summed into by autograd (the sum of two
    consumers' gradients goes to a buffer of its own), and its address cannot be handed out again meanwhile."""
    if len(_masked_twins) > 64:
        _masked_twins.clear()
    _masked_twins[dx.data_ptr()] = (dxm, float(p), int(salt), dx, dx._version)


def _take_twin(g, p: float, salt: int):
    """The masked copy of g, if g is still, value for value, the dx it was written next to: the same memory (the entry kept
    it alive) and no in-place write since the offer (views share the version counter), else None."""
    e = _masked_twins.pop(g.data_ptr(), None) if _fold_masks[0] else None
    if (e is not None and e[1] == float(p) and e[2] == int(salt) and e[0].numel() == g.numel() and e[0].device == g.device
            and e[3].numel() == g.numel() and g._version == e[4]):
        return e[0].view(g.shape)
    return None


# What keeps the twins sound when the graph is not a plain chain (tests/test_handoff_graphs_gpu.py and tests/test_handoff_cpu.py
# hold each case):
#  * a second consumer of `out` (return_latent, a forward hook that uses it in an auxiliary loss, two following blocks):
#    autograd adds the consumers' gradients.  Left alone it does so IN PLACE, into the gradient that arrives first, when
#    nothing else refers to that tensor -- which would be the dx a twin was offered for whenever the other consumer was
#    created BEFORE the consuming block in the forward.  Two things rule that out here: the registry entry holds dx (so the
#    sum goes to a fresh buffer, under whose address no twin was offered, and the elementwise pass runs), and _take_twin
#    compares the version counter, which any in-place write to dx or a view of it bumps.  (The backward passes also return
#    dx.reshape(...), a view, which torch does not sum into either; nothing relies on that.)
#  * a tensor hook that returns a new gradient: another address while dx is alive, the same way.  A hook that only reads
#    (retain_grad, a hook returning None) sees d(out) itself: the twin is a separate buffer next to it, d(out) is never altered.
#  * a torch op between the blocks: the hint is keyed by the producer's own result, the consumer sees another tensor.
#  * a forward in between (torch.no_grad() or not): every block forward clears hints and twins first.


# ----------------------------------------------------------------------------------- SiLU gates on the producer of a gradient
# Inside a `silu_gate_scope` (SpectralRegressor's layer loop: every intermediate has exactly ONE consumer there) a Function
# whose result is silu(pre) OFFERS its pre-activation under the result's address; the Function that consumes the result
# TAKES it, and its backward multiplies the gradient it forms by silu'(pre) on the store of the kernel that forms it
# (gt_dft_synthesis_gated / gt_mlp_head_bwd_gated).  The producer's backward then receives the gradient of its
# PRE-activation (ctx.g_gated) and skips its own gt_act_bwd pass: 2 x 172 us per step at the headline shape.
#
# KNOWN LIMITS (the first one measured, the other two read from the code; nothing here guards against them): the fold is
# only right while the offered result has exactly ONE consumer, the taker.
#  * A second consumer inside the scope (a module forward hook on regressor.spectral_conv[j] that uses the layer output in an
#    auxiliary loss): the producer receives silu'(pre) . g_next + g_aux and skips its SiLU backward, so g_aux is never
#    multiplied by silu'(pre).  Parameter gradients then differ from the unfolded run by 0.5 .. 1.5 relative L2 (16 x 16
#    grid, two layers, widths 32 and 20) with no error raised.  Switch the fold off for such graphs (GT_FOLD_GATES=0, or
#    ops._gate_fold[0] = False before the forward); return_latent=True already does.
#  * A tensor hook or retain_grad() on a spectral layer's output, whenever it is registered, observes the gradient of the
#    PRE-activation (already multiplied by silu'), not d(out).
#  * An offer nobody takes (consumer without input gradient, a torch op in between, a copy made by _c()) stays here until
#    the outermost scope exits, keyed by an address the allocator may hand out again.
_gate_fold = [os.environ.get("GT_FOLD_GATES", "1") != "0"]       # A/B switch (tools / tests)
_gate_depth = [0]
_silu_gates = {}                 # data_ptr of an activated result -> (ctx of its Function, pre-activation)


class silu_gate_scope:
    def __init__(self, enabled: bool = True):
        self.on = bool(enabled) and _gate_fold[0]

    def __enter__(self):
        if self.on:
            _gate_depth[0] += 1
        return self

    def __exit__(self, *exc):
        if self.on:
            _gate_depth[0] -= 1
            if _gate_depth[0] == 0:
                _silu_gates.clear()          # offers nobody took: their producers run gt_act_bwd as ever
        return False


def _offer_gate(ctx, out, pre):
    ctx.g_gated = False
    if _gate_depth[0] > 0 and pre is not None:
        _silu_gates[out.data_ptr()] = (ctx, pre)


def _take_gate(x):
    """The pre-activation whose SiLU produced ``x`` (the caller's backward MUST multiply d(x) by silu' of it), or None."""
    if _gate_depth[0] <= 0:
        return None
    ent = _silu_gates.pop(x.data_ptr(), None)
    if ent is None or ent[1].numel() != x.numel():
        return None
    ent[0].g_gated = True
    return ent[1]
