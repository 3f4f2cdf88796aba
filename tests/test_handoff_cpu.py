"""The masked twins of galerkin_transformer.ops._handoff, driven on the CPU through the event orders of
tests/test_handoff_graphs_gpu.py: a hint that survives a forward it was not meant for, another tensor at a hinted address,
a twin offered for a gradient that is then replaced by a sum or by a hook's result.  The registries are plain Python."""
import torch

from galerkin_transformer import ops


def _mask_reset():
    ops._mask_hints.clear()
    ops._masked_twins.clear()


def test_a_mask_hint_is_honoured_by_the_very_next_block_forward_only_cpu():
    old = ops._fold_masks[0]
    try:
        ops._fold_masks[0] = True
        _mask_reset()
        out = torch.zeros(4, 8)
        ops._hint_output_mask(out, 0.1, 7)
        assert ops._wanted_mask(out.view(32)) == (0.1, 7)               # the block's own dense view of it
        assert ops._wanted_mask(out) is None                            # once
        ops._hint_output_mask(out, 0.1, 9)
        assert ops._wanted_mask(torch.zeros(4, 8)) is None              # a forward it was not meant for ...
        assert ops._wanted_mask(out) is None                            # ... outlives the hint
        ops._hint_output_mask(out, 0.1, 11)
        assert ops._wanted_mask(out[:2]) is None                        # same address, another size
        ops._hint_output_mask(out, 0.0, 13)                             # no dropout: nothing wanted
        assert ops._wanted_mask(out) is None
        ops._hint_output_mask(out, 0.1, 15)
        ops._hint_output_mask(torch.zeros(2), 0.1, 17)                  # any block forward drops the hint before it
        assert ops._wanted_mask(out) is None
        ops._fold_masks[0] = False
        ops._hint_output_mask(out, 0.1, 19)
        assert ops._wanted_mask(out) is None and not ops._mask_hints
    finally:
        ops._fold_masks[0] = old
        _mask_reset()


def test_a_twin_is_only_handed_to_the_gradient_it_was_written_next_to_cpu():
    old = ops._fold_masks[0]
    try:
        ops._fold_masks[0] = True
        _mask_reset()
        dx, dxm = torch.ones(4, 8), torch.full((4, 8), 2.0)
        ops._offer_twin(dx, dxm, 0.1, 7)
        got = ops._take_twin(dx.view(2, 16), 0.1, 7)
        assert got.data_ptr() == dxm.data_ptr() and got.shape == (2, 16)
        assert ops._take_twin(dx, 0.1, 7) is None                       # once
        ops._offer_twin(dx, dxm, 0.1, 7)
        total = dx + torch.ones(4, 8)                                   # a second consumer: autograd hands on the sum
        assert ops._take_twin(total, 0.1, 7) is None
        assert ops._take_twin(2 * dx, 0.1, 7) is None                   # a hook that returned a new gradient
        assert ops._take_twin(dx, 0.1, 8) is None                       # another block's mask: refused, and used up
        assert ops._take_twin(dx, 0.1, 7) is None
        ops._offer_twin(dx, dxm, 0.1, 7)
        ops._hint_output_mask(torch.zeros(2), 0.1, 21)                  # a forward between two backwards drops leftovers
        assert ops._take_twin(dx, 0.1, 7) is None
        ops._offer_twin(dx, dxm, 0.1, 7)
        ops._fold_masks[0] = False
        assert ops._take_twin(dx, 0.1, 7) is None
    finally:
        ops._fold_masks[0] = old
        _mask_reset()


def test_a_twin_is_refused_after_an_in_place_write_to_its_gradient_cpu():
    """What autograd's in-place accumulation would look like from here: the same address, other values, a bumped version
    counter (shared by every view)."""
    old = ops._fold_masks[0]
    try:
        ops._fold_masks[0] = True
        _mask_reset()
        dx, dxm = torch.ones(4, 8), torch.full((4, 8), 2.0)
        ops._offer_twin(dx, dxm, 0.1, 7)
        dx.add_(1.0)
        assert ops._take_twin(dx, 0.1, 7) is None
        ops._offer_twin(dx, dxm, 0.1, 7)
        dx.view(32)[3] = 5.0                                            # through a view
        assert ops._take_twin(dx.view(2, 16), 0.1, 7) is None
        ops._offer_twin(dx, dxm, 0.1, 7)
        assert ops._take_twin(dx.view(2, 16), 0.1, 7) is not None
    finally:
        ops._fold_masks[0] = old
        _mask_reset()


def _mask(p, salt, shape):
    keep = torch.rand(shape, generator=torch.Generator().manual_seed(salt), dtype=torch.float64) >= p
    return keep.to(torch.float64) / (1.0 - p)


class _Block(torch.autograd.Function):
    """out = x + mask . (w x): the registry protocol of the encoder blocks (ops.FeedForwardFn / SimpleAttentionFn) in torch.
    Its backward hands back the bare dx it offered a twin for -- no reshape view in between, the case autograd would sum
    into in place if nothing else held that tensor."""
    taken = []

    @staticmethod
    def forward(ctx, x, w, p, salt):
        ctx.save_for_backward(x, w)
        ctx.mask, ctx.want = (p, salt), ops._wanted_mask(x)
        out = x + _mask(p, salt, x.shape) * (w * x)
        ops._hint_output_mask(out, p, salt)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gm = ops._take_twin(g, *ctx.mask)
        _Block.taken.append(gm is not None)
        if gm is None:
            gm = g * _mask(*ctx.mask, g.shape)
        dx = g + gm * w
        if ctx.want is not None:
            ops._offer_twin(dx, dx * _mask(*ctx.want, dx.shape), *ctx.want)
        return dx, (gm * x).sum(), None, None


def _two_blocks(order, fold, hook=False):
    ops._fold_masks[0] = fold
    _mask_reset()
    _Block.taken.clear()
    x = torch.randn(4, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64).requires_grad_()
    w = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (0.7, -1.3)]
    c = torch.linspace(-1, 1, 32, dtype=torch.float64).view(4, 8)
    x1 = _Block.apply(x, w[0], 0.25, 11)
    if hook:
        x1.register_hook(lambda g: 2 * g)
    aux = (c * x1).sum() if order == "aux_first" else 0.0     # a forward hook's auxiliary loss: before the next block runs
    out = _Block.apply(x1, w[1], 0.25, 13)
    if order == "aux_last":
        aux = (c * x1).sum()
    (out.sum() + aux).backward()
    return [x.grad, w[0].grad, w[1].grad], list(_Block.taken)


def test_twins_through_a_real_backward_in_both_orders_of_a_second_consumer_cpu():
    """aux_first is the order in which the consuming block's dx reaches autograd's buffer first, i.e. the one a sum in place
    would corrupt under the twin's address."""
    old = ops._fold_masks[0]
    try:
        for order, hook, fires in (("plain", False, True), ("aux_first", False, False), ("aux_last", False, False),
                                   ("plain", True, False), ("aux_first", True, False)):
            ref, _ = _two_blocks(order, False, hook)
            got, taken = _two_blocks(order, True, hook)
            assert taken == [False, fires], (order, hook, taken)            # (block 1 has no consumer, block 0 maybe)
            for a, b in zip(got, ref):
                assert torch.equal(a, b), (order, hook)
    finally:
        ops._fold_masks[0] = old
        _mask_reset()
