"""What the self- and the cross-attention node share, without a device: the call setup that turns the attention-dropout mode
into (mask, p_attn), and the core table with the config type."""
import pytest
import torch


def test_dropout_setup_cpu():
    """_attn_dropout_setup: 'reference' -> (None, 0.5), 'off' -> (None, 0), 'replay' pops exactly one queued mask per call (a
    Galerkin mask zero-padded to round4, the others handed through contiguous; an empty queue raises); kind='causal' puts
    ``keep`` in the mask slot with p_attn = 0 in every mode and leaves the queue alone; ``keep`` with another kind raises."""
    import galerkin_transformer as gt
    from galerkin_transformer.ops import attention as A
    dev = torch.device("cpu")
    keep = torch.ones(2, 9, dtype=torch.uint8)
    kinds = ("galerkin", "linear", "fourier", "softmax")
    mode = gt.get_attention_dropout()
    try:
        for m, p_attn in (("reference", 0.5), ("off", 0.0)):
            gt.set_attention_dropout(m)
            for who in ("simple_attention", "cross_attention"):
                for kind in kinds:
                    assert A._attn_dropout_setup(who, kind, None, dev) == (None, p_attn)

        gt.set_attention_dropout("replay")
        Dr = 17                                                     # pads to 20
        small = [2.0 * (torch.rand(2, 3, Dr, Dr) < 0.5).float() for _ in range(2)]
        big = [2.0 * (torch.rand(2, 3, 9, 9) < 0.5).double().transpose(-1, -2) for _ in range(2)]     # not contiguous, not fp32
        gt.push_attention_masks(small + big)
        for kind, m in zip(("galerkin", "linear"), small):
            before = len(A._attn_masks)
            mask, p_attn = A._attn_dropout_setup("simple_attention", kind, None, dev)
            assert len(A._attn_masks) == before - 1 and p_attn == 0.0
            assert mask.shape == (2, 3, 20, 20) and mask.dtype == torch.float32
            assert torch.equal(mask[..., :Dr, :Dr], m)
            assert mask.sum() == m.sum()                            # zeros everywhere else
        for kind, m in zip(("fourier", "softmax"), big):
            before = len(A._attn_masks)
            mask, p_attn = A._attn_dropout_setup("cross_attention", kind, None, dev)
            assert len(A._attn_masks) == before - 1 and p_attn == 0.0
            assert mask.is_contiguous() and mask.dtype == torch.float32 and torch.equal(mask, m.float())
        assert not A._attn_masks
        for kind in kinds:
            with pytest.raises(RuntimeError, match="no mask queued"):
                A._attn_dropout_setup("simple_attention", kind, None, dev)

        for m in ("reference", "off", "replay"):
            gt.set_attention_dropout(m)
            gt.push_attention_masks(small)
            for k in (keep, None):
                mask, p_attn = A._attn_dropout_setup("simple_attention", "causal", k, dev)
                assert mask is k and p_attn == 0.0
            assert len(A._attn_masks) == len(small)
            for who in ("simple_attention", "cross_attention"):
                for kind in kinds:
                    with pytest.raises(ValueError, match=f"{who}: keep is the key / value mask of kind='causal'"):
                        A._attn_dropout_setup(who, kind, keep, dev)
            assert len(A._attn_masks) == len(small)
    finally:
        gt.set_attention_dropout(mode)


def test_core_table_and_config_type_cpu():
    from galerkin_transformer.ops import attention as A
    assert set(A._CORES) == {"galerkin", "linear", "fourier", "softmax", "causal"}
    assert A._CORES["galerkin"] == A._CORES["linear"]
    pairs = {pair for pair in A._CORES.values()}
    assert len(pairs) == 4                                          # and no other two kinds share one
    for kind, pair in A._CORES.items():
        assert len(pair) == 2 and all(callable(f) for f in pair), kind
        assert pair[0] is not pair[1], kind
    assert A.AttnConfig._fields == ("kind", "h", "norm_mask", "eps", "sign", "p_attn", "p_out", "need_w", "token_norm", "share")
    cfg = A._config("galerkin", 4.0, True, 1, 1, 0, 0, 1, 0, "self")
    assert cfg == ("galerkin", 4, 1, 1.0, 1.0, 0.0, 0.0, True, False, "self")
    assert [type(v) for v in cfg] == [str, int, int, float, float, float, float, bool, bool, str]
