"""The fp32-MFMA Fourier kernel at the 64- / 96-wide head tiles (DP = 68, 100; gt_fourier_attn_wide in csrc/gt_fourier.hip),
host side: the entry point (declared, bound, exported, same signature as the narrow one), the width tuples, the symbol pick
of H.fourier_attn, and the operator's gates on a CPU call in `f32` mode.  No GPU needed."""
import ctypes
import os

import pytest
import torch


def test_wide_symbol_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    lib = ctypes.CDLL(_hip.lib_path())
    assert hasattr(lib, "gt_fourier_attn_wide")                    # the built library exports it
    assert "gt_fourier_attn_wide(" in hdr and "gt_fourier_attn(" in hdr
    assert "gt_fourier_attn_wide" in _hip.EXPORTED_SYMBOLS
    assert _hip._PROTOS["gt_fourier_attn_wide"] == _hip._PROTOS["gt_fourier_attn"]      # same signature
    assert _hip.lib().gt_abi_version() == 21 and _hip.ABI_VERSION == 21                 # symbols are only added


def test_width_tuples():
    from galerkin_transformer import _hip
    assert _hip.FOURIER_DP_WIDE == (68, 100)
    assert _hip.FOURIER_DP == (20, 36, 52)
    assert _hip.FOURIER16_DP == (20, 36, 52, 68, 100)


def test_entry_point_follows_the_width():
    from galerkin_transformer import _hip
    for DP in _hip.FOURIER_DP_WIDE:
        assert _hip._fourier_sym(DP) == "gt_fourier_attn_wide"
    for DP in _hip.FOURIER_DP + (16, 44, 84, 116):          # unsupported widths go to the narrow symbol: GT_ENOTSUP there
        assert _hip._fourier_sym(DP) == "gt_fourier_attn"


def test_cpu_call_reaches_the_operator_in_f32_mode():
    """The shipped ex1 shape (d_model 96, one head, one coordinate: DP = 100) passes every Python-side gate in `f32` mode and
    stops at the HIP operator's device check."""
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    layer = gt.SimpleTransformerEncoderLayer(d_model=96, n_head=1, pos_dim=1, attention_type="fourier")
    old = _hip.set_precision("f32")
    try:
        with pytest.raises(RuntimeError, match="no CPU fallback") as e:
            layer(torch.randn(1, 8, 96), torch.rand(1, 8, 1))
        assert not isinstance(e.value, NotImplementedError)
    finally:
        _hip.set_precision(old)
    assert _hip.get_precision() == old
