"""The 64- / 96-wide head tiles of the two-term fp16 Fourier kernels (DP = 68, 100; csrc/gt_fourier16.hip), host side: the
library's own answer to "which widths have instances", the Python tuples that route on it, and the lane models of
tests/test_lane_models_cpu.py (parametric in DP) at the two new widths, where NM = 2 / 3 and ND = 5 / 7 are values neither
the pre-split's image loops nor the kernel's fragment loops had taken before.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import test_lane_models_cpu as lane


def _image_bytes():
    from galerkin_transformer import _hip
    fn = ctypes.CDLL(_hip.lib_path()).gt_fourier16_image_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] * 4
    return fn


def test_image_bytes_knows_the_wide_tiles():
    """gt_fourier16_image_bytes is the library's list of instances: header (8 bytes per tile, rounded up to 1 KiB) + one image
    per (batch, head, 32-row tile); 0 for a width nobody builds."""
    fn = _image_bytes()
    B, n, h = 3, 1000, 2
    ntile = (n + 31) // 32
    hdr = (B * h * ntile * 8 + 1023) // 1024 * 1024
    for DP, img in ((20, 7 * 1024), (36, 11 * 1024), (52, 15 * 1024), (68, 19 * 1024), (100, 27 * 1024)):
        g = lane._f16_geom(DP)
        assert 32 * (g["RM_G"] + g["TR_G"]) == img                          # two planes of 16-byte granules
        assert fn(B, n, h, DP) == hdr + B * h * ntile * img, DP
    for DP in (84, 64, 96, 32, 116, 132, 0, 4):
        assert fn(B, n, h, DP) == 0, DP
    assert fn(0, n, h, 68) == 0 and fn(B, 0, h, 100) == 0


def test_python_routing_tuples():
    """FOURIER_DP keys the fp32-MFMA Fourier kernel and the Galerkin backward kernels, which get no wide instance: it stays as
    it was, and the fp16 kernel's widths live in a tuple of their own."""
    from galerkin_transformer import _hip
    assert _hip.FOURIER_DP == (20, 36, 52)
    assert _hip.FOURIER16_DP == (20, 36, 52, 68, 100)
    assert _hip.ABI_VERSION == 21
    for dk in (64, 96):
        for p in (1, 2):
            assert not _hip.galerkin_dkv_ln_supported(dk, p, 0b110)
            assert _hip.round4(dk + p) in _hip.FOURIER16_DP
    assert _hip.galerkin_dkv_ln_supported(32, 2, 0b110) and not _hip.galerkin_dkv_ln_supported(32, 2, 0b010)


@pytest.mark.parametrize("DP", [68, 100])
def test_presplit_image_maps_at_wide_tiles(DP):
    """fourier16_presplit_kernel's index maps at NM = 2 / 3 (one tail granule per row, TG = 1): every granule of both layouts
    is written exactly once per plane, the rm image returns X (main k-steps and the zero-padded tail), the tr image returns
    (-1)^col X in the row order 16 (e >> 2) + 4 kq + (e & 3) of the first product's result registers, columns >= DP are zeros."""
    g = lane._f16_geom(DP)
    NM, TG, MAIN_G, TAIL_G, RM_G, TR_G, ND = (g[k] for k in ("NM", "TG", "MAIN_G", "TAIL_G", "RM_G", "TR_G", "ND"))
    assert (NM, TG, ND) == ((2, 1, 5) if DP == 68 else (3, 1, 7))
    assert (2 * RM_G * 16) % 1024 == 0 and (2 * TR_G * 16) % 1024 == 0      # whole 1 KiB direct-to-LDS chunks
    rng = np.random.default_rng(DP)
    X = rng.standard_normal((45, DP))                                       # tile 1 has 13 live rows
    for tile in (0, 1):
        img, ex, ln = lane._f16_presplit(X, tile, DP)
        assert img.shape == (2 * RM_G + 2 * TR_G, 8)
        s = np.zeros((32, DP))
        rows = X[32 * tile:32 * tile + 32]
        s[:len(rows)] = rows
        sc = np.exp2(ex)
        assert 2.0 ** 13 <= np.abs(s).max() * sc < 2.0 ** 14
        assert np.sqrt((s * s).sum(1).max()) * sc < 2.0 ** ln
        val = lambda i0, i1: (img[i0] + img[i1]) / sc                       # two-term value of a granule
        for row in range(32):
            for q in range(4 * NM):
                gi = row * 4 * NM + q
                assert np.allclose(val(gi, MAIN_G + gi), s[row, 8 * q:8 * q + 8], rtol=2e-6, atol=2.0 ** -23 / sc)
            t = 2 * MAIN_G + row * TG
            tail = np.zeros(8)
            tail[:DP - 32 * NM] = s[row, 32 * NM:]
            assert np.allclose(val(t, t + TAIL_G), tail, rtol=2e-6, atol=2.0 ** -23 / sc)
        for dt in range(ND):
            for m in range(16):
                for kq in range(4):
                    gr = 2 * RM_G + 64 * dt + 4 * m + kq
                    col = 16 * dt + m
                    want = np.zeros(8)
                    if col < DP:
                        rws = [16 * (e >> 2) + 4 * kq + (e & 3) for e in range(8)]
                        want = (-1.0 if col & 1 else 1.0) * s[rws, col]
                    assert np.allclose(val(gr, gr + TR_G), want, rtol=2e-6, atol=2.0 ** -23 / sc)


@pytest.mark.parametrize("DP,n,mode", [(68, 40, "plain"), (100, 40, "plain"), (68, 44, "block_key"), (100, 36, "block_query")])
def test_lane_map_at_wide_tiles(DP, n, mode):
    """The whole single pass of fourier16_kernel on the lane model (fragment offsets into the images, tail k-step, the D-layout
    -> B-layout hand-over, running exponent, chain sign, block-mask bookkeeping) at the new widths, against the plain product
    -- the model and its 2e-6 bar are those of test_lane_models_cpu.test_fourier16_lane_map."""
    lane.test_fourier16_lane_map(DP, n, mode)
