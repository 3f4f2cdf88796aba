"""Spectral mode mixing at any channel width, host side: gt_modemix_plan (the one route pick behind gt_modemix_fwd,
gt_modemix_bwd and gt_modemix_bwd_ws_bytes) keeps every width that ran before on the resident-weight kernels, sends the
widths those refused to the tiled kernels, and agrees with the workspace query.  No GPU needed: the plan touches no device."""
import ast
import ctypes
import json
import os

import pytest
import torch

from _util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDENT, TILED = 0, 1


@pytest.fixture(scope="module")
def H():
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


def test_plan_declared_bound_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "gt_hip.h")).read()
    assert "gt_modemix_plan(" in hdr and "GT_MODEMIX_RESIDENT = 0" in hdr and "GT_MODEMIX_TILED = 1" in hdr
    assert "gt_modemix_plan" in H.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(H.lib_path()), "gt_modemix_plan")
    assert len(H._PROTOS["gt_modemix_plan"][1]) == 7
    assert (H.MODEMIX_RESIDENT, H.MODEMIX_TILED) == (RESIDENT, TILED)
    assert H.lib().gt_abi_version() == 21 and H.ABI_VERSION == 21          # the symbol is only added
    # the three other entry points keep their signatures
    assert len(H._PROTOS["gt_modemix_fwd"][1]) == 13 and len(H._PROTOS["gt_modemix_bwd"][1]) == 17
    assert len(H._PROTOS["gt_modemix_bwd_ws_bytes"][1]) == 4


def _test_modemix_cases():
    """The (B, Cin, Cout, Q, qtot, qoff) list of tests/test_kernels_gpu.py::test_modemix, read from its decorator."""
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_kernels_gpu.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "test_modemix")
    (deco,) = fn.decorator_list
    assert ast.literal_eval(deco.args[0]) == "B,Cin,Cout,Q,qtot,qoff"
    return ast.literal_eval(deco.args[1])


def _model_layers():
    """(label, Cin, Cout, Q per mode-mix call) of every spectral layer of the config.yml models and of the ex4 model, read
    off the fourier_weight parameters of the constructed models."""
    import yaml
    import galerkin_transformer as gt
    with open(os.path.join(ROOT, "galerkin-transformer_amd", "config.yml")) as f:
        cfgs = yaml.full_load(f)
    with open(os.path.join(GOLDEN, "host_init_hashes.json")) as f:
        recorded = json.load(f)
    models = {"ex1_burgers": gt.SimpleTransformer(**cfgs["ex1_burgers"])}
    for name in ("ex2_darcy", "ex3_darcy_inv"):
        cfg = dict(cfgs[name])
        for k in ("downscaler_size", "upscaler_size"):       # set by the example scripts from the grid sizes
            v = recorded[name]["config"][k]
            cfg[k] = tuple(tuple(s) if isinstance(s, list) else s for s in v) if isinstance(v, list) else v
        models[name] = gt.FourierTransformer2D(**cfg)
    models["ex4_ns_lite"] = gt.FourierTransformer2DLite(**recorded["ex4_ns_lite"]["config"])      # the ex4 script's defaults
    out = []
    for name, m in models.items():
        for k, p in m.named_parameters():
            if "fourier_weight" in k:
                assert p.shape[-1] == 2
                out.append((f"{name}:{k}", p.shape[0], p.shape[1], int(torch.tensor(p.shape[2:-1]).prod())))
    return out


def test_every_width_that_ran_before_stays_resident(H):
    cases = _test_modemix_cases()
    assert len(cases) == 6
    for B, Cin, Cout, Q, _, _ in cases:
        fwd, bwd, slices = H.modemix_plan(B, Q, Cin, Cout)
        assert (fwd, bwd) == (RESIDENT, RESIDENT), (B, Cin, Cout, Q)
        assert slices == max(1, min(-(-768 // Q), -(-B // 8)))          # the slicing rule of the resident kernels
    layers = _model_layers()
    names = {n.split(":")[0] for n, *_ in layers}
    assert {"ex1_burgers", "ex2_darcy", "ex4_ns_lite"} <= names, names       # (ex3's decoder is pointwise: no spectral layer)
    assert (96, 48) in {(ci, co) for _, ci, co, _ in layers}                 # the widest shipped layer was read, not skipped
    for label, Cin, Cout, Q in layers:
        for B in (1, 4, 16):
            assert H.modemix_plan(B, Q, Cin, Cout)[:2] == (RESIDENT, RESIDENT), (label, B)


@pytest.mark.parametrize("Cin,Cout,fwd,bwd", [(96, 64, RESIDENT, RESIDENT),      # 6144 pairs: the last resident backward
                                              (96, 80, RESIDENT, TILED), (100, 70, RESIDENT, TILED),
                                              (128, 64, RESIDENT, TILED),
                                              (160, 136, TILED, TILED),           # 2 * 160 * 136 * 4 bytes > 160 KiB
                                              (6144, 1, TILED, TILED)])           # 6144 pairs, but 16 * Cin floats of staging
def test_thresholds(H, Cin, Cout, fwd, bwd):
    for B, Q in ((1, 1), (4, 16), (16, 144)):
        assert H.modemix_plan(B, Q, Cin, Cout)[:2] == (fwd, bwd), (B, Q)
    # the pick is the refusal of the resident launchers restated: LDS need <= 160 KiB, backward also Cin * Cout <= 6144
    lds_f = (2 * Cin * Cout + 16 * Cin) * 4
    lds_b = (2 * Cin * (Cout + 1) + 16 * Cin + 16 * Cout) * 4
    assert (fwd == RESIDENT) == (lds_f <= 160 * 1024)
    assert (bwd == RESIDENT) == (Cin * Cout <= 6144 and lds_b <= 160 * 1024)


def test_workspace_query_agrees_with_the_plan(H):
    seen = set()
    for B in (1, 3, 8, 9, 17, 64):
        for Q in (1, 2, 4, 16, 144):
            for Cin, Cout in ((8, 8), (32, 32), (96, 64), (96, 72), (96, 80), (128, 128), (160, 136), (6144, 1), (1, 6144)):
                _, bwd, slices = H.modemix_plan(B, Q, Cin, Cout)
                assert slices >= 1
                want = 0 if slices == 1 else slices * Cin * Cout * Q * 2 * 4
                assert H.lib().gt_modemix_bwd_ws_bytes(B, Q, Cin, Cout) == want, (B, Q, Cin, Cout)
                seen.add((bwd, slices > 1))
    assert seen == {(RESIDENT, False), (RESIDENT, True), (TILED, False), (TILED, True)}
    # a tiled grid that fills the chip on its own keeps the batch whole: no scratch
    assert H.modemix_plan(16, 144, 128, 128) == (RESIDENT if (2 * 128 * 128 + 16 * 128) * 4 <= 160 * 1024 else TILED, TILED, 1)
    assert H.lib().gt_modemix_bwd_ws_bytes(16, 144, 128, 128) == 0
    # a small one cuts it, at least 8 samples per slice
    assert H.modemix_plan(17, 2, 96, 72)[1:] == (TILED, 3)


def test_wide_fixtures_are_complete_small_and_tiled(H):
    """tests/golden/spectral_wide/: exactly the recorded files, each under 1 MiB; every fixture loads strictly into this
    package's module, and every one has a spectral layer that the resident backward refused."""
    import galerkin_transformer as gt
    from _spectral_wide_ref import SUB, WIDE_GOLDEN, WIDE_PARTS, wide_golden
    from test_modules_gpu import build_module
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, SUB)) if f.endswith(".npz"))
    assert files == sorted(n + ".npz" for n in WIDE_GOLDEN + WIDE_PARTS)
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, SUB, f)) < (1 << 20), f
    for name in WIDE_GOLDEN:
        g = wide_golden(name)
        mod = build_module(gt, g)
        res = mod.load_state_dict(g.sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert set(g.dparam) == set(dict(mod.named_parameters())) and set(g.din) == {"x"}
        B = g.inputs["x"].shape[0]
        routes = [H.modemix_plan(B, int(torch.tensor(p.shape[2:-1]).prod()), p.shape[0], p.shape[1])[:2]
                  for k, p in mod.named_parameters() if "fourier_weight" in k]
        assert routes and all(r[1] == TILED for r in routes), (name, routes)
        assert (name == "sconv1d_w160x136") == all(r[0] == TILED for r in routes), (name, routes)


def test_plan_rejects_empty_shapes(H):
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        with pytest.raises(H.GtError):
            H.modemix_plan(*bad)
