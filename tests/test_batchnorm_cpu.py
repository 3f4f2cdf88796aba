"""batch_norm=True (BatchNorm1d in FeedForward), CPU side: the plain-torch restatement (tests/_batchnorm_ref.py) against the
fixtures recorded from the reference (tests/golden/batchnorm/), its float32-vs-float64 envelope, and the host-visible surface
of the feature (exported symbols, workspace query, checkpoint keys, refused BatchNorm1d options).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _batchnorm_ref import (BATCHNORM_CASES, BATCHNORM_GOLDEN, BUFFERS, SHARED_INPUTS, bn_prefixes, buffers_after,
                            grad_errors, ref_grads)
from _util import GOLDEN, Golden, rel_l2

# the bar test_oracle_golden.py holds the oracle to: fp32 round-off between two orderings of the same math -- 2e-6 for the
# output (and here the buffers), 5 x that for every gradient, exactly as there
REF_TOL = 2e-6
NEW_SYMBOLS = ("gt_batchnorm_ws_bytes", "gt_batchnorm_fwd", "gt_batchnorm_bwd")


def _errors(got, g, name):
    out, din, dparam, bufs = got
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(v, g.din[k]) for k, v in din.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dparam, g.dparam).items()})
    after = buffers_after(name) if g.meta["training"] else {k: v for k, v in g.sd.items() if k.rsplit(".", 1)[-1] in BUFFERS}
    assert sorted(after) == sorted(bufs) and len(after) == 3 * len(bn_prefixes(g.sd))
    for k, v in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v) == 3 + int(g.meta["training"]), k
        else:
            errs["buf:" + k] = rel_l2(bufs[k], v)
    return errs


@pytest.mark.parametrize("name", BATCHNORM_GOLDEN)
def test_restatement_matches_reference_golden(name):
    g = Golden("batchnorm/" + name)
    assert g.meta["training"] == (not name.endswith("_eval"))
    got = ref_grads(g, torch.float64)
    assert got[0].shape == g.out.shape and sorted(got[2]) == sorted(k for k, _ in _named_parameters(g))
    errs = _errors(got, g, name)
    print(name, {k: f"{v:.1e}" for k, v in errs.items() if v > REF_TOL})
    bad = {k: v for k, v in errs.items() if not v < (5 * REF_TOL if k[0] == "d" else REF_TOL)}
    assert not bad, bad


def _named_parameters(g):
    return [(k, v) for k, v in g.sd.items() if k.rsplit(".", 1)[-1] not in BUFFERS]


@pytest.mark.parametrize("name", BATCHNORM_GOLDEN)
def test_restatement_fp64_envelope(name):
    """float32 restatement vs the float64 one, per fixture and per tensor: the numerical envelope the HIP path is judged in
    (the figures the header of test_batchnorm_gpu.py quotes come from here)."""
    g = Golden("batchnorm/" + name)
    o32, di32, dp32, b32 = ref_grads(g, torch.float32)
    o64, di64, dp64, b64 = ref_grads(g, torch.float64)
    errs = {"out": rel_l2(o32, o64)}
    errs.update({"d" + k: rel_l2(v, di64[k]) for k, v in di32.items()})
    errs.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64).items()})
    errs.update({"buf:" + k: rel_l2(v, b64[k]) for k, v in b32.items() if v.is_floating_point()})
    worst = max(errs, key=errs.get)
    over = {k: f"{v:.1e}" for k, v in errs.items() if v > 1e-5 / 12}
    print(f"{name}: out {errs['out']:.2e}, worst {worst} {errs[worst]:.2e}, {len(over)} of {len(errs)} above 1e-5 / 12: {over}")
    assert errs["out"] < 1e-6, errs["out"]                 # the bar of test_oracle_fp64_envelope
    # gradients: a sanity ceiling of 1e3 x eps as in test_instance_norm_cpu.py, not a parity bar; the figures are printed
    assert errs[worst] < 6e-5, (worst, errs[worst])


def test_fixtures_hold_arrays_only():
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "batchnorm")) if f.endswith(".npz"))
    assert files == sorted(n + ".npz" for n in BATCHNORM_GOLDEN + SHARED_INPUTS)
    for f in files:
        path = os.path.join(GOLDEN, "batchnorm", f)
        assert os.path.getsize(path) < (1 << 20), f
        z = np.load(path, allow_pickle=False)
        for k in z.files:
            assert k == "meta" or k in ("out", "cot") or k.split("/")[0] in ("sd", "in", "din", "dparam", "buf1"), (f, k)
            assert z[k].dtype.kind in "fiub", (f, k, z[k].dtype)
        meta = json.loads(bytes(z["meta"]).decode())
        cfg = meta.get("config", meta)
        assert cfg.get("batch_norm", meta["kind"] == "feed_forward") is True
        keys = meta["state_dict_keys"]
        assert any(k.endswith("ff.bn." + b) or k == "bn." + b for k in keys for b in BUFFERS)
        if f.endswith("_in.npz"):
            assert [k[3:] for k in z.files if k.startswith("sd/")] == keys
            for k in keys:      # the buffers are away from nn.BatchNorm1d's initial (0, 1, 0)
                if k.endswith("running_mean"):
                    assert float(np.abs(z["sd/" + k]).min()) > 0
                if k.endswith("running_var"):
                    assert float(np.abs(z["sd/" + k] - 1).max()) > 0.1
                if k.endswith("num_batches_tracked"):
                    assert int(z["sd/" + k]) == 3


def test_new_symbols_declared_bound_and_exported():
    from galerkin_transformer import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gt_hip.h")).read()
    lib = ctypes.CDLL(_hip.lib_path())
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in _hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert _hip.lib().gt_abi_version() == 21 and _hip.ABI_VERSION == 21
    assert "#define GT_ABI_VERSION 21" in hdr


def test_workspace_query():
    """Host code: 0 for a width that is no multiple of 4, else one (mean, M2) pair of column groups per chunk, per group of
    64 chunks and once more; the chunks are 32 .. 128 rows long until there would be more than 4096 of them."""
    from galerkin_transformer import _hip
    q = _hip.lib().gt_batchnorm_ws_bytes
    assert q(150, 30) == 0 and q(150, 32) > 0
    assert q(0, 32) == 0 and q(150, 0) == 0 and q(150, -4) == 0
    pair = lambda f: 2 * (f // 4) * 16
    assert q(2, 32) == (1 + 1 + 1) * pair(32)
    T = 2 * 141 * 141
    nch = -(-T // 32)
    assert q(T, 256) == (nch + -(-nch // 64) + 1) * pair(256) and -(-nch // 64) > 1      # the second merge level is in use
    T = 128 * 141 * 141                                                                  # the bench's hidden matrix
    assert q(T, 256) == (-(-T // 1024) + -(-(-(-T // 1024)) // 64) + 1) * pair(256)
    assert 0 < q(1 << 33, 256) <= (4096 + 64 + 1) * pair(256)                            # bounded whatever T is


@pytest.mark.parametrize("case", BATCHNORM_CASES)
def test_module_keeps_the_reference_state_dict_keys(case):
    import galerkin_transformer as gt
    g = Golden("batchnorm/" + case)
    if g.meta["kind"] == "feed_forward":
        mod = gt.FeedForward(g.meta["in_dim"], g.meta["dim_feedforward"], batch_norm=True, activation=g.meta["activation"])
    elif g.meta["kind"] == "encoder_layer":
        kw = {k: v for k, v in g.meta.items() if k not in ("kind", "B", "n", "base", "state_dict_keys", "training")}
        mod = gt.SimpleTransformerEncoderLayer(dropout=0.0, ffn_dropout=0.0, **kw)
    else:
        mod = gt.SimpleTransformer(**g.meta["config"])
    assert list(mod.state_dict()) == g.meta["state_dict_keys"] == list(g.sd)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    norms = [m for m in mod.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(norms) == len(bn_prefixes(g.sd)) and all(int(m.num_batches_tracked) == 3 for m in norms)


def test_batch_norm_reaches_the_hip_operator():
    """No NotImplementedError any more: a CPU tensor gets as far as the operator's device check."""
    import galerkin_transformer as gt
    ff = gt.FeedForward(16, 32, batch_norm=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ff(torch.randn(2, 8, 16))
    layer = gt.SimpleTransformerEncoderLayer(d_model=64, n_head=4, pos_dim=2, attention_type="galerkin", layer_norm=False,
                                             batch_norm=True)
    assert isinstance(layer.ff.bn, torch.nn.BatchNorm1d)
    assert int(ff.bn.num_batches_tracked) == 0


@pytest.mark.parametrize("change", (dict(momentum=None), dict(affine=False), dict(track_running_stats=False)))
def test_refused_batchnorm_options_raise(change):
    import galerkin_transformer as gt
    ff = gt.FeedForward(16, 32, batch_norm=True)
    ff.bn = torch.nn.BatchNorm1d(32, **change)
    with pytest.raises(NotImplementedError, match="momentum, affine=True and track_running_stats=True"):
        ff(torch.randn(2, 8, 16))
    gelu = gt.FeedForward(16, 32, batch_norm=True, activation="gelu")
    with pytest.raises(NotImplementedError, match="gelu"):
        gelu(torch.randn(2, 8, 16))
