"""CPU tests of the random-feature attention baselines ('rfa' / 'favor'): ABI surface, state-dict compatibility with the
reference's example, the refusals, the float64 restatement tests/_rfa_ref.py against the fixtures of tests/golden/rfa/, and
a lane model of one wave of gt_rfattn_kv (tools/mfma_sim.py)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from _rfa_ref import FIXTURES, RfaGolden, kva
from _util import all_golden, rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mfma_sim as S  # noqa: E402

NEW_SYMBOLS = ("gt_rfattn_slabs", "gt_rfattn_ws_bytes", "gt_rfattn_kv", "gt_rfattn_q", "gt_rfattn_bwd_q", "gt_rfattn_bwd_kv")


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
    assert _hip.RFATTN_D == (32, 64, 96)
    # the queries answer from the arguments alone
    assert _hip.rfattn_slabs(1) == 1 and _hip.rfattn_slabs(10 ** 6) > 1
    n2 = next(n for n in range(1, 10 ** 4) if _hip.rfattn_slabs(n) == 2)
    assert _hip.lib().gt_rfattn_ws_bytes(2, n2 - 1, 96) == 0
    assert _hip.lib().gt_rfattn_ws_bytes(2, n2, 96) == 2 * 2 * 96 * 100 * 4
    assert _hip.lib().gt_rfattn_ws_bytes(2, n2, 80) == 0


def test_fixtures_live_in_their_subfolder():
    assert not [f for f in all_golden() if "rfa" in f or "favor" in f]
    for name in FIXTURES:
        g = RfaGolden(name)
        assert g.meta["min_den_over_mean"] >= 0.1 and set(g.noise) >= {"out"} | set(g.dparam)


def _build(g):
    import galerkin_transformer as gt
    m, what = g.meta, g.meta["what"]
    if what == "attn":
        return gt.RandomFourierAttention(m["d_model"], 1, pos_dim=m["pos_dim"], eps=m["eps"], attention_type=g.kind)
    if what == "layer":
        return gt.RandomFeatureEncoderLayer(d_model=m["d_model"], n_head=1, dim_feedforward=m["dim_feedforward"],
                                            attention_type=g.kind, dropout=0.0, ffn_dropout=0.0)
    return gt.RandomFeatureTransformer(**m["config"])


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_is_the_reference_examples(name):
    g = RfaGolden(name)
    mod = _build(g)
    sd = mod.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in g.sd.items()}
    mod.load_state_dict(g.sd, strict=True)
    assert {k for k, _ in mod.named_parameters()} == set(g.dparam)
    omegas = [k for k in sd if k.endswith("feature_map.omega")]
    assert len(omegas) == (g.meta["config"]["num_encoder_layers"] if g.meta["what"] == "model" else 1)
    for k in omegas:
        assert k not in dict(mod.named_parameters()) and torch.equal(mod.state_dict()[k], g.sd[k])


def test_refusals():
    import galerkin_transformer as gt
    from galerkin_transformer import ops
    made = []
    orig = torch.nn.Linear.__init__

    def spy(self, *a, **k):
        made.append(a)
        return orig(self, *a, **k)
    torch.nn.Linear.__init__ = spy
    try:
        with pytest.raises(ValueError, match="one head"):
            gt.RandomFourierAttention(64, 2)
        with pytest.raises(ValueError, match="one head"):
            gt.RandomFeatureEncoderLayer(d_model=96)          # the example's default n_head = 2 never ran either
        with pytest.raises(NotImplementedError, match="d=80"):
            gt.RandomFourierAttention(80, 1)
        with pytest.raises(ValueError, match="'rfa' or 'favor'"):
            gt.RandomFourierAttention(64, 1, attention_type="cosine")
    finally:
        torch.nn.Linear.__init__ = orig
    assert not made                                            # refused before any parameter was created
    mod = gt.RandomFourierAttention(32, 1)
    x = torch.randn(2, 5, 32)
    with pytest.raises(ValueError, match="pos"):
        mod(x, x, x, pos=None)
    with pytest.raises(NotImplementedError, match="one tensor"):
        mod(x, x.clone(), x, pos=torch.rand(2, 5, 1))
    w = lambda *s: torch.zeros(*s)
    with pytest.raises(NotImplementedError, match="d=80"):      # before anything is allocated or launched: CPU tensors
        ops.random_feature_attention(w(2, 5, 80), w(2, 5, 1), w(240, 80), w(240), w(80, 40), w(80, 81), w(80), kind="rfa")
    with pytest.raises(ValueError, match="pos"):
        ops.random_feature_attention(w(2, 5, 32), None, w(96, 32), w(96), w(32, 16), w(32, 33), w(32), kind="rfa")
    # a supported shape on CPU tensors reaches the operator, which has no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback") as ei:
        mod(x, x, x, pos=torch.rand(2, 5, 1))
    assert not isinstance(ei.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gt.RandomFeatureTransformer(**RfaGolden("model_rfa").meta["config"])(torch.randn(2, 16, 1), None, torch.rand(2, 16, 1))


def test_feature_map_modules():
    import galerkin_transformer as gt
    torch.manual_seed(0)
    for cls, kind, orth in ((gt.RandomFourierFeatures, "rfa", False), (gt.Favor, "favor", True)):
        fm = cls(32, n_dims=32)
        assert fm.kind == kind and fm.orthogonal is orth and tuple(fm.omega.shape) == (32, 16) and fm.redraw
        assert "omega" in dict(fm.named_buffers()) and not list(fm.parameters())
        fm.new_feature_map(torch.device("cpu"))
        om = fm.omega.clone()
        assert float(om.abs().max()) > 0
        fm.redraw = False
        fm.new_feature_map(torch.device("cpu"))
        assert torch.equal(fm.omega, om)
        fm.redraw, fm.deterministic_eval = True, True
        fm.eval().new_feature_map(torch.device("cpu"))
        assert torch.equal(fm.omega, om)
        fm.train().new_feature_map(torch.device("cpu"))
        assert not torch.equal(fm.omega, om)
        if orth:
            gram = fm.omega.t().double() @ fm.omega.double()
            assert float((gram - torch.diag(torch.diag(gram))).abs().max()) < 1e-5 * float(torch.diag(gram).max())
        # the torch definition of phi is the restatement's
        from _rfa_ref import phi
        z = torch.randn(3, 7, 32, dtype=torch.float64)
        fm.double()
        assert rel_l2(fm(z), phi(z, fm.omega, kind)) < 1e-14


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_reference(name):
    g = RfaGolden(name)
    out, dx, dparam = g.restated(torch.float64)
    xname = "node" if g.meta["what"] == "model" else "x"
    errs = {"out": rel_l2(out, g.out), "d" + xname: rel_l2(dx, g.din[xname])}
    errs.update({k: rel_l2(v, g.dparam[k]) for k, v in dparam.items()})
    assert set(dparam) == set(g.dparam)
    print(name, max(errs.values()))
    assert max(errs.values()) < 1e-12, {k: v for k, v in errs.items() if v >= 1e-12}


# ------------------------------------------------------------------------------------------------- lane model
def _wave_kv(K, V, omega, n, tok0, kind):
    """One wave of gt_rfattn_kv on its 16-token tile, lane by lane as the kernel indexes it (d = 32: KS = 2 float4 groups of
    z per lane, NU = 1 tile of u, NF = 2 feature tiles, 2 dim tiles).  Returns the wave's slab contribution [32][36]."""
    d, HF, KS, NU, NF = 32, 16, 2, 1, 2
    j, kq = S.X, S.KQ
    sc = d ** -0.25
    rowj = np.minimum(tok0 + j, n - 1)
    xs = np.zeros((KS, 4, 64))
    for s in range(KS):
        for c in range(4):
            xs[s, c] = sc * K[rowj, 16 * s + 4 * kq + c]
    cj = (xs ** 2).sum((0, 1))
    cj = cj + cj[(S.LANES ^ 16)] + (cj + cj[(S.LANES ^ 16)])[(S.LANES ^ 32)]      # the two xor shuffles
    cj = 0.5 * cj + 0.5 * math.log(d)
    c4 = np.stack([cj[4 * kq + r] for r in range(4)], 1)                             # __shfl(cj, 4 kq + r)
    u = np.zeros((64, 4))
    for s in range(KS):
        for c in range(4):
            u = S.mfma(xs[s, c], omega[16 * s + 4 * kq + c, j], u)                   # N tile: A = z, B = Om
    live = (tok0 + 4 * kq[:, None] + np.arange(4)[None, :]) < n
    if kind == "favor":
        lo, hi = np.exp(u - c4), np.exp(-u - c4)
    else:
        lo, hi = math.sqrt(2 / d) * np.cos(u), math.sqrt(2 / d) * np.sin(u)
    pn = [np.where(live, lo, 0.0), np.where(live, hi, 0.0)]                          # feature tiles 0 (first half), 1
    slab = np.zeros((d, d + 4))
    for f in range(NF):
        ks = np.zeros(64)
        for dt in range(2):
            acc = np.zeros((64, 4))
            for r in range(4):
                row4 = np.minimum(tok0 + 4 * kq + r, n - 1)
                acc = S.mfma(V[row4, 16 * dt + j], pn[f][:, r], acc)                 # A = V^T, B = phi: the hand-over
            for lane in range(64):
                slab[16 * f + j[lane], 16 * dt + 4 * kq[lane]:16 * dt + 4 * kq[lane] + 4] = acc[lane]
        for r in range(4):
            ks += pn[f][:, r]
        ks = ks + ks[S.LANES ^ 16]
        ks = ks + ks[S.LANES ^ 32]
        slab[16 * f + j[kq == 0], d] = ks[kq == 0]
    return slab


@pytest.mark.parametrize("kind", ["rfa", "favor"])
def test_lane_model_of_kv_wave(kind):
    """d = 32, n = 70: the wave that owns tokens 64..79 (second tile, partial) and the one that owns 0..15 -- the index maps
    of the phi hand-over between the two products and the exclusion of rows >= n, against plain numpy."""
    rng = np.random.default_rng(7)
    d, n = 32, 70
    K, V, omega = 0.5 * rng.standard_normal((n, d)), rng.standard_normal((n, d)), rng.standard_normal((d, d // 2))
    t = lambda a: torch.from_numpy(a)[None]
    for tok0 in (0, 64):
        rows = slice(tok0, min(tok0 + 16, n))
        want = kva(t(K[rows]), t(V[rows]), torch.from_numpy(omega), kind)[0].numpy()
        got = _wave_kv(K, V, omega, n, tok0, kind)
        assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
        assert (got[:, d + 1:] == 0).all()
