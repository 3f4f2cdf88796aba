"""The graph feature extractor without a device: the plain-torch restatement (_graph_ref) against the fixtures recorded from
the reference (tests/golden/graph/), the module tree and initialisation of GCN, the edge features of BurgersDataset, and the
refusals that need no kernel."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from _graph_ref import GRAPH_GOLDEN, all_errors, burgers_edge, extra, init_hashes, ref_grads
from _util import Golden, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTOL = 2e-6            # the oracle suite's bar for a float32 restatement against the float32 reference


@pytest.fixture(scope="module")
def GT():
    import galerkin_transformer as gt
    return gt


@pytest.mark.parametrize("name", GRAPH_GOLDEN)
def test_restatement_matches_reference(name):
    g = Golden("graph/" + name)
    out, din, dparam = ref_grads(g, torch.float32)
    assert out.shape == g.out.shape
    assert set(g.din) >= {"edge"} and set(g.dparam) == set(g.sd)
    errs = all_errors(out, din, dparam, g.out, g.din, g.dparam)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < OTOL, errs


def test_restatement_takes_both_layouts_of_one_layer():
    g = Golden("graph/g_gconv_layer")
    assert rel_l2(extra("g_gconv_layer", "out_t"), g.out) < OTOL
    assert rel_l2(extra("g_gconv_layer", "dx_t").transpose(1, 2), g.din["x"]) < OTOL
    assert rel_l2(extra("g_gconv_layer", "dedge_t"), g.din["edge"]) < OTOL


@pytest.mark.parametrize("name", GRAPH_GOLDEN)
def test_restatement_fp64_envelope(name):
    """How far the float32 restatement sits from the float64 one, per tensor: the noise the device gates may add to TOL."""
    g = Golden("graph/" + name)
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    errs = all_errors(o32, di32, dp32, o64, di64, dp64)
    worst = max(errs, key=errs.get)
    print(f"{name}: worst {worst} {errs[worst]:.1e}", {k: f"{v:.1e}" for k, v in errs.items() if v > 5e-7})
    assert errs[worst] < 2e-6, errs


def _gcn_hashes(mod):
    return {k: hashlib.sha256(v.detach().numpy().tobytes()).hexdigest() for k, v in mod.state_dict().items()}


def test_gcn_state_dict_and_init(GT):
    inv = init_hashes()
    torch.manual_seed(inv["seed"])
    gcn = GT.GCN(*inv["args"])
    assert {k: list(v.shape) for k, v in gcn.state_dict().items()} == {k: v["shape"] for k, v in inv["params"].items()}
    assert list(gcn.state_dict()) == list(inv["params"])
    assert _gcn_hashes(gcn) == {k: v["sha256"] for k, v in inv["params"].items()}
    assert isinstance(gcn.relu, torch.nn.ReLU) and isinstance(gcn.dropout, torch.nn.Dropout) and gcn.dropout.p == 0.1
    assert repr(gcn.gcn_layer0) == "GraphConvolution (1 -> 32)"
    raw = GT.GCN(node_feats=2, out_features=16, num_gcn_layers=4, edge_feats=3, raw_laplacian=True)
    shapes = {k: tuple(v.shape) for k, v in raw.state_dict().items()}
    assert shapes["edge_learner.lap_conv1.conv.0.weight"] == (8, 3, 3, 3)           # D = 13: c0 = int(13 / 3 * 2) = 8
    assert shapes["edge_learner.lap_conv2.conv.0.weight"] == (5, 8, 3, 3)
    assert shapes["gcn_layer0.weight"] == (2, 16) and shapes["gcn_layers.2.bias"] == (16,)
    with pytest.raises(AssertionError):
        GT.EdgeEncoder(4, 4)


@pytest.mark.parametrize("name", ["g_gcn_l2", "g_gcn_l4_raw", "g_gcn_noact", "g_gcn_n70"])
def test_gcn_loads_reference_state_dict(GT, name):
    g = Golden("graph/" + name)
    m = g.meta
    gcn = GT.GCN(node_feats=m["node_feats"], out_features=m["out_features"], num_gcn_layers=m["num_gcn_layers"],
                 edge_feats=m["edge_feats"], activation=m["activation"], raw_laplacian=m["raw_laplacian"])
    res = gcn.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_models_build_the_extractor(GT):
    inv = init_hashes()
    for name, cls in (("g_model1d_gcn", GT.SimpleTransformer), ("g_model2d_gcn", GT.FourierTransformer2D)):
        g = Golden("graph/" + name)
        model = cls(**g.meta["config"])
        assert isinstance(model.feat_extract, GT.GCN)
        res = model.load_state_dict(g.sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert [k for k in model.state_dict() if k.startswith("feat_extract.")] == \
            ["feat_extract." + k for k in inv["params"]]
    # the extractor is the first thing SimpleTransformer draws: the same seed gives the GCN's own parameters
    cfg = dict(Golden("graph/g_model1d_gcn").meta["config"], node_feats=1, n_hidden=32, num_feat_layers=2, edge_feats=6)
    torch.manual_seed(inv["seed"])
    model = GT.SimpleTransformer(**cfg)
    assert _gcn_hashes(model.feat_extract) == {k: v["sha256"] for k, v in inv["params"].items()}
    # without the switch nothing changes
    plain = GT.SimpleTransformer(**dict(cfg, feat_extract_type=None, num_feat_layers=0))
    assert isinstance(plain.feat_extract, GT.Identity)
    plain2d = GT.FourierTransformer2D(**dict(Golden("graph/g_model2d_gcn").meta["config"], num_feat_layers=0))
    assert isinstance(plain2d.feat_extract, GT.Identity) and not list(plain2d.feat_extract.parameters())


def test_refusals(GT):
    with pytest.raises(ValueError, match="num_gcn_layers >= 2"):
        GT.GCN(1, 32, 1, 6)
    cfg = Golden("graph/g_model1d_gcn").meta["config"]
    for cls in (GT.SimpleTransformer, GT.FourierTransformer2D):
        with pytest.raises(NotImplementedError, match="GCN"):
            cls(**dict(Golden("graph/g_model2d_gcn").meta["config"] if cls is GT.FourierTransformer2D else cfg,
                       feat_extract_type="gat"))
    from galerkin_transformer import ops
    B, n, C = 1, 4, 4
    x, e = torch.zeros(B, n, C), torch.zeros(B, C, n, n)
    with pytest.raises(NotImplementedError, match="9 layers"):
        ops.graph_conv_stack(x, e, [torch.zeros(C, C)] * 9, [None] * 9, [False] * 9)
    with pytest.raises(RuntimeError, match="no CPU fallback") as ei:
        ops.graph_conv_stack(x, e, [torch.zeros(C, C)] * 2, [torch.zeros(C)] * 2, [False] * 2)
    assert not isinstance(ei.value, NotImplementedError)
    gcn = GT.GCN(1, 8, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcn(torch.zeros(1, 5, 1), torch.zeros(1, 5, 5, 2))


def test_symbols_declared_and_exported():
    from galerkin_transformer import _hip
    with open(os.path.join(ROOT, "include", "gt_hip.h")) as f:
        header = f.read()
    syms = [s for s in _hip.EXPORTED_SYMBOLS if s.startswith("gt_graphconv")]
    assert sorted(syms) == ["gt_graphconv_bwd_data", "gt_graphconv_bwd_edge", "gt_graphconv_fwd"]
    for s in syms:
        assert re.search(r"\bint " + s + r"\(", header), s
    assert sorted(set(re.findall(r"\b(gt_graphconv\w*)\(", header))) == sorted(syms)
    assert f"#define GT_GRAPHCONV_MAX_N     {_hip.GRAPHCONV_MAX_N}" in header and _hip.GRAPHCONV_MAX_N >= 8192
    assert f"#define GT_GRAPHCONV_MAX_PAIRS {_hip.GRAPHCONV_MAX_PAIRS}" in header
    assert _hip.ABI_VERSION == 21


def test_burgers_edge_features(GT):
    meta, ref = burgers_edge()
    n = meta["n_grid"]
    for tag, kw in meta["variants"].items():
        ds = GT.BurgersDataset(subsample=4, n_grid_fine=4 * n, synthetic=True, n_samples_synthetic=4, return_edge=True, **kw)
        item = ds[1]
        edge, mass = item["edge"], item["mass"]
        assert edge.dtype == torch.float32 and mass.dtype == torch.float32
        assert tuple(edge.shape) == ref[tag + "/edge"].shape and tuple(mass.shape) == (n, n)
        assert edge.shape[-1] == ds.n_krylov + 2 * ds.return_distance_features + ds.return_mass_features
        assert rel_l2(edge, torch.from_numpy(ref[tag + "/edge"])) < 1e-6, tag
        for c in range(edge.shape[-1]):
            assert rel_l2(edge[..., c], torch.from_numpy(ref[tag + "/edge"][..., c])) < 1e-6, (tag, c)
        assert rel_l2(mass, torch.from_numpy(ref[tag + "/mass"].reshape(n, n))) < 1e-6, tag
        assert torch.equal(ds[0]["edge"], edge)
    with pytest.raises(NotImplementedError):
        GT.BurgersDataset(subsample=4, n_grid_fine=4 * n, synthetic=True, n_samples_synthetic=4, return_edge=True,
                          smoother="gs")
    plain = GT.BurgersDataset(subsample=4, n_grid_fine=4 * n, synthetic=True, n_samples_synthetic=4)[0]
    assert torch.equal(plain["edge"], torch.tensor([1.0])) and torch.equal(plain["mass"], torch.tensor([1.0]))
    # distance features off: the Krylov channels alone, whatever return_mass_features says (as in the reference)
    ds = GT.BurgersDataset(subsample=4, n_grid_fine=4 * n, synthetic=True, n_samples_synthetic=4, return_edge=True,
                           return_distance_features=False, return_mass_features=True, n_krylov=1)
    assert tuple(ds[0]["edge"].shape) == (n, n, 1)
    np.testing.assert_allclose(ds[0]["edge"][..., 0].numpy(), ref["default/edge"][..., 0], rtol=0, atol=1e-6)
