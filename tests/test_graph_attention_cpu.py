"""The graph-attention feature extractor without a device: the plain-torch restatement (_gat_ref) against the fixtures
recorded from the reference (tests/golden/gat/), the module tree and initialisation of GraphAttention / GAT, and the refusals
that need no kernel."""
import hashlib
import os
import re

import pytest
import torch

from _gat_ref import ALL_GOLDEN, GAT_GOLDEN, all_errors, fixture_keep, init_hashes, ref_grads
from _util import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTOL = 2e-6            # the oracle suite's bar for a float32 restatement against the float32 reference


@pytest.fixture(scope="module")
def GT():
    import galerkin_transformer as gt
    return gt


@pytest.mark.parametrize("name", ALL_GOLDEN)
def test_restatement_matches_reference(name):
    g = Golden("gat/" + name)
    out, din, dparam = ref_grads(g, torch.float32)
    assert out.shape == g.out.shape
    assert set(g.dparam) == set(g.sd) and "adj" not in g.din and "edge" not in g.din      # adj.grad is None in the reference
    errs = all_errors(out, din, dparam, g.out, g.din, g.dparam)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < OTOL, errs


@pytest.mark.parametrize("name", ALL_GOLDEN)
def test_restatement_fp64_envelope(name):
    """How far the float32 restatement sits from the float64 one, per tensor: the noise the device gates may add to TOL."""
    g = Golden("gat/" + name)
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    errs = all_errors(o32, di32, dp32, o64, di64, dp64)
    worst = max(errs, key=errs.get)
    print(f"{name}: worst {worst} {errs[worst]:.1e}", {k: f"{v:.1e}" for k, v in errs.items()})
    assert errs[worst] < 2e-6, errs


def test_fixtures_hold_the_edge_cases():
    keep = fixture_keep(Golden("gat/a_layer"))
    assert int((~keep.any(-1)).sum()) == 1 and not keep[1, 7].any()             # one row keeps nothing
    g = Golden("gat/a_gat_l2")
    adj = g.inputs["edge"][..., 0]
    assert float(adj[0, 4, 20]) == pytest.approx(5e-7) and not fixture_keep(g)[0, 4, 20]
    g = Golden("gat/a_layer_noconcat")
    assert not g.meta["concat"] and not g.meta["graph_lap"] and bool((g.inputs["adj"] < 0).any())
    for name in ALL_GOLDEN:                                                       # no value a rounding could flip
        g = Golden("gat/" + name)
        a = (g.inputs["adj"] if "adj" in g.inputs else g.inputs["edge"][..., 0]).abs()
        odd = (a > 0) & (a < 1e-3)
        assert int(odd.sum()) == (1 if name == "a_gat_l2" else 0), name


def test_empty_row_is_uniform():
    from _gat_ref import attention_core
    B, n, Fd = 1, 33, 4
    gen = torch.Generator().manual_seed(3)
    h, s, t = torch.randn(B, n, Fd, generator=gen), torch.randn(B, n, generator=gen), torch.randn(B, n, generator=gen)
    keep = torch.eye(n, dtype=torch.bool)[None].clone()
    keep[0, 5] = False
    _, _, L, Pm = attention_core(h, s, t, keep)
    assert torch.allclose(Pm[0, 5], torch.full((n,), 1.0 / n)) and float(Pm[0, 5, 0]) == pytest.approx(0.0303, abs=1e-4)
    assert float(L[0, 5]) == pytest.approx(float(torch.log(torch.tensor(33.0))))


def _hashes(mod):
    return {k: hashlib.sha256(v.detach().numpy().tobytes()).hexdigest() for k, v in mod.state_dict().items()}


def test_gat_state_dict_and_init(GT):
    inv = init_hashes()
    torch.manual_seed(inv["seed"])
    gat = GT.GAT(*inv["args"])
    assert list(gat.state_dict()) == list(inv["params"]) == ["gat_layer0.W", "gat_layer0.a", "gat_layers.0.W", "gat_layers.0.a"]
    assert {k: list(v.shape) for k, v in gat.state_dict().items()} == {k: v["shape"] for k, v in inv["params"].items()}
    assert _hashes(gat) == {k: v["sha256"] for k, v in inv["params"].items()}
    assert repr(gat.gat_layer0) == "GraphAttention (1 -> 32)" and repr(gat.gat_layers[0]) == "GraphAttention (32 -> 32)"
    layer = gat.gat_layer0
    assert isinstance(layer.leakyrelu, torch.nn.LeakyReLU) and layer.leakyrelu.negative_slope == 1e-2
    assert isinstance(layer.dropout, float) and layer.dropout == 0.1 and list(layer.state_dict()) == ["W", "a"]
    assert isinstance(gat.relu, torch.nn.ReLU) and gat.activation is False
    import libs
    assert libs.GAT is GT.GAT and libs.GraphAttention is GT.GraphAttention


@pytest.mark.parametrize("name", GAT_GOLDEN)
def test_gat_loads_reference_state_dict(GT, name):
    g = Golden("gat/" + name)
    m = g.meta
    gat = GT.GAT(node_feats=m["node_feats"], out_features=m["out_features"], num_gcn_layers=m["num_gcn_layers"],
                 activation=m["activation"])
    res = gat.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_model_takes_the_extractor_by_assignment(GT):
    g = Golden("gat/a_model1d_gat")
    cfg = dict(g.meta["config"], feat_extract_type=None, num_feat_layers=0)
    model = GT.SimpleTransformer(**cfg)
    model.feat_extract = GT.GAT(node_feats=cfg["node_feats"], out_features=cfg["n_hidden"], num_gcn_layers=2,
                                activation=cfg["graph_activation"])
    res = model.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_refusals(GT):
    with pytest.raises(ValueError, match="num_gcn_layers >= 2"):
        GT.GAT(1, 32, 1)
    from galerkin_transformer import ops
    B, n, Fd = 1, 5, 8
    x, adj = torch.zeros(B, n, 3), torch.eye(n)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback") as ei:
        ops.graph_attention_stack(x, adj, [torch.zeros(3, Fd)], [torch.zeros(2 * Fd, 1)], [False])
    assert not isinstance(ei.value, NotImplementedError)
    with pytest.raises(NotImplementedError, match="F = 6"):
        ops.graph_attention_stack(x, adj, [torch.zeros(3, 6)], [torch.zeros(12, 1)], [False])
    with pytest.raises(NotImplementedError, match="F = 260"):
        ops.graph_attention_stack(x, adj, [torch.zeros(3, 260)], [torch.zeros(520, 1)], [False])
    with pytest.raises(ValueError):
        ops.graph_attention_stack(x, adj, [torch.zeros(3, Fd)], [torch.zeros(Fd, 1)], [False])
    layer = GT.GraphAttention(3, Fd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(x, adj)
    gat = GT.GAT(3, Fd, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gat(x, torch.zeros(B, n, n, 2))


def test_symbols_declared_and_exported():
    from galerkin_transformer import _hip
    with open(os.path.join(ROOT, "include", "gt_hip.h")) as f:
        header = f.read()
    syms = sorted(s for s in _hip.EXPORTED_SYMBOLS if s.startswith("gt_graphattn"))
    assert syms == ["gt_graphattn_bwd_col", "gt_graphattn_bwd_row", "gt_graphattn_fwd", "gt_graphattn_mask",
                    "gt_graphattn_weights"]
    for s in syms:
        assert re.search(r"\bint " + s + r"\(", header), s
    assert sorted(set(re.findall(r"\b(gt_graphattn\w*)\(", header))) == syms
    assert f"#define GT_GRAPHATTN_MAX_N {_hip.GRAPHATTN_MAX_N}" in header and _hip.GRAPHATTN_MAX_N >= 8192
    assert f"#define GT_GRAPHATTN_MAX_F {_hip.GRAPHATTN_MAX_F}" in header
    assert _hip.ABI_VERSION == 21
