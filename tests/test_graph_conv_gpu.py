"""The graph feature extractor on the device (-m gpu): the three gt_graphconv_* kernels through the C ABI against float64
einsums, GraphConvolution / GCN and the two models that carry it against the fixtures recorded from the reference
(tests/golden/graph/), and the behaviour around them (one write of dE, graph capture, dropout seeds, nothing leaking).

Bars.  Kernels: KTOL = 2e-6 relative L2 (the kernel suites' bar).  Modules: TOL = 1e-5 for the output; d(x), d(edge) and every
parameter gradient max(TOL, 12 x the float32 restatement's own deviation from float64), the rule of
test_cross_attention_gpu._gate, computed in the test on the CPU -- never from the device run.  Deviations of the float32
restatement from float64 measured on the CPU (test_graph_conv_cpu.py::test_restatement_fp64_envelope), largest per fixture:
    g_gcn_l2 6.6e-07, g_gcn_l4_raw 7.6e-07, g_gcn_noact 5.8e-07 (all: edge_learner.lap_conv1.conv.0.weight),
    g_gcn_n70 1.4e-06 (edge_learner.lap_conv2.conv.0.weight), g_gconv_layer 1.8e-07 (weight),
    g_model1d_gcn 1.5e-06 (encoder_layers.1.attn.norm_K.0.weight),
    g_model2d_gcn 1.1e-06 (feat_extract.edge_learner.lap_conv1.conv.0.weight)."""
import pytest
import torch

from _graph_ref import GCN_GOLDEN, MODEL_GOLDEN, all_errors, extra, ref_grads
from _util import Golden, TOL, rel_l2
from test_softmax_attention_gpu import _run_fixture as run_plain_fixture

pytestmark = pytest.mark.gpu

KTOL = 2e-6
CANARY = 7.25
GUARD = 64
GROUPS = ((1,), (5, 3), (3, 5, 3), (32,))
EINVAL, ENOTSUP = -1, -4


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


# ------------------------------------------------------------------------------------------------- kernels
def _guarded(rows, ld, dev):
    """A [rows, ld] view in the middle of a buffer filled with the canary."""
    buf = torch.full((2 * GUARD + rows * ld,), CANARY, device=dev)
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)


def _padded(t, ld, dev):
    """t [rows, C] as the leading columns of a [rows, ld] device buffer whose pad columns hold the canary."""
    buf = torch.full((t.shape[0], ld), CANARY)
    buf[:, :t.shape[1]] = t
    return buf.to(dev)


def _check_canaries(buf, view, Cc):
    rows, ld = view.shape
    assert (buf[:GUARD] == CANARY).all() and (buf[GUARD + rows * ld:] == CANARY).all()
    assert (view[:, Cc:] == CANARY).all()


def _kernel_case(dev, B, n, groups, ld_pad, bias_on, relu, seed, offset=0):
    from galerkin_transformer import _hip
    Cc, T = sum(groups), B * n
    ld = Cc + ld_pad
    g = torch.Generator().manual_seed(seed)
    Es = [torch.randn(B, c, n, n, generator=g) for c in groups]
    if offset:          # group tensors off a 16-byte boundary
        holders = [torch.zeros(e.numel() + offset, device=dev) for e in Es]
        Ed = [h[offset:].view(e.shape).copy_(e.to(dev)) for h, e in zip(holders, Es)]
    else:
        Ed = [e.to(dev) for e in Es]
    E64 = torch.cat(Es, 1).double()
    S, G = torch.randn(T, Cc, generator=g), torch.randn(T, Cc, generator=g)
    bias = torch.randn(Cc, generator=g) if bias_on else None
    Sd, Gd = _padded(S, ld, dev), _padded(G, ld, dev)
    act = _hip.ACT_RELU if relu else _hip.ACT_NONE
    tag = (B, n, groups, ld_pad, bias_on, relu, offset)

    # forward
    y64 = torch.einsum("bcij,bjc->bic", E64, S.double().view(B, n, Cc))
    if bias_on:
        y64 = y64 + bias.double()
    if relu:
        y64 = y64.relu()
    outs = []
    for _ in range(2):
        buf, Y = _guarded(T, ld, dev)
        _hip.graphconv_fwd(Ed, Sd, None if bias is None else bias.to(dev), B, n, Cc, act, Y=Y, lds=ld, ldy=ld)
        _check_canaries(buf, Y, Cc)
        outs.append(Y[:, :Cc].clone())
    assert torch.equal(*outs), tag
    assert rel_l2(outs[0].view(B, n, Cc), y64) < KTOL, ("fwd", tag, rel_l2(outs[0].view(B, n, Cc), y64))

    # transposed product
    ds64 = torch.einsum("bcij,bic->bjc", E64, G.double().view(B, n, Cc))
    outs = []
    for _ in range(2):
        buf, dS = _guarded(T, ld, dev)
        _hip.graphconv_bwd_data(Ed, Gd, B, n, Cc, dS=dS, ldg=ld, ldds=ld)
        _check_canaries(buf, dS, Cc)
        outs.append(dS[:, :Cc].clone())
    assert torch.equal(*outs), tag
    assert rel_l2(outs[0].view(B, n, Cc), ds64) < KTOL, ("bwd_data", tag, rel_l2(outs[0].view(B, n, Cc), ds64))
    assert (Sd[:, Cc:] == CANARY).all() and (Gd[:, Cc:] == CANARY).all()
    return Es, Cc, ld, g


def _edge_case(dev, B, n, groups, ld_pad, P, skip_first, seed):
    from galerkin_transformer import _hip
    Cc, T = sum(groups), B * n
    ld = Cc + ld_pad
    g = torch.Generator().manual_seed(seed)
    Gs = [torch.randn(T, Cc, generator=g) for _ in range(P)]
    Ss = [torch.randn(T, Cc, generator=g) for _ in range(P)]
    de64 = sum(torch.einsum("bic,bjc->bcij", a.double().view(B, n, Cc), b.double().view(B, n, Cc)) for a, b in zip(Gs, Ss))
    Gd, Sd = [_padded(a, ld, dev) for a in Gs], [_padded(a, ld, dev) for a in Ss]
    tag = (B, n, groups, ld_pad, P, skip_first)
    runs = []
    for _ in range(2):
        bufs, des = [], []
        for gi, c in enumerate(groups):
            if skip_first and gi == 0:
                bufs.append(None)
                des.append((None, c))
                continue
            buf = torch.full((2 * GUARD + B * c * n * n,), CANARY, device=dev)
            bufs.append(buf)
            des.append(buf[GUARD:GUARD + B * c * n * n].view(B, c, n, n))
        _hip.graphconv_bwd_edge(des, Gd, Sd, B, n, Cc, ldg=ld, lds=ld)
        for buf in bufs:
            assert buf is None or ((buf[:GUARD] == CANARY).all() and (buf[-GUARD:] == CANARY).all()), tag
        runs.append([None if isinstance(d, tuple) else d.clone() for d in des])
    c0 = 0
    for gi, c in enumerate(groups):
        if runs[0][gi] is not None:
            assert torch.equal(runs[0][gi], runs[1][gi]), tag
            err = rel_l2(runs[0][gi], de64[:, c0:c0 + c])
            assert err < KTOL, ("bwd_edge", tag, gi, err)
        c0 += c


@pytest.mark.parametrize("n", [1, 5, 33, 34, 35, 64, 257])
def test_kernels_against_float64(GT, gpu_device, n):
    k = 0
    for B in (1, 2):
        for groups in GROUPS:
            # every switch takes both values under every (B, groups) pair's neighbours: ld_pad, bias and ReLU cycle with k
            ld_pad, bias_on, relu = (0, 3)[k & 1], bool((k >> 1) & 1), bool((k >> 2) & 1) ^ bool(k & 1)
            _kernel_case(gpu_device, B, n, groups, ld_pad, bias_on, relu, seed=1000 * n + k)
            _kernel_case(gpu_device, B, n, groups, 3 - ld_pad, not bias_on, not relu, seed=2000 * n + k)
            for P in (1, 2, 8):
                _edge_case(gpu_device, B, n, groups, ld_pad, P, skip_first=False, seed=3000 * n + 10 * k + P)
            if len(groups) > 1:
                _edge_case(gpu_device, B, n, groups, 3 - ld_pad, 2, skip_first=True, seed=4000 * n + k)
            k += 1
    torch.cuda.synchronize()


def test_kernels_past_one_sweep_and_off_alignment(GT, gpu_device):
    """n = 1030: four full 256-column sweeps and a rest, n % 4 = 2; and n = 64 with group tensors one float off a 16-byte
    boundary, which must take the dword path."""
    _kernel_case(gpu_device, 1, 1030, (5, 3), 3, True, True, seed=77)
    _edge_case(gpu_device, 1, 1030, (5, 3), 0, 2, skip_first=False, seed=78)
    _edge_case(gpu_device, 1, 1030, (5, 3), 3, 8, skip_first=True, seed=79)
    _kernel_case(gpu_device, 2, 64, (3, 5, 3), 0, True, False, seed=80, offset=1)
    _kernel_case(gpu_device, 1, 1028, (3,), 0, False, False, seed=81)          # the 16-byte path past one sweep
    torch.cuda.synchronize()


def test_kernels_refuse(GT, gpu_device):
    from galerkin_transformer import _hip
    lib, st, dev = _hip.lib(), _hip.stream_ptr(), gpu_device
    B, n, Cc = 1, 4, 8
    E = torch.zeros(B, Cc, n, n, device=dev)
    v = torch.zeros(B * n, Cc, device=dev)
    p = v.data_ptr()

    def groups(cs, ptrs=None):
        eg = _hip.GtEdgeGroups()
        eg.n_groups = len(cs) if ptrs is None else ptrs
        for i, c in enumerate(cs[:3]):
            eg.e[i], eg.c[i] = E.data_ptr(), c
        return eg

    def pairs(P):
        pr = _hip.GtGraphPairs()
        pr.n_pairs = P
        for i in range(min(P, _hip.GRAPHCONV_MAX_PAIRS)):
            pr.g[i], pr.s[i] = p, p
        return pr

    ok = groups((Cc,))
    assert lib.gt_graphconv_fwd(ok, p, Cc, None, p, Cc, B, n, Cc, 0, st) == 0
    assert lib.gt_graphconv_bwd_edge(ok, pairs(9), Cc, Cc, B, n, Cc, st) == ENOTSUP
    assert lib.gt_graphconv_bwd_edge(ok, pairs(0), Cc, Cc, B, n, Cc, st) == EINVAL
    for bad in (groups((Cc,), ptrs=0), groups((2, 2, 2), ptrs=4)):
        assert lib.gt_graphconv_fwd(bad, p, Cc, None, p, Cc, B, n, Cc, 0, st) == EINVAL
        assert lib.gt_graphconv_bwd_data(bad, p, Cc, p, Cc, B, n, Cc, st) == EINVAL
        assert lib.gt_graphconv_bwd_edge(bad, pairs(1), Cc, Cc, B, n, Cc, st) == EINVAL
    assert lib.gt_graphconv_fwd(groups((3, 4)), p, Cc, None, p, Cc, B, n, Cc, 0, st) == EINVAL       # sum c_g != C
    assert lib.gt_graphconv_fwd(ok, p, Cc - 1, None, p, Cc, B, n, Cc, 0, st) == EINVAL               # ld < C
    assert lib.gt_graphconv_fwd(ok, p, Cc, None, p, Cc - 1, B, n, Cc, 0, st) == EINVAL
    assert lib.gt_graphconv_bwd_data(ok, p, Cc - 1, p, Cc, B, n, Cc, st) == EINVAL
    assert lib.gt_graphconv_bwd_edge(ok, pairs(1), Cc, Cc - 1, B, n, Cc, st) == EINVAL
    assert lib.gt_graphconv_fwd(ok, p, Cc, None, p, Cc, B, 0, Cc, 0, st) == EINVAL                   # n = 0
    assert lib.gt_graphconv_bwd_data(ok, p, Cc, p, Cc, B, 0, Cc, st) == EINVAL
    assert lib.gt_graphconv_bwd_edge(ok, pairs(1), Cc, Cc, B, 0, Cc, st) == EINVAL
    assert lib.gt_graphconv_fwd(ok, p, Cc, None, p, Cc, B, n, Cc, _hip.ACT_SILU, st) == EINVAL
    # past the documented bound: refused from the arguments alone (these buffers are far too small for such an n)
    big = _hip.GRAPHCONV_MAX_N + 1
    assert lib.gt_graphconv_fwd(ok, p, Cc, None, p, Cc, B, big, Cc, 0, st) == ENOTSUP
    assert lib.gt_graphconv_bwd_data(ok, p, Cc, p, Cc, B, big, Cc, st) == ENOTSUP
    assert lib.gt_graphconv_bwd_edge(ok, pairs(1), Cc, Cc, B, big, Cc, st) == ENOTSUP
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- modules
def _no_dropout(mod):
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def _build(GT, g):
    m, kind = g.meta, g.meta["kind"]
    if kind == "gcn":
        return GT.GCN(node_feats=m["node_feats"], out_features=m["out_features"], num_gcn_layers=m["num_gcn_layers"],
                      edge_feats=m["edge_feats"], activation=m["activation"], raw_laplacian=m["raw_laplacian"])
    if kind == "graph_convolution":
        return GT.GraphConvolution(m["in_features"], m["out_features"])
    if kind == "simple_transformer_gcn":
        return GT.SimpleTransformer(**m["config"])
    return GT.FourierTransformer2D(**m["config"])


def _call(mod, g, ins):
    kind = g.meta["kind"]
    if kind in ("gcn", "graph_convolution"):
        return mod(ins["x"], ins["edge"])
    if kind == "simple_transformer_gcn":
        return mod(ins["node"], ins["edge"], ins["pos"])["preds"]
    return mod(ins["node"], ins["edge"], ins["pos"], ins["grid"])["preds"]


def _run(GT, dev, g, inputs=None, train_dropout=False, cot=None):
    torch.manual_seed(0)
    mod = _build(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = (mod if train_dropout else _no_dropout(mod)).to(dev).train()
    GT.set_attention_dropout("off")
    try:
        ins = {k: v.to(dev) for k, v in (inputs or g.inputs).items()}
        for k in g.din:
            ins[k].requires_grad_(True)
        out = _call(mod, g, ins)
        out.backward((g.cot if cot is None else cot).to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    return out.detach(), {k: ins[k].grad for k in g.din}, {k: p.grad for k, p in mod.named_parameters()}


def _gate(name, errs, noise):
    print(name, "worst", max(errs.values()), {k: (f"{v:.1e}", f"{noise.get(k, 0.0):.1e}") for k, v in errs.items()
                                              if v > 0.5 * TOL})
    bad = {k: (v, max(TOL, 12.0 * noise.get(k, 0.0))) for k, v in errs.items()
           if k != "out" and not v < max(TOL, 12.0 * noise.get(k, 0.0))}
    assert errs["out"] < TOL, errs["out"]
    assert not bad, bad


def _noise(g):
    o32, di32, dp32 = ref_grads(g, torch.float32)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    n = all_errors(o32, di32, dp32, o64, di64, dp64)
    n.pop("out")
    return n


@pytest.mark.parametrize("name", GCN_GOLDEN + MODEL_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("graph/" + name)
    out, din, grads = _run(GT, gpu_device, g)
    assert out.shape == g.out.shape
    for k in g.dparam:
        assert grads[k] is not None, k
    _gate(name, all_errors(out, din, grads, g.out, g.din, g.dparam), _noise(g))


def test_graph_convolution_both_layouts(GT, gpu_device):
    g = Golden("graph/g_gconv_layer")
    noise = _noise(g)
    out, din, grads = _run(GT, gpu_device, g)
    assert out.shape == g.out.shape == (2, 8, 34)
    _gate("g_gconv_layer [B, n, in]", all_errors(out, din, grads, g.out, g.din, g.dparam), noise)
    ins_t = dict(g.inputs, x=g.inputs["x"].transpose(1, 2).contiguous())
    out_t, din_t, grads_t = _run(GT, gpu_device, g, inputs=ins_t)
    ref_din = dict(x=extra("g_gconv_layer", "dx_t"), edge=extra("g_gconv_layer", "dedge_t"))
    assert din_t["x"].shape == (2, 5, 34)
    _gate("g_gconv_layer [B, in, n]", all_errors(out_t, din_t, grads_t, extra("g_gconv_layer", "out_t"), ref_din, g.dparam),
          noise)


@pytest.mark.parametrize("B,n,C", [(1, 33, 16), (2, 32, 32), (1, 32, 32)])
def test_batch_of_one_and_n_equal_to_c(GT, gpu_device, B, n, C):
    """The two shapes where the reference's GraphConvolution.forward goes wrong (GCN's docstring): the formula holds here."""
    L, F = 3, 3
    torch.manual_seed(100 * B + n)
    gcn = GT.GCN(node_feats=2, out_features=C, num_gcn_layers=L, edge_feats=F, raw_laplacian=True)
    with torch.no_grad():
        for p in gcn.parameters():
            p.add_(0.02 * torch.randn_like(p))
    g = Golden("graph/g_gcn_l2")
    g.meta = dict(kind="gcn", node_feats=2, out_features=C, num_gcn_layers=L, edge_feats=F, activation=True, raw_laplacian=True)
    g.sd = {k: v.detach().clone() for k, v in gcn.state_dict().items()}
    g.inputs = dict(x=torch.randn(B, n, 2), edge=torch.randn(B, n, n, F) / 4)
    g.cot = torch.randn(B, n, C)
    g.din, g.dparam = dict(x=None, edge=None), dict.fromkeys(g.sd)
    out, din, grads = _run(GT, gpu_device, g)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    assert out.shape == (B, n, C)
    _gate(f"gcn B {B} n {n} C {C}", all_errors(out, din, grads, o64, di64, dp64), _noise(g))


def test_stack_equals_chain_of_single_layers(GT, gpu_device):
    """GCN (channel groups, one write of dE) against a chain of single GraphConvolution modules over the concatenated edge
    tensor, ReLU where due: 1e-5 on the output and every gradient.  In a Profile of the stack's backward
    gt_graphconv_bwd_edge appears exactly once, and with an edge input that needs no gradient it writes the encoder's
    C - F channels only -- never the bytes of a [B, C, n, n] tensor."""
    from galerkin_transformer import _hip
    dev = gpu_device
    g = Golden("graph/g_gcn_l4_raw")
    m = g.meta
    B, n, Cc, L, F = m["B"], m["n"], m["out_features"], m["num_gcn_layers"], m["edge_feats"]
    out, din, grads = _run(GT, dev, g)

    gcn = _no_dropout(_build(GT, g))
    gcn.load_state_dict(g.sd)
    gcn = gcn.to(dev).train()
    x = g.inputs["x"].to(dev).requires_grad_(True)
    edge = g.inputs["edge"].to(dev).requires_grad_(True)
    E = gcn.edge_learner(edge.permute(0, 3, 1, 2).contiguous())
    assert E.shape == (B, Cc, n, n)
    h = x
    for l, layer in enumerate([gcn.gcn_layer0] + list(gcn.gcn_layers)):
        h = layer(h, E).permute(0, 2, 1)
        if 0 < l < L - 1:
            h = torch.relu(h)
    h.backward(g.cot.to(dev))
    torch.cuda.synchronize()
    chain = {k: p.grad for k, p in gcn.named_parameters()}
    errs = all_errors(out, din, grads, h.detach(), dict(x=x.grad, edge=edge.grad), chain)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL, errs

    for edge_grad in (True, False):
        for p in gcn.parameters():
            p.grad = None
        x2 = g.inputs["x"].to(dev).requires_grad_(True)
        e2 = g.inputs["edge"].to(dev).requires_grad_(edge_grad)
        y = gcn(x2, e2)
        with _hip.Profile() as prof:
            y.backward(g.cot.to(dev))
        torch.cuda.synchronize()
        recs = [r for r in prof.records if r[0] == "gt_graphconv_bwd_edge"]
        assert len(recs) == 1, [r[0] for r in prof.records]
        c_out = Cc if edge_grad else Cc - F
        assert recs[0][2] == 4.0 * B * (c_out * n * n + 2 * L * Cc * n)
        assert sum(r[0] == "gt_graphconv_bwd_data" for r in prof.records) == L
        cat_bytes, vec_bytes = 4.0 * B * Cc * n * n, 4.0 * B * 2 * L * Cc * n
        if not edge_grad:              # the edge part of the record: the encoder's channels, not a whole [B, C, n, n]
            assert recs[0][2] - vec_bytes == 4.0 * B * (Cc - F) * n * n < cat_bytes
            assert rel_l2(gcn.gcn_layer0.weight.grad, grads["gcn_layer0.weight"]) < TOL


def test_model_trains_a_step_and_captures(GT, gpu_device):
    """g_model1d_gcn's model, forward + WeightedL2Loss + backward: captured into one graph it replays bit-identically to
    eager, twice; the dataset's edge features need no gradient, the node features neither."""
    g = Golden("graph/g_model1d_gcn")
    dev = gpu_device
    torch.manual_seed(3)
    model = GT.SimpleTransformer(**g.meta["config"])
    model.load_state_dict(g.sd)
    model = _no_dropout(model).to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    node, edge, pos = (g.inputs[k].to(dev) for k in ("node", "edge", "pos"))
    N, n = node.shape[:2]
    gen = torch.Generator().manual_seed(11)
    u, up = torch.randn(N, n, generator=gen).to(dev), (torch.randn(N, n, generator=gen) * n).to(dev)
    lf = GT.WeightedL2Loss(regularizer=True, h=1 / n, gamma=0.5)

    def step():
        out = model(node, edge, pos)["preds"]
        loss, reg, _ = lf.terms(out[..., 0], u, targets_prime=up)
        return torch.autograd.grad(lf.reduce(loss) + lf.reduce(reg), params)

    GT.set_attention_dropout("off")
    try:
        eager = [t.clone() for t in step()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        replays = []
        for _ in range(2):
            graph.replay()
            replays.append([t.clone() for t in captured])
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    for e, r0, r1 in zip(eager, *replays):
        assert torch.isfinite(e).all()
        assert torch.equal(r0, r1) and torch.equal(e, r0)
    assert any(float(t.abs().max()) > 0 for t in eager)


def test_nothing_leaks_into_the_galerkin_path(GT, gpu_device):
    gal = Golden("enc_galerkin_c2")
    before = run_plain_fixture(GT, gpu_device, gal)
    _run(GT, gpu_device, Golden("graph/g_gcn_l4_raw"))
    _run(GT, gpu_device, Golden("graph/g_model1d_gcn"))
    after = run_plain_fixture(GT, gpu_device, gal)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
    for k, v in before[2].items():
        assert torch.equal(v, after[2][k]), k


def test_encoder_dropout_follows_the_seed(GT, gpu_device):
    """Training mode with the edge encoder's Dropout(0.1) left on: finite, the same bits under the same seed, other bits
    after advance_seed."""
    from galerkin_transformer import _hip
    g = Golden("graph/g_gcn_l2")

    def run(advance):
        _hip.set_seed(1234)
        if advance:
            _hip.advance_seed()
        return _run(GT, gpu_device, g, train_dropout=True)

    a, b, c = run(False), run(False), run(True)
    for t in [a[0]] + list(a[1].values()) + list(a[2].values()):
        assert torch.isfinite(t).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1]["edge"], b[1]["edge"])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert not torch.equal(a[0], c[0])
    assert rel_l2(a[0], Golden("graph/g_gcn_l2").out) > 1e-3          # the dropout did act
