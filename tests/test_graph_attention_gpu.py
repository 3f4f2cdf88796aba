"""Graph attention on the device (-m gpu): the gt_graphattn_* kernels through the C ABI against float64, GraphAttention / GAT
and the 1-D model that carries it against the fixtures recorded from the reference (tests/golden/gat/), and the behaviour
around them (dropout replay, refusals, one mask pass per stack, no n x n float tensor, graph capture, nothing leaking).

Bars.  Kernels: KTOL = 2e-6 relative L2 for out, U, L, dU and dH.  ds, dt and da = [ds dt]^T h are cancelling sums
(sum_j P_ij (dP_ij - D_i) = 0): max(KTOL, 12 x the float32 CPU restatement's own deviation from float64), computed in the
test on the CPU -- never from the device run (the rule of test_cross_attention_gpu._gate).  s, t are standard normal, so
the signs of s_i + t_j mix in every row and ds does not vanish.  Modules: TOL = 1e-5 on the output, the 12 x noise rule on
every gradient."""
import math

import pytest
import torch

from _gat_ref import ALL_GOLDEN, all_errors, attention_core, keep_of, ref_grads, unpack_bits
from _util import Golden, TOL, rel_l2
from test_softmax_attention_gpu import _run_fixture as run_plain_fixture

pytestmark = pytest.mark.gpu

KTOL = 2e-6
CANARY = 7.25
GUARD = 64
EINVAL, ENOTSUP = -1, -4
ALPHA = 1e-2
THRESH = 1e-6


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


def _adj(B, n, g, graph_lap):
    """About eight kept entries per row, values at exactly +-thresh (not kept: the predicate is strict) and just beyond,
    negative entries (kept only with graph_lap); row 0 of sample 0 keeps nothing, row 1 exactly one entry."""
    dens = min(1.0, 8.0 / n)
    a = torch.randn(B, n, n, generator=g) * (torch.rand(B, n, n, generator=g) < dens)
    a[(a != 0) & (a.abs() < 1e-3)] = 0.5
    edge = torch.tensor([THRESH, -THRESH, 2 * THRESH, -2 * THRESH, 0.0], dtype=torch.float32)
    idx = torch.randint(0, n, (B, 5, 2), generator=g)
    for b in range(B):
        for k in range(5):
            a[b, idx[b, k, 0], idx[b, k, 1]] = edge[k]
    a[0, 0, :] = 0.0
    if n > 1:
        a[0, 1, :] = 0.0
        a[0, 1, n // 2] = 0.75
    if B > 1:
        a[1, 0, 0] = 1.0            # sample 1 is never all-empty
    return a.contiguous()


def _kernel_case(dev, B, n, Fd, ld_pad, graph_lap, concat, relu, seed, p=0.0):
    from galerkin_transformer import _hip
    T, ld = B * n, Fd + ld_pad
    g = torch.Generator().manual_seed(seed)
    adj = _adj(B, n, g, graph_lap)
    keep = keep_of(adj, graph_lap, THRESH)
    h, s, t = torch.randn(B, n, Fd, generator=g), torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    dout, a = torch.randn(B, n, Fd, generator=g), torch.randn(2 * Fd, generator=g)
    tag = (B, n, Fd, ld_pad, graph_lap, concat, relu, p)

    # the mask pass: bits, transposed bits, the weight of a masked entry
    if seed & 1:        # adj as channel 0 of an edge tensor [B, n, n, 3], read in place
        edge = torch.full((B, n, n, 3), CANARY)
        edge[..., 0] = adj
        bits, bitsT, w0 = _hip.graphattn_mask(edge.to(dev)[..., 0], graph_lap, THRESH)
    else:
        bits, bitsT, w0 = _hip.graphattn_mask(adj.to(dev), graph_lap, THRESH)
    assert torch.equal(unpack_bits(bits, n).cpu(), keep), tag
    assert torch.equal(unpack_bits(bitsT, n).cpu(), keep.transpose(1, 2)), tag
    W = _hip.graphattn_words(n)
    pad = torch.arange(64 * W, device=dev) >= n
    for words in (bits, bitsT):       # the bits past n are zero
        allbits = ((words[..., None] >> torch.arange(64, device=dev)) & 1).reshape(B, n, 64 * W)
        assert not allbits[:, :, pad].any(), tag
    w0_ref = torch.where(keep.any(-1), torch.zeros(B, n), torch.full((B, n), 1.0) / n)
    assert torch.equal(w0.cpu(), w0_ref), tag
    assert not keep[0, 0].any() and (n == 1 or int(keep[0, 1].sum()) == 1)

    st = torch.stack([s.reshape(T), t.reshape(T)], dim=1).contiguous().to(dev)          # (s, t) interleaved: ldst = 2
    hd, doutd, ad = _padded(h.reshape(T, Fd), ld, dev), _padded(dout.reshape(T, Fd), ld, dev), a.to(dev)
    drop = _hip.dropout_desc(p, 77, dev)

    def forward():
        ubuf, U = _guarded(T, ld, dev)
        obuf, out = _guarded(T, ld, dev)
        lbuf, Lg = _guarded(1, T, dev)
        _hip.graphattn_fwd(bits, w0, st, st[:, 1], 2, hd, U, out, Lg, B, n, Fd, ALPHA, concat, relu, drop, ldh=ld, ldo=ld)
        _check_canaries(ubuf, U, Fd)
        _check_canaries(obuf, out, Fd)
        _check_canaries(lbuf, Lg, T)
        return U, out, Lg

    def backward(U, Lg):
        dbuf, dU = _guarded(T, ld, dev)
        sbuf, dst = _guarded(T, 2, dev)
        pbuf, dtp = _guarded(B * W, n, dev)
        hbuf, dH = _guarded(T, ld, dev)
        _hip.graphattn_bwd_row(bits, st, st[:, 1], 2, Lg, doutd, U, hd, dU, dst, dtp, B, n, Fd, ALPHA, concat, relu, drop,
                               ldo=ld, ldh=ld, lddu=ld)
        _check_canaries(dbuf, dU, Fd)
        _check_canaries(pbuf, dtp, n)
        ds_only = dst[:, 0].clone()
        assert (dst[:, 1] == CANARY).all()          # bwd_row writes ds alone
        _hip.graphattn_bwd_col(bitsT, w0, st, st[:, 1], 2, Lg, dU, ad, dst, dtp, dst[:, 1], dH, B, n, Fd, ALPHA, drop,
                               lddu=ld, lddh=ld)
        _check_canaries(hbuf, dH, Fd)
        _check_canaries(sbuf, dst, 2)
        assert torch.equal(dst[:, 0], ds_only)
        return dU, dst, dH

    U, out, Lg = forward()
    U2, out2, Lg2 = forward()
    assert torch.equal(U, U2) and torch.equal(out, out2) and torch.equal(Lg, Lg2), tag
    dU, dst, dH = backward(U, Lg)
    dU2, dst2, dH2 = backward(U, Lg)
    assert torch.equal(dU, dU2) and torch.equal(dst, dst2) and torch.equal(dH, dH2), tag
    assert (hd[:, Fd:] == CANARY).all() and (doutd[:, Fd:] == CANARY).all()

    mask = None
    if p > 0:           # the kernels' own mask, through the only window onto it
        Pm = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, drop).cpu()
        P = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, None).cpu()
        assert ((Pm == 0) | ((Pm - P / (1 - p)).abs() <= 1e-6 * P)).all(), tag
        mask = torch.where(Pm > 0, 1.0 / (1.0 - p), 0.0)

    def reference(dtype):
        hh, ss, tt = (v.to(dtype).clone().requires_grad_(True) for v in (h, s, t))
        o, Uu, LL, _ = attention_core(hh, ss, tt, keep, alpha=ALPHA, concat=concat, relu=relu,
                                      mask=None if mask is None else mask.to(dtype))
        gU, = torch.autograd.grad(o, Uu, dout.to(dtype), retain_graph=True)
        gh, gs, gt = torch.autograd.grad(o, [hh, ss, tt], dout.to(dtype))
        aa = a.to(dtype)
        dHr = gh + gs[..., None] * aa[:Fd] + gt[..., None] * aa[Fd:]
        da = torch.stack([gs.reshape(T), gt.reshape(T)], 0) @ hh.detach().reshape(T, Fd)
        return dict(out=o.detach(), U=Uu.detach(), L=LL.detach(), dU=gU, dH=dHr, ds=gs, dt=gt, da=da)

    def cancelled_terms(r):
        """The size of what cancels in ds_i = sum_j P_ij (m_ij dPm_ij - D_i): A_ij = keep_ij P_ij (|m_ij dPm_ij| + |D_i|) summed
        like ds, dt and da.  Where the exact value is identically zero -- every row keeps at most one entry (n = 1), or all its
        kept entries sit on one side of the LeakyReLU, so that sum_j P_ij (dP_ij - D_i) = 0 leaves with one common slope (a
        few rows at n = 5) -- a relative error has no denominator, and a float32 evaluation is off by rounding times THIS
        size: the bar there is KTOL times it, on the absolute error."""
        h64 = h.double()
        P = attention_core(h64, s.double(), t.double(), keep, alpha=ALPHA, concat=concat, relu=relu)[3]
        dPm = r["dU"] @ h64.transpose(1, 2)
        if mask is not None:
            dPm = dPm * mask.double()
        A = keep * P * (dPm.abs() + (r["dU"] * r["U"]).sum(-1, keepdim=True).abs())
        rows, cols = A.sum(-1), A.sum(-2)
        return dict(ds=float(rows.norm()), dt=float(cols.norm()),
                    da=float((torch.stack([rows.reshape(T), cols.reshape(T)], 0) @ h64.abs().reshape(T, Fd)).norm()))

    r64, r32 = reference(torch.float64), reference(torch.float32)
    dst_c = dst.cpu()
    got = dict(out=out[:, :Fd].reshape(B, n, Fd), U=U[:, :Fd].reshape(B, n, Fd), L=Lg.reshape(B, n),
               dU=dU[:, :Fd].reshape(B, n, Fd), dH=dH[:, :Fd].reshape(B, n, Fd), ds=dst_c[:, 0].reshape(B, n),
               dt=dst_c[:, 1].reshape(B, n), da=dst_c.double().t() @ h.double().reshape(T, Fd))
    errs, bad = {}, {}
    for k, v in got.items():
        errs[k] = rel_l2(v, r64[k])
        bar = KTOL if k not in ("ds", "dt", "da") else max(KTOL, 12.0 * rel_l2(r32[k], r64[k]))
        if k in ("ds", "dt", "da") and float(r64[k].norm()) <= 1e-9 * cancelled_terms(r64)[k]:
            # identically zero (float64 leaves its own rounding, 1e-16 of the terms): the absolute error against the terms
            errs[k] = float((v.double().cpu() - r64[k]).norm())
            bar = max(KTOL * cancelled_terms(r64)[k], 1e-300)
        if not errs[k] < bar:
            bad[k] = (errs[k], bar)
    print(tag, {k: f"{v:.1e}" for k, v in errs.items()})
    assert not bad, (tag, bad)
    # the literal -9e15: a row that keeps nothing has uniform weights and sends nothing into s; masked entries nothing into t
    assert float(dst_c[0, 0]) == 0.0 and abs(float(Lg.reshape(B, n)[0, 0]) - math.log(n)) < 1e-6


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 64, 65, 257])
def test_kernels_against_float64(GT, gpu_device, n):
    k = 0
    for B in (1, 2):
        for Fd in (4, 8, 36, 96, 132):
            ld_pad, graph_lap, concat, relu = (0, 3)[k & 1], bool((k >> 1) & 1), bool((k >> 2) & 1) ^ bool(k & 1), bool(k % 3 == 0)
            _kernel_case(gpu_device, B, n, Fd, ld_pad, graph_lap, concat, relu, seed=1000 * n + k)
            _kernel_case(gpu_device, B, n, Fd, 3 - ld_pad, not graph_lap, not concat, not relu, seed=2000 * n + k)
            k += 1
    torch.cuda.synchronize()


def test_kernels_past_one_sweep_and_widest(GT, gpu_device):
    """n = 1030: seventeen 64-column chunks, n % 4 = 2; F = 256: the bwd_row tile that needs more than 64 KiB of LDS."""
    _kernel_case(gpu_device, 1, 1030, 36, 3, True, True, False, seed=77)
    _kernel_case(gpu_device, 1, 65, 256, 0, True, True, True, seed=78)
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_and_replay(GT, gpu_device, p):
    from galerkin_transformer import _hip
    dev = gpu_device
    B, n = 2, 70                                        # dense adj: B n n = 9800 kept-eligible entries
    g = torch.Generator().manual_seed(int(100 * p))
    st = torch.randn(B * n, 2, generator=g).to(dev)
    bits, bitsT, w0 = _hip.graphattn_mask(torch.ones(B, n, n, device=dev), True, THRESH)
    Lg = torch.empty(B, n, device=dev)
    hd = torch.randn(B * n, 4, generator=g).to(dev)
    _hip.set_seed(4321)
    drop = _hip.dropout_desc(p, 5, dev)
    _hip.graphattn_fwd(bits, w0, st, st[:, 1], 2, hd, None, torch.empty_like(hd), Lg, B, n, 4, ALPHA, True, False, drop)
    P = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, None)
    assert (P > 0).all() and rel_l2(P.sum(-1), torch.ones(B, n)) < KTOL
    Pm = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, drop)
    assert ((Pm == 0) | ((Pm - P / (1 - p)).abs() <= 1e-6 * P)).all()          # every entry is 0 or P / (1 - p)
    N = B * n * n
    assert N >= 8192
    frac = float((Pm > 0).sum()) / N
    assert abs(frac - (1 - p)) < 5.0 * math.sqrt(p * (1 - p) / N), (frac, p)
    kept = Pm > 0                                       # no row and no column is dropped wholesale
    assert kept.any(-1).all() and kept.any(-2).all()
    again = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, drop)
    assert torch.equal(Pm, again)                        # the same seed: the same bits
    _hip.advance_seed()
    moved = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, drop)
    assert not torch.equal(Pm > 0, moved > 0)
    other = _hip.graphattn_weights(bits, w0, st, st[:, 1], 2, Lg, B, n, ALPHA, _hip.dropout_desc(p, 6, dev))
    assert not torch.equal(moved > 0, other > 0)         # another salt: another mask
    _hip.set_seed(4321)
    # forward and all gradients with the kernels' mask replayed into the float64 reference: sparse adj, several tiles
    _kernel_case(dev, 2, 65, 36, 3, True, True, False, seed=int(1000 * p), p=p)
    _kernel_case(dev, 1, 130, 96, 0, False, False, True, seed=int(1000 * p) + 1, p=p)
    torch.cuda.synchronize()


def test_kernels_refuse(GT, gpu_device):
    from galerkin_transformer import _hip
    lib, st, dev = _hip.lib(), _hip.stream_ptr(), gpu_device
    B, n, Fd = 1, 4, 8
    v = torch.zeros(64, device=dev)           # deliberately tiny: nothing may be launched on a refusal
    p = v.data_ptr()

    def fwd(B=B, n=n, Fd=Fd, ldst=1, ldh=Fd, ldo=Fd, alpha=ALPHA):
        return lib.gt_graphattn_fwd(p, p, p, p, ldst, p, ldh, p, p, ldo, p, B, n, Fd, alpha, 1, 0, None, st)

    def row(B=B, n=n, Fd=Fd, ldo=Fd, ldh=Fd, lddu=Fd):
        return lib.gt_graphattn_bwd_row(p, p, p, 1, p, p, p, ldo, p, ldh, p, lddu, p, p, B, n, Fd, ALPHA, 1, 0, None, st)

    def col(B=B, n=n, Fd=Fd, lddu=Fd, lddh=Fd):
        return lib.gt_graphattn_bwd_col(p, p, p, p, 1, p, p, lddu, p, p, p, p, p, lddh, B, n, Fd, ALPHA, None, st)

    def mask(B=B, n=n):
        return lib.gt_graphattn_mask(p, 1, p, p, p, B, n, 1, THRESH, st)

    def weights(B=B, n=n):
        return lib.gt_graphattn_weights(p, p, p, p, 1, p, p, B, n, ALPHA, None, st)

    big = _hip.GRAPHATTN_MAX_N + 1
    with _hip.Profile() as prof:
        for f in (fwd, row, col):
            assert f(Fd=6) == ENOTSUP and f(Fd=260) == ENOTSUP and f(n=0) == EINVAL and f(B=0) == EINVAL
            assert f(n=big) == ENOTSUP
        assert fwd(ldh=Fd - 1) == EINVAL and fwd(ldo=Fd - 1) == EINVAL and fwd(ldst=0) == EINVAL
        assert fwd(alpha=-0.5) == ENOTSUP
        assert row(ldo=Fd - 1) == EINVAL and row(ldh=Fd - 1) == EINVAL and row(lddu=Fd - 1) == EINVAL
        assert col(lddu=Fd - 1) == EINVAL and col(lddh=Fd - 1) == EINVAL
        for f in (mask, weights):
            assert f(n=0) == EINVAL and f(n=big) == ENOTSUP
        assert lib.gt_graphattn_mask(None, 1, p, p, p, B, n, 1, THRESH, st) == EINVAL
        assert lib.gt_graphattn_mask(p, 0, p, p, p, B, n, 1, THRESH, st) == EINVAL
        bad = _hip.GtDropout()
        bad.p, bad.salt, bad.seed = 1.0, 1, _hip.seed_state(dev).data_ptr()
        assert lib.gt_graphattn_fwd(p, p, p, p, 1, p, Fd, p, p, Fd, p, B, n, Fd, ALPHA, 1, 0, bad, st) == EINVAL
        # through the binding: an exception, and no Profile record
        adj = torch.eye(n, device=dev)[None].contiguous()
        bits, bitsT, w0 = _hip.graphattn_mask(adj, True, THRESH)
        n_ok = len(prof.records)
        assert n_ok == 1
        h6, st6, L6 = torch.zeros(n, 6, device=dev), torch.zeros(n, 2, device=dev), torch.zeros(1, n, device=dev)
        with pytest.raises(NotImplementedError):
            _hip.graphattn_fwd(bits, w0, st6, st6[:, 1], 2, h6, None, torch.empty_like(h6), L6, 1, n, 6, ALPHA, True, False)
        h8 = torch.zeros(n, 8, device=dev)
        with pytest.raises(_hip.GtError):
            _hip.graphattn_fwd(bits, w0, st6, st6[:, 1], 2, h8, None, torch.empty_like(h8), L6, 1, n, 8, ALPHA, True, False,
                               ldh=7)
        assert len(prof.records) == n_ok, [r[0] for r in prof.records]
    torch.cuda.synchronize()
    assert (v == 0).all()


# ------------------------------------------------------------------------------------------------- modules
def _quiet(mod, GT):
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, GT.GraphAttention):
            m.dropout = 0.0
    return mod


def _build(GT, g):
    m, kind = g.meta, g.meta["kind"]
    if kind == "graph_attention":
        return GT.GraphAttention(m["in_features"], m["out_features"], alpha=m["alpha"], concat=m["concat"],
                                 graph_lap=m["graph_lap"], interaction_thresh=m["thresh"])
    if kind == "gat":
        return GT.GAT(node_feats=m["node_feats"], out_features=m["out_features"], num_gcn_layers=m["num_gcn_layers"],
                      activation=m["activation"])
    cfg = m["config"]         # the config switch is not wired (test_graph_conv_cpu.py::test_refusals): by assignment
    model = GT.SimpleTransformer(**dict(cfg, feat_extract_type=None, num_feat_layers=0))
    model.feat_extract = GT.GAT(node_feats=cfg["node_feats"], out_features=cfg["n_hidden"],
                                num_gcn_layers=cfg["num_feat_layers"], activation=cfg["graph_activation"])
    return model


def _call(mod, g, ins):
    kind = g.meta["kind"]
    if kind == "graph_attention":
        return mod(ins["node"], ins["adj"])
    if kind == "gat":
        return mod(ins["x"], ins["edge"])
    return mod(ins["node"], ins["edge"], ins["pos"])["preds"]


def _run(GT, dev, g, quiet=True):
    torch.manual_seed(0)
    mod = _build(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = (_quiet(mod, GT) if quiet else mod).to(dev).train()
    GT.set_attention_dropout("off")
    try:
        ins = {k: v.to(dev) for k, v in g.inputs.items()}
        for k in g.din:
            ins[k].requires_grad_(True)
        out = _call(mod, g, ins)
        out.backward(g.cot.to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    for k in ("adj", "edge"):
        assert k not in ins or ins[k].grad is None
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


@pytest.mark.parametrize("name", ALL_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name):
    g = Golden("gat/" + name)
    out, din, grads = _run(GT, gpu_device, g)
    assert out.shape == g.out.shape
    for k in g.dparam:
        assert grads[k] is not None, k
    _gate(name, all_errors(out, din, grads, g.out, g.din, g.dparam), _noise(g))


def _synthetic(GT, B, n, Fd, L, activation, seed):
    """A GAT with perturbed parameters as a fixture-shaped object, its references from the float64 restatement."""
    torch.manual_seed(seed)
    gat = GT.GAT(node_feats=2, out_features=Fd, num_gcn_layers=L, activation=activation)
    with torch.no_grad():
        for p in gat.parameters():
            p.add_(0.02 * torch.randn_like(p))
    g = Golden("gat/a_gat_l2")
    g.meta = dict(kind="gat", node_feats=2, out_features=Fd, num_gcn_layers=L, activation=activation)
    g.sd = {k: v.detach().clone() for k, v in gat.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    adj = _adj(B, n, gen, True)
    adj[:, torch.arange(n), torch.arange(n)] = 2.0
    edge = torch.randn(B, n, n, 2, generator=gen)
    edge[..., 0] = adj
    g.inputs = dict(x=torch.randn(B, n, 2, generator=gen), edge=edge)
    g.cot = torch.randn(B, n, Fd, generator=gen)
    g.din, g.dparam = dict(x=None), dict.fromkeys(g.sd)
    return g


@pytest.mark.parametrize("B,n,Fd", [(1, 33, 16), (2, 32, 32), (1, 32, 32)])
def test_batch_of_one_and_n_equal_to_f(GT, gpu_device, B, n, Fd):
    g = _synthetic(GT, B, n, Fd, 3, True, 100 * B + n)
    out, din, grads = _run(GT, gpu_device, g)
    o64, di64, dp64 = ref_grads(g, torch.float64)
    assert out.shape == (B, n, Fd)
    _gate(f"gat B {B} n {n} F {Fd}", all_errors(out, din, grads, o64, di64, dp64), _noise(g))


def test_stack_equals_chain_and_packs_the_mask_once(GT, gpu_device):
    """GAT (one operator over L = 4 layers) against a chain of single GraphAttention modules with the ReLUs where due, and
    the launches of the stack's forward + backward: one mask pass, L forward, L bwd_row, L bwd_col."""
    from galerkin_transformer import _hip
    dev = gpu_device
    g = Golden("gat/a_gat_l4_act")
    L = g.meta["num_gcn_layers"]
    out, din, grads = _run(GT, dev, g)

    gat = _quiet(_build(GT, g), GT)
    gat.load_state_dict(g.sd)
    gat = gat.to(dev).train()
    x = g.inputs["x"].to(dev).requires_grad_(True)
    edge = g.inputs["edge"].to(dev)
    adj = edge[..., 0].contiguous()
    hcur = x
    for l, layer in enumerate([gat.gat_layer0] + list(gat.gat_layers)):
        hcur = layer(hcur, adj)
        if 0 < l < L - 1:
            hcur = torch.relu(hcur)
    hcur.backward(g.cot.to(dev))
    torch.cuda.synchronize()
    chain = {k: p.grad for k, p in gat.named_parameters()}
    errs = all_errors(out, din, grads, hcur.detach(), dict(x=x.grad), chain)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL, errs

    for prm in gat.parameters():
        prm.grad = None
    x2 = g.inputs["x"].to(dev).requires_grad_(True)
    with _hip.Profile() as prof:
        gat(x2, edge).backward(g.cot.to(dev))
    torch.cuda.synchronize()
    names = [r[0] for r in prof.records]
    assert names.count("gt_graphattn_mask") == 1, names
    for sym in ("gt_graphattn_fwd", "gt_graphattn_bwd_row", "gt_graphattn_bwd_col"):
        assert names.count(sym) == L, (sym, names)
    assert "gt_graphattn_weights" not in names
    # eval mode / no_grad: nothing dropped, nothing saved -- the same output as the quiet training run
    noisy = _build(GT, g)
    noisy.load_state_dict(g.sd)
    noisy = noisy.to(dev).eval()
    assert noisy.gat_layer0.dropout == 0.1
    with torch.no_grad():
        y = noisy(g.inputs["x"].to(dev), edge)
    assert torch.equal(y, out)


def test_no_n_by_n_float_tensor(GT, gpu_device):
    """B 2, n 1024, F 32, L 2, forward + backward: the allocator's peak rises by less than ONE [B, n, n] float tensor.  The two
    bit masks are 1/16 of that bound, the saved and transient [B, n, F] tensors about a quarter."""
    dev = gpu_device
    B, n, Fd, L = 2, 1024, 32, 2
    g = _synthetic(GT, B, n, Fd, L, False, 7)
    gat = _build(GT, g)
    gat.load_state_dict(g.sd)
    gat = gat.to(dev).train()           # dropout 0.1 on: the mask is regenerated, never stored
    x = g.inputs["x"].to(dev).requires_grad_(True)
    edge, cot = g.inputs["edge"].to(dev), g.cot.to(dev)

    def step():
        for p in gat.parameters():
            p.grad = None
        x.grad = None
        gat(x, edge).backward(cot)

    step()                               # scratch buffers, the seed state, lazily built handles
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise} B against {4 * B * n * n} B")
    assert rise < 4 * B * n * n, rise
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


def test_training_step_captures(GT, gpu_device):
    """A GAT training step with its dropout ON, captured into one graph: it replays bit-identically to eager, twice (the seed
    is device-resident and the salts are rewound to the eager step's)."""
    from galerkin_transformer import _hip
    dev = gpu_device
    g = Golden("gat/a_gat_l4_act")
    gat = _build(GT, g)
    gat.load_state_dict(g.sd)
    gat = gat.to(dev).train()
    params = list(gat.parameters())
    x, edge, cot = g.inputs["x"].to(dev), g.inputs["edge"].to(dev), g.cot.to(dev)

    def step():
        return torch.autograd.grad((gat(x, edge) * cot).sum(), params)

    _hip.set_seed(99)
    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    _hip.set_seed(99)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append([t.clone() for t in captured])
    torch.cuda.synchronize()
    for e, r0, r1 in zip(eager, *replays):
        assert torch.isfinite(e).all()
        assert torch.equal(r0, r1) and torch.equal(e, r0)
    assert any(float(t.abs().max()) > 0 for t in eager)
    assert rel_l2(eager[0], _quiet_grad(GT, dev, g, cot)) > 1e-3          # the dropout did act


def _quiet_grad(GT, dev, g, cot):
    gat = _quiet(_build(GT, g), GT)
    gat.load_state_dict(g.sd)
    gat = gat.to(dev).train()
    out = gat(g.inputs["x"].to(dev), g.inputs["edge"].to(dev))
    return torch.autograd.grad((out * cot).sum(), list(gat.parameters()))[0]


def test_nothing_leaks_into_the_galerkin_path(GT, gpu_device):
    gal = Golden("enc_galerkin_c2")
    before = run_plain_fixture(GT, gpu_device, gal)
    _run(GT, gpu_device, Golden("gat/a_gat_l4_act"), quiet=False)
    _run(GT, gpu_device, Golden("gat/a_model1d_gat"))
    after = run_plain_fixture(GT, gpu_device, gal)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x"], after[1]["x"])
    for k, v in before[2].items():
        assert torch.equal(v, after[2][k]), k
