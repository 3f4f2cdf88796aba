"""batch_norm=True (BatchNorm1d in FeedForward) on the device (-m gpu): the gt_batchnorm_* kernels through the C ABI against
float64, the operator and the modules against the fixtures recorded from the reference (tests/golden/batchnorm/), the hidden
dropout in front of the norm, and the behaviour around them (buffers, graph capture, batch_norm=False untouched, refusals).

Bars.  Kernels: KTOL = 2e-6 relative L2 against float64 (the bar of the token-norm kernels, test_instance_norm_gpu.py); the
mean is measured in units of the column's standard deviation, which is how it enters z.  Offset column (|mean| / std = 1e3):
4 x the error of float32 torch.nn.functional.batch_norm on the same data against float64, measured in the test.  Operator
and modules: TOL = 1e-5 relative L2 for the output, dx and every parameter gradient, except where the float32 restatement
itself sits further than TOL / 12 from the float64 one: there max(TOL, 12 x that deviation), computed in the test from the
CPU restatement -- never from the device run.  Buffers after a step: KTOL; num_batches_tracked exactly.  Deviations of the
float32 restatement from float64 measured on the CPU (test_batchnorm_cpu.py::test_restatement_fp64_envelope), largest per
fixture:
    ff_bn_relu 4.3e-07 (lr1.bias), _eval 3.6e-07, ff_bn_silu 9.8e-07 (lr1.bias: bound 1.2e-05), _eval 3.2e-07,
    enc_galerkin_bn_c2 6.6e-07, _eval 6.4e-07, model_burgers_bn_small 6.4e-06 (encoder_layers.1.ff.lr1.bias; 42 of its 62 tensors lie above
    TOL / 12 = 8.3e-07 and get a bound above TOL, the largest 7.7e-05), _eval 1.3e-06 (encoder_layers.1.attn.norm_K.0.bias;
    8 of 62 above TOL / 12, the largest bound 1.6e-05).
Everywhere else the 1e-5 bar binds."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from _batchnorm_ref import (BATCHNORM_GOLDEN, BUFFERS, bn_prefixes, buffers_after, feed_forward_bn, grad_errors, ref_grads)
from _util import Golden, TOL, rel_l2
from test_modules_gpu import build_module, run_module

pytestmark = pytest.mark.gpu

KTOL = 2e-6
WIDTHS = (32, 96, 192, 256, 384, 1200)
# f = 1200 is 300 column groups: a single row lane (RL = 1) and two column blocks, the second with 44 live lanes of 256; the
# other widths have one column block and RL >= 2.  It is about the columns, so it runs at one row count.
WIDE, WIDE_ROWS = 1200, (150,)
# no multiple of a chunk length (32 .. 128 rows); 2 * 141^2 rows make 1243 chunks, i.e. 20 groups for the second merge level
ROWS = (33, 150, 1849, 2 * 141 * 141)
MODES = (None, "f32", "bf16")          # None: the default arithmetic


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


@contextlib.contextmanager
def precision(mode):
    from galerkin_transformer import _hip
    old = _hip.set_precision(mode) if mode is not None else None
    try:
        yield
    finally:
        if old is not None:
            _hip.set_precision(old)


def _data(T, f, dev, seed, offset=None):
    """hid [T, f]: per-column scale in [0.5, 2] and offset ~ N(0, 1) (or the given one); dz, gamma, beta, running buffers."""
    g = torch.Generator().manual_seed(seed)
    off = torch.randn(f, generator=g) if offset is None else torch.full((f,), float(offset))
    x = torch.randn(T, f, generator=g) * (0.5 + 1.5 * torch.rand(f, generator=g)) + off
    dz = torch.randn(T, f, generator=g)
    gamma, beta = 1.0 + 0.5 * torch.randn(f, generator=g), torch.randn(f, generator=g)
    rm, rv = 0.3 * torch.randn(f, generator=g), 0.5 + torch.rand(f, generator=g)
    return tuple(t.to(dev) for t in (x, dz, gamma, beta, rm, rv))


def _ref64(x, dz, gamma, beta, rm, rv, eps, momentum, training):
    """float64 torch: dict(z, d, dgamma, dbeta, mean, rstd, bvar, rm, rv) -- d is the gradient w.r.t. x in front of any gate."""
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    T = x.shape[0]
    if training:
        mean = x64.mean(dim=0)
        var = ((x64 - mean) ** 2).mean(dim=0)
        new = ((1 - momentum) * rm.double() + momentum * mean.detach(),
               (1 - momentum) * rv.double() + momentum * var.detach() * T / max(T - 1, 1))
    else:
        mean, var, new = rm.double(), rv.double(), (rm.double(), rv.double())
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (x64 - mean) * rstd * g64 + b64
    d, dg, db = torch.autograd.grad(z, [x64, g64, b64], dz.double())
    return dict(z=z.detach(), d=d, dgamma=dg, dbeta=db, mean=mean.detach(), rstd=rstd.detach(), bvar=var.detach(),
                rm=new[0], rv=new[1])


def _dsilu64(pre):
    p = pre.double()
    s = torch.sigmoid(p)
    return s * (1 + p * (1 - s))


def _kernel_errors(_hip, x, dz, gamma, beta, rm, rv, eps, momentum, training, seed):
    """One forward and the backward under each of the three gates against float64: {quantity: error}."""
    dev, (T, f) = x.device, x.shape
    r = _ref64(x, dz, gamma, beta, rm, rv, eps, momentum, training)
    rm1, rv1 = rm.clone(), rv.clone()
    z, stats, bvar = _hip.batchnorm_fwd(x, gamma, beta, eps, rm1, rv1, momentum, training)
    errs = dict(z=rel_l2(z, r["z"]), rstd=rel_l2(stats[:, 1], r["rstd"]), bvar=rel_l2(bvar, r["bvar"]),
                # the mean in units of the column's standard deviation (an error relative to itself would measure the
                # data's cancellation where a column's mean happens to be small)
                mean=float(((stats[:, 0].double() - r["mean"]) * r["rstd"]).norm() / f ** 0.5),
                running_mean=rel_l2(rm1, r["rm"]), running_var=rel_l2(rv1, r["rv"]))
    if not training:
        assert torch.equal(rm1, rm) and torch.equal(rv1, rv) and torch.equal(bvar, rv) and torch.equal(stats[:, 0], rm)
    p_h = 0.25
    pre = torch.randn(T, f, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    drop = _hip.dropout_desc(p_h, 77 + seed, dev)
    mask = _hip.dropout_apply(torch.ones(T, f, device=dev), drop)          # 0 or 1 / (1 - p_h), indexed by the flat element
    assert 0.2 < float((mask == 0).float().mean()) < 0.3 and float(mask.max()) == pytest.approx(1 / (1 - p_h))
    gates = {"none": ((_hip.AUX_NONE, None, 1.0, None), r["d"]),
             "gt0": ((_hip.AUX_GT0, None, 1.0 / (1.0 - p_h), None), r["d"] * (x > 0).double() / (1.0 - p_h)),
             "dsilu": ((_hip.AUX_DSILU, pre, 1.0, drop), r["d"] * _dsilu64(pre) * mask.double()),
             "dsilu_nodrop": ((_hip.AUX_DSILU, pre, 1.0, None), r["d"] * _dsilu64(pre))}
    for name, (gate, want) in gates.items():
        gh, dg, db = _hip.batchnorm_bwd(x, dz, gamma, stats, training, gate=gate)
        assert torch.isfinite(gh).all()
        errs["gh_" + name] = rel_l2(gh, want)
        errs["dgamma_" + name], errs["dbeta_" + name] = rel_l2(dg, r["dgamma"]), rel_l2(db, r["dbeta"])
        # in place (dX == dZ): the same bits; a second run: the same bits
        gi = dz.clone()
        ghi, dgi, dbi = _hip.batchnorm_bwd(x, gi, gamma, stats, training, gate=gate, out=gi)
        assert ghi is gi and torch.equal(ghi, gh) and torch.equal(dgi, dg) and torch.equal(dbi, db), name
        gh2, dg2, db2 = _hip.batchnorm_bwd(x, dz, gamma, stats, training, gate=gate)
        assert torch.equal(gh2, gh) and torch.equal(dg2, dg) and torch.equal(db2, db), name
    # forward once more: the same bits (buffers included); in place (Z == X): the same bits
    rm2, rv2 = rm.clone(), rv.clone()
    z2, stats2, bvar2 = _hip.batchnorm_fwd(x, gamma, beta, eps, rm2, rv2, momentum, training)
    assert torch.equal(z2, z) and torch.equal(stats2, stats) and torch.equal(bvar2, bvar)
    assert torch.equal(rm2, rm1) and torch.equal(rv2, rv1)
    xi, rm3, rv3 = x.clone(), rm.clone(), rv.clone()
    zi, si, bi = _hip.batchnorm_fwd(xi, gamma, beta, eps, rm3, rv3, momentum, training, out=xi)
    assert zi is xi and torch.equal(zi, z) and torch.equal(si, stats) and torch.equal(bi, bvar) and torch.equal(rm3, rm1)
    if training:          # the buffers after three calls on the same data
        for _ in range(2):
            _hip.batchnorm_fwd(x, gamma, beta, eps, rm1, rv1, momentum, True)
        m3, v3 = rm.double(), rv.double()
        for _ in range(3):
            m3 = (1 - momentum) * m3 + momentum * r["mean"]
            v3 = (1 - momentum) * v3 + momentum * r["bvar"] * T / (T - 1)
        errs["running_mean_3"], errs["running_var_3"] = rel_l2(rm1, m3), rel_l2(rv1, v3)
    return errs


@pytest.mark.parametrize("training", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("f", WIDTHS)
def test_batchnorm_kernels(GT, gpu_device, f, training):
    from galerkin_transformer import _hip
    eps, momentum = 1e-5, 0.1
    for T in (WIDE_ROWS if f == WIDE else ROWS):
        data = _data(T, f, gpu_device, 1000 * f + T)
        errs = _kernel_errors(_hip, *data, eps, momentum, training, seed=f + T)
        print(f, T, "train" if training else "eval", {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < KTOL for v in errs.values()), (T, {k: v for k, v in errs.items() if not v < KTOL})


def test_two_rows_stay_finite(GT, gpu_device):
    """T = 2, the least torch accepts in training mode: xh = +-1 whatever the data, so only finiteness is asked."""
    from galerkin_transformer import _hip
    x, dz, gamma, beta, rm, rv = _data(2, 64, gpu_device, 5)
    z, stats, bvar = _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True)
    gh, dg, db = _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=(_hip.AUX_GT0, None, 1.0, None))
    for t in (z, stats, bvar, rm, rv, gh, dg, db):
        assert torch.isfinite(t).all()


def test_dead_and_constant_columns(GT, gpu_device):
    """An all-zero column (a dead ReLU unit) and a constant one: variance exactly 0, z = beta exactly, everything finite, and
    behind the ReLU gate the dead unit's gradient is exactly 0."""
    from galerkin_transformer import _hip
    T, f, eps = 1849, 96, 1e-5
    x, dz, gamma, beta, rm, rv = _data(T, f, gpu_device, 11)
    x[:, 3], x[:, 40], x[:, 41] = 0.0, 7.25, -1e3
    r = _ref64(x, dz, gamma, beta, rm, rv, eps, 0.1, True)
    z, stats, bvar = _hip.batchnorm_fwd(x, gamma, beta, eps, rm, rv, 0.1, True)
    gh, dg, db = _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=(_hip.AUX_GT0, None, 1.0, None))
    for t in (z, stats, bvar, rm, rv, gh, dg, db):
        assert torch.isfinite(t).all()
    for c, v in ((3, 0.0), (40, 7.25), (41, -1e3)):
        assert float(stats[c, 0]) == v and float(bvar[c]) == 0.0
        assert float(stats[c, 1]) == pytest.approx(eps ** -0.5, rel=1e-6)
        assert torch.equal(z[:, c], beta[c].expand(T)), c
    assert (gh[:, 3] == 0).all() and (gh[:, 41] == 0).all()
    keep = torch.ones(f, dtype=torch.bool, device=gpu_device)
    keep[[3, 40, 41]] = False
    assert rel_l2(z[:, keep], r["z"][:, keep]) < KTOL
    assert rel_l2(gh[:, keep], (r["d"] * (x > 0).double())[:, keep]) < KTOL
    assert rel_l2(db, r["dbeta"]) < KTOL and rel_l2(dg[keep], r["dgamma"][keep]) < KTOL


def test_offset_column_keeps_its_digits(GT, gpu_device):
    """Every column is 1e3 + N(0, 1): |mean| / std = 1e3.  z and the gradient against float64; the allowance is what float32
    torch.nn.functional.batch_norm loses on the same data (CPU, against float64), times 4.  A variance formed as
    E[x^2] - mean^2 is off by ~5e-2 here."""
    from galerkin_transformer import _hip
    T, f, eps = 1849, 96, 1e-5
    g = torch.Generator().manual_seed(4242)
    x = (1e3 + torch.randn(T, f, generator=g)).to(gpu_device)
    dz = torch.randn(T, f, generator=g).to(gpu_device)
    gamma, beta = (1.0 + 0.5 * torch.randn(f, generator=g)).to(gpu_device), torch.randn(f, generator=g).to(gpu_device)
    rm, rv = torch.zeros(f, device=gpu_device), torch.ones(f, device=gpu_device)
    r = _ref64(x, dz, gamma, beta, rm, rv, eps, 0.1, True)
    z, stats, bvar = _hip.batchnorm_fwd(x, gamma, beta, eps, rm, rv, 0.1, True)
    gh, dg, db = _hip.batchnorm_bwd(x, dz, gamma, stats, True)
    # the yardstick: torch's own float32 operator on the CPU
    xc = x.cpu().requires_grad_(True)
    zt = F.batch_norm(xc, None, None, weight=gamma.cpu(), bias=beta.cpu(), training=True, eps=eps)
    (dt,) = torch.autograd.grad(zt, xc, dz.cpu())
    allow_z, allow_d = 4 * rel_l2(zt, r["z"]), 4 * rel_l2(dt, r["d"])
    err_z, err_d = rel_l2(z, r["z"]), rel_l2(gh, r["d"])
    print(f"offset column: z {err_z:.2e} (allowance {allow_z:.2e}), d {err_d:.2e} (allowance {allow_d:.2e}), "
          f"bvar {rel_l2(bvar, r['bvar']):.2e}, dgamma {rel_l2(dg, r['dgamma']):.2e}, dbeta {rel_l2(db, r['dbeta']):.2e}")
    assert err_z < allow_z, (err_z, allow_z)
    assert err_d < allow_d, (err_d, allow_d)


def test_zero_weights(GT, gpu_device):
    """gamma with zeros: the gradient is exactly zero there and dgamma is still right (xh comes from the raw hid)."""
    from galerkin_transformer import _hip
    x, dz, gamma, beta, rm, rv = _data(150, 64, gpu_device, 99)
    gamma[::3] = 0
    r = _ref64(x, dz, gamma, beta, rm, rv, 1e-5, 0.1, True)
    z, stats, _ = _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True)
    gh, dg, db = _hip.batchnorm_bwd(x, dz, gamma, stats, True)
    assert (gh[:, ::3] == 0).all() and float(dg[::3].abs().min()) > 0
    assert rel_l2(dg, r["dgamma"]) < KTOL and rel_l2(db, r["dbeta"]) < KTOL and rel_l2(gh, r["d"]) < KTOL


def test_refusals(GT, gpu_device):
    from galerkin_transformer import _hip
    dev = gpu_device
    x, dz, gamma, beta, rm, rv = _data(64, 30, dev, 1)
    assert _hip.lib().gt_batchnorm_ws_bytes(64, 30) == 0
    with pytest.raises(_hip.GtNotSupported):
        _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True)
    with pytest.raises(_hip.GtNotSupported):
        _hip.batchnorm_bwd(x, dz, gamma, torch.zeros(30, 2, device=dev), True)
    # one row in training mode: an error before anything is launched, the buffers untouched; eval mode takes it
    x, dz, gamma, beta, rm, rv = _data(1, 32, dev, 2)
    rm0, rv0 = rm.clone(), rv.clone()
    with pytest.raises(_hip.GtError, match="GT_EINVAL"):
        _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True)
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    z, stats, _ = _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, False)
    assert torch.isfinite(z).all() and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    # the mask replay belongs to the SiLU gate; a scratch buffer that is too small
    x, dz, gamma, beta, rm, rv = _data(64, 32, dev, 3)
    z, stats, _ = _hip.batchnorm_fwd(x, gamma, beta, 1e-5, rm, rv, 0.1, True)
    with pytest.raises(_hip.GtError, match="GT_EINVAL"):
        _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=(_hip.AUX_GT0, None, 1.0, _hip.dropout_desc(0.25, 5, dev)))
    with pytest.raises(_hip.GtError, match="GT_EINVAL"):
        _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=(_hip.AUX_DSILU, None, 1.0, None))
    with pytest.raises(_hip.GtNotSupported):
        _hip.batchnorm_bwd(x, dz, gamma, stats, True, gate=(_hip.AUX_MUL, x, 1.0, None))
    need = _hip.lib().gt_batchnorm_ws_bytes(64, 32)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    rc = _hip.lib().gt_batchnorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, rm.data_ptr(), rv.data_ptr(), 0.1,
                                     1, z.data_ptr(), stats.data_ptr(), torch.empty(32, device=dev).data_ptr(), 64, 32,
                                     ws.data_ptr(), need - 16, _hip.stream_ptr())
    assert rc == -3                                                                       # GT_EWS
    torch.cuda.synchronize()
    ff = GT.FeedForward(16, 30, batch_norm=True).to(dev)
    with _hip.Profile() as prof:
        with pytest.raises(NotImplementedError, match="multiple of 4"):
            ff(torch.randn(2, 8, 16, device=dev))
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            GT.FeedForward(16, 32, batch_norm=True).to(dev)(torch.randn(1, 1, 16, device=dev))
    assert not prof.records


# ------------------------------------------------------------------------------------ operator and modules
def _no_dropout(mod):
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return mod


def _build(GT, g):
    if g.meta["kind"] == "feed_forward":
        return GT.FeedForward(g.meta["in_dim"], g.meta["dim_feedforward"], batch_norm=True, activation=g.meta["activation"],
                              dropout=0.0)
    m = {k: v for k, v in g.meta.items() if k not in ("state_dict_keys", "training")}
    return build_module(GT, type("G", (), {"meta": m})())


def _run(mod, g, ins):
    return mod(ins["x"]) if g.meta["kind"] == "feed_forward" else run_module(mod, g, ins)


def _run_fixture(GT, dev, g):
    """The module of fixture g from its state_dict (buffers included), in the mode the fixture was recorded in: (out, d
    inputs, parameter gradients, buffers after the step)."""
    torch.manual_seed(0)
    mod = _build(GT, g)
    res = mod.load_state_dict(g.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod = _no_dropout(mod).to(dev)
    mod = mod.train() if g.meta["training"] else mod.eval()
    GT.set_attention_dropout("off")
    try:
        ins = {k: v.to(dev) for k, v in g.inputs.items()}
        for k in g.din:
            ins[k].requires_grad_(True)
        out = _run(mod, g, ins)
        out.backward(g.cot.to(dev))
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    grads = {k: p.grad for k, p in mod.named_parameters()}
    bufs = {k: v.detach().clone() for k, v in mod.state_dict().items() if k.rsplit(".", 1)[-1] in BUFFERS}
    return out.detach(), {k: ins[k].grad for k in g.din}, grads, bufs


def _gate(name, errs, noise):
    bound = {k: max(TOL, 12.0 * noise.get(k, 0.0)) for k in errs}
    ratios = {k: v / bound[k] for k, v in errs.items()}
    worst, wr = max(errs, key=errs.get), max(ratios, key=ratios.get)
    print(f"{name}: worst {worst} {errs[worst]:.2e}; worst error / bound {wr} {ratios[wr]:.2f}",
          {k: (f"{v:.1e}", f"{noise.get(k, 0.0):.1e}") for k, v in errs.items() if v > 0.5 * TOL})
    assert errs["out"] < TOL, errs["out"]
    bad = {k: (v, bound[k]) for k, v in errs.items() if not v < bound[k]}
    assert not bad, bad


def _noise(g):
    """The float32 restatement's own distance from float64, per tensor (CPU): what 1e-5 can and cannot ask of a gradient."""
    o32, di32, dp32, _ = ref_grads(g, torch.float32)
    o64, di64, dp64, _ = ref_grads(g, torch.float64)
    noise = {"d" + k: rel_l2(di32[k], di64[k]) for k in di32}
    noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64).items()})
    return noise


@pytest.mark.parametrize("mode", (None, "f32"), ids=("default", "f32"))
@pytest.mark.parametrize("name", BATCHNORM_GOLDEN)
def test_module_matches_reference_golden(GT, gpu_device, name, mode):
    """Fails on a tree without the feature: FeedForward.fused_forward raises NotImplementedError for batch_norm=True."""
    g = Golden("batchnorm/" + name)
    with precision(mode):
        out, din, grads, bufs = _run_fixture(GT, gpu_device, g)
    assert out.shape == g.out.shape
    errs = {"out": rel_l2(out, g.out)}
    errs.update({"d" + k: rel_l2(din[k], g.din[k]) for k in g.din})
    for k in g.dparam:
        assert grads[k] is not None, k
    errs.update({"dW:" + k: v for k, v in grad_errors(grads, g.dparam).items()})
    _gate(f"{name} [{mode or 'default'}]", errs, _noise(g))
    # the buffers: after a training step the reference's, after an eval step the ones that went in, bit for bit
    training = g.meta["training"]
    want = buffers_after(name) if training else {k: g.sd[k] for k in bufs}
    assert sorted(want) == sorted(bufs) and len(bufs) == 3 * len(bn_prefixes(g.sd))
    for k, v in want.items():
        if k.endswith("num_batches_tracked"):
            assert bufs[k].dtype == torch.int64 and int(bufs[k]) == int(v) == 3 + int(training), k
        elif training:
            assert rel_l2(bufs[k], v) < KTOL, (k, rel_l2(bufs[k], v))
            assert not torch.equal(bufs[k].cpu(), g.sd[k]), k
        else:
            assert torch.equal(bufs[k].cpu(), v), k


@pytest.mark.parametrize("act,d,f,n", (("relu", 128, 256, 150), ("silu", 96, 192, 33)))
def test_dropout_in_front_of_the_norm(GT, gpu_device, act, d, f, n):
    """ops.feed_forward_bn with p_h = 0.25: the statistics see the dropped, rescaled hidden values.  The mask is rebuilt from
    the salt the operator drew (out.grad_fn.cfg) with the elementwise kernel and replayed in the float64 restatement; the
    module bar applies, its noise term from the float32 restatement on the CPU with the same mask."""
    from galerkin_transformer import _hip, ops
    dev, B, p_h = gpu_device, 2, 0.25
    gen = torch.Generator().manual_seed(31 + d)
    rn = lambda *s, scale=1.0: scale * torch.randn(*s, generator=gen)
    sd = {"lr1.weight": rn(f, d, scale=d ** -0.5), "lr1.bias": rn(f, scale=0.1), "lr2.weight": rn(d, f, scale=f ** -0.5),
          "lr2.bias": rn(d, scale=0.1), "bn.weight": 1.0 + rn(f, scale=0.3), "bn.bias": rn(f, scale=0.3),
          "bn.running_mean": rn(f, scale=0.1), "bn.running_var": 0.5 + torch.rand(f, generator=gen)}
    x, cot = rn(B, n, d), rn(B, n, d)
    names = [k for k in sd if "running" not in k]
    for res in (False, True):
        p = {k: v.clone().to(dev).requires_grad_(k in names) for k, v in sd.items()}
        xg = x.to(dev).requires_grad_(True)
        out = ops.feed_forward_bn(xg, p["lr1.weight"], p["lr1.bias"], p["lr2.weight"], p["lr2.bias"], p["bn.weight"],
                                  p["bn.bias"], p["bn.running_mean"], p["bn.running_var"], res=xg if res else None, act=act,
                                  p_h=p_h, p_out=0.0, eps=1e-5, momentum=0.1, training=True)
        cfg = out.grad_fn.cfg
        assert cfg[1] == p_h and cfg[2] == 0.0
        mask = _hip.dropout_apply(torch.ones(B * n, f, device=dev), _hip.dropout_desc(p_h, cfg[3], dev)).cpu()
        assert 0.2 < float((mask == 0).float().mean()) < 0.3
        grads = torch.autograd.grad(out, [xg] + [p[k] for k in names], cot.to(dev))
        torch.cuda.synchronize()

        def ref(dtype):
            s = {k: v.to(dtype).requires_grad_(k in names) for k, v in sd.items()}
            xx, ups = x.to(dtype).requires_grad_(True), []
            o = feed_forward_bn(s, xx, act, True, drop_mask=mask.reshape(B, n, f), updates=ups)
            o = o + xx if res else o
            gs = torch.autograd.grad(o, [xx] + [s[k] for k in names], cot.to(dtype))
            return o.detach(), gs[0], dict(zip(names, gs[1:])), ups[0]

        o64, dx64, dp64, up64 = ref(torch.float64)
        o32, dx32, dp32, _ = ref(torch.float32)
        errs = {"out": rel_l2(out, o64), "dx": rel_l2(grads[0], dx64)}
        errs.update({"dW:" + k: v for k, v in grad_errors(dict(zip(names, grads[1:])), dp64).items()})
        noise = {"dx": rel_l2(dx32, dx64)}
        noise.update({"dW:" + k: v for k, v in grad_errors(dp32, dp64).items()})
        _gate(f"feed_forward_bn {act} p_h={p_h} res={res}", errs, noise)
        assert rel_l2(p["bn.running_mean"], up64[0]) < KTOL and rel_l2(p["bn.running_var"], up64[1]) < KTOL


# ------------------------------------------------------------------------------------ behaviour
def _layer(GT, dev, name="enc_galerkin_bn_c2"):
    g = Golden("batchnorm/" + name)
    mod = _build(GT, g)
    mod.load_state_dict(g.sd, strict=True)
    return g, _no_dropout(mod).to(dev)


def _buffers(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if k.rsplit(".", 1)[-1] in BUFFERS}


@pytest.mark.parametrize("mode", MODES, ids=("default", "f32", "bf16"))
def test_train_step_changes_the_buffers_eval_step_does_not(GT, gpu_device, mode):
    dev = gpu_device
    g, mod = _layer(GT, dev)
    x, pos, cot = g.inputs["x"].to(dev), g.inputs["pos"].to(dev), g.cot.to(dev)
    GT.set_attention_dropout("off")
    try:
        with precision(mode):
            b0 = _buffers(mod)
            mod.eval()
            y_eval = mod(x.clone().requires_grad_(True), pos)
            y_eval.backward(cot)
            b1 = _buffers(mod)
            assert all(torch.equal(b0[k], b1[k]) for k in b0)
            mod.train()
            y_train = mod(x.clone().requires_grad_(True), pos)
            y_train.backward(cot)
            b2 = _buffers(mod)
            assert all(not torch.equal(b1[k], b2[k]) for k in b1)
            assert int(b2["ff.bn.num_batches_tracked"]) == int(b1["ff.bn.num_batches_tracked"]) + 1
            assert torch.isfinite(y_train).all() and rel_l2(y_train, y_eval) > 1e-3          # batch vs running statistics
            mod.eval()
            y_eval2 = mod(x, pos)
            assert all(torch.equal(b2[k], v) for k, v in _buffers(mod).items())
            assert not torch.equal(y_eval2, y_eval)                                          # the new buffers are in use
            # the norm's buffers are the reference's whatever arithmetic the products around it run in: the kernels are fp32
            if mode != "bf16":
                want = buffers_after("enc_galerkin_bn_c2")
                assert rel_l2(b2["ff.bn.running_var"], want["ff.bn.running_var"]) < 10 * KTOL
    finally:
        GT.set_attention_dropout("reference")


@pytest.mark.parametrize("mode", MODES, ids=("default", "f32", "bf16"))
def test_graph_capture_replays_eager(GT, gpu_device, mode):
    """One captured training step, replayed three times, against three eager steps from the same state: the gradients, the
    running buffers and num_batches_tracked, bit for bit."""
    dev = gpu_device
    g, mod = _layer(GT, dev)
    mod.train()
    x = g.inputs["x"].to(dev).requires_grad_(True)
    pos, cot = g.inputs["pos"].to(dev), g.cot.to(dev)
    params = list(mod.parameters())
    start = _buffers(mod)

    def reset():
        with torch.no_grad():
            for k, v in mod.state_dict().items():
                if k in start:
                    v.copy_(start[k])

    def step():
        return torch.autograd.grad(mod(x, pos), [x] + params, cot)

    GT.set_attention_dropout("off")
    try:
        with precision(mode):
            for _ in range(3):
                eager = [t.clone() for t in step()]
            eager_bufs = _buffers(mod)
            assert int(eager_bufs["ff.bn.num_batches_tracked"]) == int(start["ff.bn.num_batches_tracked"]) + 3
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    step()
            torch.cuda.current_stream().wait_stream(s)
            reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                captured = step()
            reset()                      # a capture runs nothing, but whatever it did to the buffers is undone here
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    for k, v in _buffers(mod).items():
        assert torch.equal(v, eager_bufs[k]), k


@pytest.mark.parametrize("mode", MODES, ids=("default", "f32", "bf16"))
def test_batch_norm_false_is_unaffected(GT, gpu_device, mode):
    """batch_norm=False: FeedForward is ops.feed_forward as before, bit for bit, and no gt_batchnorm_* launch is made -- also
    after layers with the norm ran in the same process.  With the norm: one forward and one backward launch per layer."""
    from galerkin_transformer import _hip, ops
    dev = gpu_device
    torch.manual_seed(5)
    ff = GT.FeedForward(128, 256, batch_norm=False, dropout=0.0).to(dev).train()
    x, cot = torch.randn(2, 150, 128, device=dev), torch.randn(2, 150, 128, device=dev)

    def plain():
        xg = x.clone().requires_grad_(True)
        y = ops.feed_forward(xg, ff.lr1.weight, ff.lr1.bias, ff.lr2.weight, ff.lr2.bias, res=xg, act="relu")
        return [y.detach()] + list(torch.autograd.grad(y, [xg] + list(ff.parameters()), cot))

    def module():
        xg = x.clone().requires_grad_(True)
        y = ff.fused_forward(xg, residual=xg)
        return [y.detach()] + list(torch.autograd.grad(y, [xg] + list(ff.parameters()), cot))

    GT.set_attention_dropout("off")
    try:
        with precision(mode):
            before = plain()
            g, layer = _layer(GT, dev)
            layer.train()
            with _hip.Profile() as prof:
                out = layer(g.inputs["x"].to(dev).requires_grad_(True), g.inputs["pos"].to(dev))
                out.backward(g.cot.to(dev))
            keys = [r[0] for r in prof.records]
            assert keys.count("gt_batchnorm_fwd") == 1 and keys.count("gt_batchnorm_bwd") == 1
            with _hip.Profile() as prof:
                after = module()
            assert prof.records and not [r[0] for r in prof.records if "batchnorm" in r[0]]
            torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    assert not hasattr(ff, "bn") and len(before) == len(after)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
