"""The Galerkin core on the device (-m gpu), per element against float64: gt_galerkin_ktv[_affine] on both kernels and at a
slab count of the test's choosing, gt_galerkin_finalize_fwd/bwd on every row grouping and parts count of their launchers and
in the three multiplier modes, gt_galerkin_dkv and gt_galerkin_dkv_ln[_plain]; then SimpleAttention('galerkin') on the routes
no fixture takes (more than four heads, h DP > 256).

Gate (tests/_galerkin_ref.py: gate_violation).  |got - ref64| <= 4 R32[family] 2^-24 E per element, E the contract's formula on
absolute values, and an exact zero wherever E == 0 (pads, masked-out entries, empty chunks); no element is left out.  R32 is
the float32 restatement's own largest normalised error over the family's cases, measured on the CPU by
tests/test_galerkin_ref_cpu.py (never on a kernel); the factor 4 covers an accumulation order other than index order
(four-token MFMA steps, the four token lanes of the borders, the wave fold in LDS, four slab chains).

    family     R32 (CPU)   largest device ratio |got - ref64| / (2^-24 E)
    ktv        7.7         7.69  (2,64,4,64,0,1) affine, slabs
    fin_fwd    4.7         4.66  (128,8,20,18,16,1) mask, P
    fin_bwd    5.3         5.08  (128,8,20,18,16,1) drop, dWfc
    dkv        5.0         4.38  (2,50,4,36,0), dK
    dkv_ln     2.7         2.47  (300,17,4,16,2) affine, dx

Every output buffer is pre-filled with NaN and written through the C ABI; the second launch of every case goes through the
binding's own wrapper and is bit-identical (the kernels have no atomics).

Kernel of every ktv case (the launcher's predicate, restated in _galerkin_ref.ktv_staged: h <= 4, h DP <= 256, 16-byte aligned
tiles -> galerkin_ktv_lds_kernel, else galerkin_ktv_kernel; the Profile record names the entry point only):
    staged  (B, n, h, dk, p, slabs) = (1,1,1,16,0,1) (1,17,2,16,1,1) (2,130,4,32,2,3) (1,63,3,48,2,4) (2,65,1,96,1,2)
            (2,64,4,64,0,1) (1,100,2,16,2,7) (1,20,2,16,2,8)
    stream  (2,70,5,16,2,2) (1,33,8,16,1,1) (1,50,9,16,0,3) (2,65,6,32,0,2) (1,40,4,64,2,2) (1,35,3,96,1,2)
            (2,130,2,32,2,3) with the tiles one float off a 16-byte boundary

gt_galerkin_dkv[_ln] take head tiles of 20, 36 and 52 floats.  The case (1,17,1,16,0) has DP = 16: the launchers refuse it
(GT_ENOTSUP, nothing written), which is what the test asserts for it; (1,17,1,16,2) runs the B h = 1 grid instead.

Modules (B = 2, n = 70, self-attention, norm=True), the bars of test_cross_attention_gpu.py: output below TOL = 1e-5, every
other tensor below max(TOL, 12 x the float32 restatement's deviation from float64).  Measured error (worst tensor) / its bar:
    (d_model, n_head, pos_dim)   output          worst other tensor
    (128, 8, 1)                  3.5e-07 / 1e-5  6.6e-07 / 1e-5  (dW norm_K.0.weight)
    (80, 5, 2)                   2.8e-07 / 1e-5  4.3e-07 / 1e-5  (dW norm_V.1.weight)
    (256, 4, 2)                  5.2e-07 / 1e-5  6.5e-07 / 1e-5  (dx)
    (96, 6, 0)                   2.4e-07 / 1e-5  3.9e-07 / 1e-5  (dW norm_V.2.weight)
    (128, 8, 1) replay           3.4e-07 / 1e-5  5.5e-07 / 1e-5  (dW norm_K.5.bias)
(12 x the float32 restatement's deviation stayed below TOL for every tensor, so every bar is TOL.)"""
import pytest
import torch

import _galerkin_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


def _nan(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(tag, name, got, ref, E, fam):
    got = got.detach().cpu()
    print(f"ratio {fam:<8s} {tag:<36s} {name:<8s} {R.ratio(got, ref, E):.2f}")
    bad = R.gate_violation(got, ref, E, fam)
    assert bad is None, (tag, name, bad)


def _cases(fam):
    return [pytest.param(c, id=c["id"]) for c in R.CASES if c["fam"] == fam]


# ---------------------------------------------------------------------------------------------- K^T V
@pytest.mark.parametrize("variant", ("affine", "plain"))
@pytest.mark.parametrize("case", _cases("ktv"))
def test_ktv(H, gpu_device, case, variant):
    dev = gpu_device
    B, n, h, dk, p, S = (case[k] for k in ("B", "n", "h", "dk", "p", "S"))
    DP = R.round4(dk + p)
    ops = R.build_case(case)
    K, V = (ops["Kt"], ops["Vt"]) if variant == "affine" else (ops["Kx"], ops["Vx"])
    if case["mis"]:             # views one float into a larger buffer
        def shifted(t):
            buf = torch.zeros(t.numel() + 8, device=dev)
            buf[1:1 + t.numel()] = t.reshape(-1).to(dev)
            return buf[1:1 + t.numel()].view(t.shape)
        Kd, Vd = shifted(K), shifted(V)
        assert Kd.data_ptr() % 16 == 4 and Vd.data_ptr() % 16 == 4
    else:
        Kd, Vd = K.to(dev), V.to(dev)
    gamma, beta = (None, None) if variant == "affine" else (ops["gamma"].to(dev), ops["beta"].to(dev))
    assert H.galerkin_ktv_supported(dk, p)
    assert R.ktv_staged(Kd, Vd, h, dk, p) == (case["route"] == "staged"), "the case is on another kernel than it says"
    slabs = _nan(dev, S, B, h, DP, DP)
    H._launch("gt_galerkin_ktv_affine", Kd, Vd, gamma, beta, B, n, h, dk, p, slabs, S)
    with H.Profile() as prof:
        again = H.galerkin_ktv(Kd, Vd, B, n, h, dk, p, gamma=gamma, beta=beta, n_slabs=S)
    torch.cuda.synchronize()
    assert [r[0] for r in prof.records] == ["gt_galerkin_ktv"] and tuple(prof.records[0][6]) == (B, n, h, dk, p)
    assert _bits_equal(slabs, again), "second launch differs"
    ref, E = R.evaluate(case, ops, "ktv", variant)["slabs"]
    tag = f"{case['id']} {variant}"
    _check(tag, "slabs", slabs, ref, E, "ktv")
    _check(tag, "sum", slabs.double().sum(0), ref.sum(0), E.sum(0), "ktv")
    for q, (lo, hi) in enumerate(R.chunks(n, S)):
        if lo >= hi:
            assert not bool(slabs[q].any()), ("an empty chunk's slab", q)


def test_ktv_default_slab_count_is_the_librarys(H, gpu_device):
    """n_slabs=None keeps gt_galerkin_ktv_slabs, and the slabs of any count sum to the same matrix."""
    case = next(c for c in R.CASES if c["id"] == "ktv-2x130x4x32x2-s3")
    ops = R.build_case(case)
    K, V = ops["Kt"].to(gpu_device), ops["Vt"].to(gpu_device)
    a = H.galerkin_ktv(K, V, 2, 130, 4, 32, 2)
    torch.cuda.synchronize()
    assert a.shape[0] == H.lib().gt_galerkin_ktv_slabs(2, 130) == 3
    ref, E = R.ktv_ref(ops["Kt"], ops["Vt"], 2, 130, 4, 32, 2, a.shape[0])
    _check(case["id"], "default", a, ref, E, "ktv")


# ---------------------------------------------------------------------------------------------- finalize
@pytest.mark.parametrize("mode", R.FIN_MODES)
@pytest.mark.parametrize("case", _cases("fin"))
def test_finalize(H, gpu_device, case, mode):
    """Forward and backward in one multiplier mode.  'mask' and 'drop' read their slabs at a stride larger than a slab, the
    gap full of NaN; n_tokens differs from every other dimension in all three."""
    dev = gpu_device
    B, h, DP, Dr, d, S, p, nt = (case[k] for k in ("B", "h", "DP", "Dr", "d", "S", "p", "n_tokens"))
    assert nt not in (B, h, DP, Dr, d, S, B * h)
    ops = R.build_case(case)
    dense = B * h * DP * DP
    stride = dense if mode == "none" else dense + 24
    flat = _nan(dev, S * stride)
    torch.as_strided(flat, (S, dense), (stride, 1)).copy_(ops["slabs"].reshape(S, dense))
    Wfc, dPt = ops["Wfc"].to(dev), ops["dPt"].to(dev)
    mask = ops["mask"].to(dev) if mode == "mask" else None
    H.set_seed(R.SEED, dev)
    assert int(H.seed_state(dev).item()) == R.SEED
    drop = H.dropout_desc(R.DROP_P, R.fin_salt(case), dev) if mode == "drop" else None
    ref = R.evaluate(case, ops, "fin", mode)
    tag = f"{case['id']} {mode}"

    Mt, P, Pv = _nan(dev, B, h, DP, DP), _nan(dev, B, h * DP, d), _nan(dev, B, h * (Dr - p), d)
    H._launch("gt_galerkin_finalize_fwd", flat, S, stride, B, h, DP, Dr, d, nt, mask, drop, Wfc, Mt, P, Pv, p)
    again = H.galerkin_finalize_fwd(flat, S, stride, B, h, DP, Dr, d, nt, mask, drop, Wfc, value_rows_of=p)
    torch.cuda.synchronize()
    for a, b, name in zip((Mt, P, Pv), again, ("Mt", "P", "Pv")):
        assert _bits_equal(a, b), (name, "second launch differs")
    for name, got in (("Mt", Mt), ("P", P), ("Pv", Pv)):
        _check(tag, name, got, *ref[name], "fin_fwd")
    assert _bits_equal(Pv, P.view(B, h, DP, d)[:, :, p:Dr].reshape(B, h * (Dr - p), d)), "Pv is not the value rows of P"
    if DP > Dr:
        assert not bool(Mt[:, :, Dr:].any()) and not bool(Mt[:, :, :, Dr:].any()), "pad rows / columns of Mt"
        assert not bool(P.view(B, h, DP, d)[:, :, Dr:].any()), "pad rows of P"
    if mode != "none":          # the multiplier's zeros are exact zeros of M (and some are there)
        mul = R.fin_mul(B, h, DP, ops["mask"] if mode == "mask" else None,
                        (R.SEED, R.fin_salt(case), R.DROP_P) if mode == "drop" else None)
        dead = (mul == 0)[:, :, :Dr, :Dr]
        assert 0.2 < float(dead.double().mean()) < 0.8
        assert not bool(Mt.cpu()[:, :, :Dr, :Dr][dead].any())

    Mt_in = R.fin_Mt_in(case, ops, mode).to(dev)
    dM, dW = _nan(dev, B, h, DP, DP), _nan(dev, B, d, h * Dr)
    H._launch("gt_galerkin_finalize_bwd", dPt, Mt_in, mask, drop, Wfc, B, h, DP, Dr, d, nt, dM, dW)
    again = H.galerkin_finalize_bwd(dPt, Mt_in, mask, drop, Wfc, B, h, DP, Dr, d, nt)
    torch.cuda.synchronize()
    for a, b, name in zip((dM, dW), again, ("dM", "dW")):
        assert _bits_equal(a, b), (name, "second launch differs")
    _check(tag, "dM", dM, *ref["dM"], "fin_bwd")
    _check(tag, "dW", dW, *ref["dW"], "fin_bwd")            # every sample's slab against its own reference
    if DP > Dr:
        assert not bool(dM[:, :, Dr:].any()) and not bool(dM[:, :, :, Dr:].any()), "pad rows / columns of dM"


# ---------------------------------------------------------------------------------------------- dK', dV'
def _dkv_ln_abi(H, dev, K, V, dM, dQp, qkv, gamma, beta, stats, B, n, h, dk, p, d_qkv):
    dg, db = _nan(dev, 2, h, dk), _nan(dev, 2, h, dk)
    ws = H.workspace(dev, H.lib().gt_galerkin_dkv_ln_ws_bytes(B, h, dk))
    H._launch("gt_galerkin_dkv_ln_plain", K, V, dM, dQp, qkv, gamma, beta, stats, B, n, h, dk, p, d_qkv, dg, db, ws=ws)
    return d_qkv, dg, db


@pytest.mark.parametrize("case", _cases("dkv"))
def test_dkv_and_dkv_ln(H, gpu_device, case):
    dev = gpu_device
    B, n, h, dk, p = (case[k] for k in ("B", "n", "h", "dk", "p"))
    T, DP, hd = B * n, R.round4(dk + p), h * dk
    ops = R.build_case(case)
    o = {k: v.to(dev) for k, v in ops.items()}
    dK, dV = _nan(dev, T, h, DP), _nan(dev, T, h, DP)
    if DP not in R.DKV_DP:       # no kernel for this head tile: refused before any launch, the callers fall back
        assert not H.galerkin_dkv_ln_supported(dk, p, 0b110)
        d_qkv = _nan(dev, T, 3 * hd)
        with H.Profile() as prof:
            with pytest.raises(H.GtNotSupported):
                H.galerkin_dkv(o["Kt"], o["Vt"], o["dM"], dK, dV, B, n, h, DP)
            with pytest.raises(H.GtNotSupported):
                H.galerkin_dkv_ln(o["Kt"], o["Vt"], o["dM"], o["dQp"], o["qkv"], o["gamma"], o["stats"], B, n, h, dk, p, d_qkv=d_qkv)
            with pytest.raises(H.GtNotSupported):
                H.galerkin_dkv_ln(o["Kx"], o["Vx"], o["dM"], o["dQp"], None, o["gamma"], o["stats"], B, n, h, dk, p, d_qkv=d_qkv,
                                  beta=o["beta"])
        torch.cuda.synchronize()
        assert not prof.records
        assert bool(torch.isnan(dK).all()) and bool(torch.isnan(dV).all()) and bool(torch.isnan(d_qkv).all())
        return
    H._launch("gt_galerkin_dkv", o["Kt"], o["Vt"], o["dM"], dK, dV, B, n, h, DP)
    dK2, dV2 = _nan(dev, T, h, DP), _nan(dev, T, h, DP)
    H.galerkin_dkv(o["Kt"], o["Vt"], o["dM"], dK2, dV2, B, n, h, DP)
    torch.cuda.synchronize()
    assert _bits_equal(dK, dK2) and _bits_equal(dV, dV2), "second launch differs"
    ref = R.evaluate(case, ops, "dkv", "tiles")
    _check(case["id"], "dK", dK, *ref["dK"], "dkv")
    _check(case["id"], "dV", dV, *ref["dV"], "dkv")

    assert H.galerkin_dkv_ln_supported(dk, p, 0b110)
    for variant in ("affine", "plain"):
        K, V, qkv, beta = (o["Kt"], o["Vt"], o["qkv"], None) if variant == "affine" else (o["Kx"], o["Vx"], None, o["beta"])
        args = (K, V, o["dM"], o["dQp"], qkv, o["gamma"])
        tag = f"{case['id']} {variant}"
        # with dQp: the Q block is the value columns of dQp
        d_qkv, dg, db = _dkv_ln_abi(H, dev, *args, beta, o["stats"], B, n, h, dk, p, _nan(dev, T, 3 * hd))
        again = H.galerkin_dkv_ln(*args, o["stats"], B, n, h, dk, p, beta=beta)
        torch.cuda.synchronize()
        for a, b, name in zip((d_qkv, dg, db), again, ("d_qkv", "dgamma", "dbeta")):
            assert _bits_equal(a, b), (variant, name, "second launch differs")
        assert _bits_equal(d_qkv[:, :hd], o["dQp"][:, :, p:p + dk].reshape(T, hd)), "Q block"
        ref = R.evaluate(case, ops, "dkv_ln", variant)
        _check(tag, "dx", torch.stack([d_qkv[:, hd:2 * hd], d_qkv[:, 2 * hd:]]), *ref["dx"], "dkv_ln")
        _check(tag, "dgamma", dg, *ref["dgamma"], "dkv_ln")
        _check(tag, "dbeta", db, *ref["dbeta"], "dkv_ln")
        # without dQp: the caller's Q block stays as it is, the rest is the same
        mine = _nan(dev, T, 3 * hd)
        mine[:, :hd] = torch.arange(T * hd, device=dev, dtype=torch.float32).reshape(T, hd) * 0.5 - 3.0
        keep = mine[:, :hd].clone()
        d2, dg2, db2 = _dkv_ln_abi(H, dev, K, V, o["dM"], None, qkv, o["gamma"], beta, o["stats"], B, n, h, dk, p, mine)
        torch.cuda.synchronize()
        assert _bits_equal(d2[:, :hd], keep), "the Q block was touched"
        assert _bits_equal(d2[:, hd:], d_qkv[:, hd:]) and _bits_equal(dg2, dg) and _bits_equal(db2, db)


# ---------------------------------------------------------------------------------------------- the module on those routes
class _Fixture:
    """What _cross_ref.ref_grads / all_errors and test_cross_attention_gpu._run read of a Golden, made on the spot."""

    def __init__(self, GT, d_model, n_head, pos_dim, replay):
        B, n = 2, 70
        gen = torch.Generator().manual_seed(1000 * d_model + 10 * n_head + pos_dim)
        self.meta = dict(n_head=n_head, d_model=d_model, pos_dim=pos_dim, attention_type="galerkin", norm=True,
                         norm_type="layer", eps=1e-5, form=("x", "x", "x"))
        torch.manual_seed(0)
        mod = GT.SimpleAttention(n_head, d_model, pos_dim=pos_dim, attention_type="galerkin", dropout=0.0, norm=True, eps=1e-5)
        with torch.no_grad():       # off the initialisation: every weight, gamma and beta of its own size
            for prm in mod.parameters():
                prm.add_(0.1 * torch.randn(prm.shape, generator=gen))
        self.sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        self.inputs = {"x": torch.randn(B, n, d_model, generator=gen)}
        if pos_dim:
            self.inputs["pos"] = torch.rand(B, n, pos_dim, generator=gen)
        self.din = {"x": None}
        self.dparam = {k: None for k in self.sd}
        self.cot = torch.randn(B, n, d_model, generator=gen)
        Dr = d_model // n_head + pos_dim
        self.masks = [(torch.rand(B, n_head, Dr, Dr, generator=gen) >= 0.5).float() * 2.0] if replay else []


@pytest.mark.parametrize("d_model,n_head,pos_dim,replay", [(128, 8, 1, False), (80, 5, 2, False), (256, 4, 2, False),
                                                           (96, 6, 0, False), (128, 8, 1, True)])
def test_module_on_the_streaming_route(gpu_device, d_model, n_head, pos_dim, replay):
    """SimpleAttention('galerkin') as self-attention with more than four heads or h DP > 256 against the float64 restatement:
    forward, the returned weight and every gradient; a gt_galerkin_ktv launch is among the records (not the gt_gemm fallback)."""
    import galerkin_transformer as GT
    from galerkin_transformer import _hip
    from _cross_ref import all_errors, ref_grads
    from _util import TOL
    from test_cross_attention_gpu import _gate, _run
    _hip.lib()
    g = _Fixture(GT, d_model, n_head, pos_dim, replay)
    dk = d_model // n_head
    assert n_head > 4 or n_head * R.round4(dk + pos_dim) > 256, "a case of the staged kernel"
    with _hip.Profile() as prof:
        out, w, din, grads = _run(GT, gpu_device, g)
    ktv = [r for r in prof.records if r[0] == "gt_galerkin_ktv"]
    assert len(ktv) == 1 and tuple(ktv[0][6]) == (2, 70, n_head, dk, pos_dim), [r[0] for r in prof.records]
    r64 = ref_grads(g, torch.float64)
    assert w is not None and w.shape == r64[1].shape
    for k in g.dparam:
        assert grads[k] is not None, k
    errs = all_errors(out, w, din, grads, *r64, g)
    noise = all_errors(*ref_grads(g, torch.float32), *r64, g)
    name = f"galerkin d{d_model} h{n_head} p{pos_dim}" + (" replay" if replay else "")
    bars = {k: (TOL if k == "out" else max(TOL, 12.0 * noise.get(k, 0.0))) for k in errs}
    worst = max(errs, key=lambda k: errs[k] / bars[k])
    print(f"module {name}: out {errs['out']:.1e} / {bars['out']:.1e}, worst {worst} {errs[worst]:.1e} / {bars[worst]:.1e}")
    _gate(name, errs, noise)
