"""Every gt_gemm engine against the header's epilogue formula (tests/_gemm_ref.py), element by element.  (-m gpu)

The formula of include/gt_hip.h is implemented by the fp32 tile and streamed kernels (vec4 / vec2 / scalar stores, five tile
configurations), the split-operand ring and staged kernels, the packed-B kernels (fast and per-row epilogue) and, by hand,
by the pointer re-basing of the width split.  Each case of `_gemm_ref.CASES` runs one of them -- confirmed through
gt_gemm_kernel_name on the plain product of the same shape and alignment, so that a routing change fails loudly -- with every
epilogue operand a view into a larger buffer of its own pitch, guard rows and batch gaps, the outputs pre-filled with a
sentinel bit pattern.

Checks without a tolerance: guard cells keep the sentinel and every cell inside is written; where the dropout mask (rebuilt on
the host from the device seed, `_gemm_ref.drop_mask`) or GT_AUX_GT0 zeroes an element, C is `res` bit for bit (0 without a
residual); c_masked is C * keepscale or 0, from the C that was written; the same call twice gives the same bits.

The gate, per element of C, pre and c_masked:   |got - ref64| <= c 2^-24 E + 2^-24 |ref64|
with E the envelope of `_gemm_ref.gemm_ref` and c = 4 x the family's largest normalised error of the float32 restatement
(`_gemm_ref.R32`, measured and pinned by tests/test_gemm_ref_cpu.py -- never taken from a kernel).  ReLU decisions within
8 x 2^-24 E of zero are left out (share <= 1e-4, pinned there too); nothing else is.  The fp32 kernels and bf16x3 (three
exact bf16 terms, products down to 2^-16 of a term in fp32) are held to this fp32-class bound.

GT_PREC_F16X2 on the packed-B kernels (gemm_x3h_kernel) is not fp32-class per PRODUCT but per row and weight tile
("Numerical guarantees of the two-term fp16 arithmetic"): a value is scaled by a power of two 2^e that tracks
its activation row (its 32-column weight tile), 2^e < 2 max|x|, and kept as two fp16 terms h0 + h1 of the scaled value.
h0 carries 11 significand bits, h1 the next 11 unless fp16's fixed step at that scale cuts them: |x - 2^e (h0 + h1)| <=
2^-23 2^e <= 2^-22 max|x| -- an absolute bound under the ROW's scale, not relative to x.  The kernel forms h0 g0 + h0 g1 +
h1 g0 and drops h1 g1, |h1 g1| <= 2^-12 2^-12 2^ea 2^eb <= 2^-22 rowmax|A_m| tilemax|B|.  Each of the three contributions to
one term a b is therefore <= 2^-22 rowmax|A_m| tilemax|B|, so the product's own error is bounded by
    sum_k 2^-22 rowmax|A_m| tilemax|B|   =   2^-22 K rowmax|A_m| tilemax|B|
per contribution, 3 x that in the worst case.  The gate for that kernel is
    |got - ref64| <= 4 x 2^-22 K rowmax|A_m| tilemax|B| G  +  c 2^-24 E  +  2^-24 |ref64|
(G: the factor the product enters the output with -- |alpha|, the activation's Lipschitz bound, |f(aux)|, keep scale,
|out_scale|; the second term is the fp32 accumulation and epilogue as above).  Inputs are of one magnitude class (normal
deviates), so rowmax and tilemax are within a small factor of the typical value and the bound stays tight."""
import ctypes as C

import pytest
import torch

import _gemm_ref as R
from _gemm_ref import CASES
from _util import rel_l2

pytestmark = pytest.mark.gpu

KTOL = 2e-6                 # the suite's global relative-L2 gate (fp32 accumulation-order noise), kept as a second assertion
X3_TOL = {"f32": 2e-6, "bf16x3": 2e-6, "f16x2": 2e-6}
SEED = 0x0123_4567_89AB_CDEF
_BY_ID = {c["id"]: c for c in CASES}
_SMALL = [c["id"] for c in CASES if c["fam"] != "wsplit"]
_WIDE = [c["id"] for c in CASES if c["fam"] == "wsplit"]


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pack_ahead(H, monkeypatch, keep):
    """gt_gemm_desc.b_packed through the binding's own hook: weight_packs.use() is where `_hip.gemm(weight_b=True)` takes a
    weight packed ahead from; here it packs on the spot with gt_gemm_pack_b_many."""
    def use(d, B):
        L = H.lib()
        need = int(L.gt_gemm_packed_b_bytes(C.byref(d)))
        assert need > 0, "not a packed-B product"
        pack = torch.empty(need, dtype=torch.uint8, device=B.device)
        descs = (H.GtGemmDesc * 1)(H.GtGemmDesc.from_buffer_copy(d))
        H.check(L.gt_gemm_pack_b_many(descs, (C.c_void_p * 1)(pack.data_ptr()), 1, H.stream_ptr()), "gt_gemm_pack_b_many")
        d.b_packed = pack.data_ptr()
        keep.append(pack)
    monkeypatch.setattr(H.weight_packs, "use", use)


def _launch(H, dev, fields, ahead=False):
    kw = dict(fields)
    A, B, Cout, M, N, K = (kw.pop(k) for k in ("A", "B", "Cout", "M", "N", "K"))
    for k in ("drop", "a_drop", "c_mask"):
        if kw.get(k) is not None:
            kw[k] = H.dropout_desc(kw[k][0], kw[k][1], dev)
    H.gemm(A, B, Cout, M, N, K, weight_b=ahead, **kw)


def _setup(H, dev, case, monkeypatch):
    if case["cfg"] is not None:
        monkeypatch.setenv("GT_GEMM_CFG", str(case["cfg"]))      # make_plan reads it per call
    else:
        monkeypatch.delenv("GT_GEMM_CFG", raising=False)
    monkeypatch.delenv("GT_GEMM_BK", raising=False)
    H.set_seed(SEED, dev)
    seed = int(H.seed_state(dev).item())
    assert seed == SEED
    fields, outs = R.build_case(case, dev)
    name = H.gemm_kernel_name(fields["A"], fields["B"], case["M"], case["N"], case["K"], layout_a=case["la"], layout_b=case["lb"],
                              lda=fields["lda"], ldb=fields["ldb"], ldc=fields["ldc"], split_k=fields["split_k"],
                              precision=case["prec"])
    assert R.expected_kernel(case) in name, (case["id"], name)
    return fields, outs, seed, name


def _check(case, fields, outs, ref, name, report):
    fam, cid = case["fam"], case["id"]
    # ---- without a tolerance, first.  Guard cells (pad columns, guard rows, batch gaps) are bitwise the sentinel and
    # everything inside is written
    for out, buf in outs.items():
        inside, bits = buf.inside(), buf.bits()
        assert bool((bits[~inside] == R.SENTINEL).all()), (cid, out, "a store outside [:M, :N]")
        assert not bool((bits[inside] == R.SENTINEL).any()), (cid, out, "an element was not written")
    # exact zeros of the epilogue factor (host mask, GT_AUX_GT0 on aux <= 0): C is the residual, bit for bit
    Cg = outs["C"].view()
    z = ref["zeroed"]
    if bool(z.any()):
        if fields.get("res") is not None:
            r = torch.as_strided(fields["res"], Cg.shape, fields["r_bs"] + (fields["ldr"], 1))
            assert torch.equal(_bits(Cg[z]), _bits(r[z])), (cid, "dropped / gated elements must equal res bit for bit")
        else:
            assert bool((Cg[z] == 0).all()), (cid, "dropped / gated elements must be 0")
    if "c_masked" in outs:          # from the C that was written
        k2 = ref["keep2"]
        p2 = fields["c_mask"][0]
        scale = torch.tensor(R.drop_scale(p2), dtype=torch.float32, device=Cg.device)
        want = torch.where(k2 != 0, Cg * scale, torch.zeros_like(Cg))
        assert torch.equal(outs["c_masked"].view(), want), (cid, "c_masked != C * keepscale of the host mask")
        assert abs(float((k2 == 0).double().mean()) - p2) <= 5.0 * (p2 * (1.0 - p2) / k2.numel()) ** 0.5 + 1.0 / k2.numel()
    # ---- the gate, per element, and the suite's global gate behind it
    c = 4.0 * R.R32[fam]
    extra = R.f16x2_extra(fields, ref) if "gemm_x3h_kernel" in name else {}
    kink = ref["kink"]
    report["kink"] = float(kink.double().mean())
    for out, E in (("C", "E_C"), ("pre", "E_pre"), ("c_masked", "E_cm")):
        if out not in outs:
            continue
        got, want = outs[out].view().double(), ref[out]
        tol = R.U24 * (c * ref[E] + (4.0 * extra[out] if extra else 0.0)) + R.U24 * want.abs()
        ratio = torch.where(kink, torch.zeros_like(tol), (got - want).abs() / tol.clamp_min(1e-300))
        worst = float(ratio.max())
        report[out] = worst
        print(f"gate {cid:<44s} {out:<8s} worst |err|/allowed = {worst:.3f}  rel_l2 = {rel_l2(got, want):.2e}  "
              f"kink = {report['kink']:.1e}")
        if not worst <= 1.0:
            at = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
            raise AssertionError((cid, out, "per-element gate", worst, "at [b0, b1, m, n] =", at, float(got[tuple(at)]),
                                  float(want[tuple(at)])))
        assert rel_l2(got, want) < X3_TOL[case["prec"]], (cid, out, rel_l2(got, want))
    if fields.get("a_colsum") is not None:
        got, want = fields["a_colsum"].double(), ref["a_colsum"]
        assert not bool((_bits(fields["a_colsum"]) == R.SENTINEL).any())
        assert rel_l2(got, want) < KTOL, (cid, "a_colsum", rel_l2(got, want))


def _run(H, dev, case, monkeypatch):
    fields, outs, seed, name = _setup(H, dev, case, monkeypatch)
    keep = []
    if case["packed_ahead"]:
        assert "gemm_x3h_kernel" in name
        _pack_ahead(H, monkeypatch, keep)
    _launch(H, dev, fields, case["packed_ahead"])
    torch.cuda.synchronize()
    assert not case["packed_ahead"] or len(keep) == 1
    ref = R.ref_fields(fields, seed)
    report = {}
    _check(case, fields, outs, ref, name, report)
    first = {k: b.flat.clone() for k, b in outs.items()}            # the same call twice: the same bits
    _launch(H, dev, fields, case["packed_ahead"])
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert torch.equal(_bits(b.flat), _bits(first[k])), (case["id"], k, "not bitwise reproducible")
    return report


@pytest.mark.parametrize("cid", _SMALL)
def test_epilogue_matrix(H, gpu_device, monkeypatch, cid):
    _run(H, gpu_device, _BY_ID[cid], monkeypatch)


def _plan(H, case):
    d = H._new_desc()
    d.M, d.N, d.K, d.layout_a, d.layout_b = case["M"], case["N"], case["K"], case["la"], case["lb"]
    d.batch0, d.batch1 = case["batch"]
    d.lda = d.ldb = d.ldc = 4
    d.precision = H.PREC_CODE[case["prec"]]
    bm, bn, sp = C.c_int32(), C.c_int32(), C.c_int32()
    H.check(H.lib().gt_gemm_plan(C.byref(d), C.byref(bm), C.byref(bn), C.byref(sp)), "gt_gemm_plan")
    return bm.value, bn.value, sp.value


@pytest.mark.parametrize("cid", _WIDE)
def test_width_split_for_real(H, gpu_device, monkeypatch, cid):
    """N = 144 / 288: the aligned columns and the remainder are two launches (gt_gemm_desc.hip: width_split), every epilogue
    pointer re-based by hand and the dropout mask re-indexed through drop_ld / n_off -- with the full stack, padded pitches
    and guards.  The precondition of the split is stated from gt_gemm_plan and asserted, so the case cannot quietly turn
    into one launch again."""
    case = _BY_ID[cid]
    if case["cfg"] is not None:
        monkeypatch.setenv("GT_GEMM_CFG", str(case["cfg"]))
    else:
        monkeypatch.delenv("GT_GEMM_CFG", raising=False)
    bm, bn, split = _plan(H, case)
    tiles_m = -(-case["M"] // bm)
    nb = case["batch"][0] * case["batch"][1]
    assert bn == 128 and split == 1 and 1 <= case["N"] % 128 <= 64, (bm, bn, split)
    assert tiles_m * (case["N"] // 128) * nb >= 512, (tiles_m, case["N"] // 128, nb)
    _run(H, gpu_device, case, monkeypatch)


def test_host_mask_is_the_device_mask(H, gpu_device):
    """The host restatement against the standalone device pass, once (the matrix itself never uses gt_dropout_apply)."""
    dev = gpu_device
    H.set_seed(SEED ^ (7 << 40), dev)
    seed = int(H.seed_state(dev).item())
    n = 100003
    for p, salt in ((0.3, 5), (0.05, 0x7FFFFFFF)):
        got = H.dropout_apply(torch.ones(n, device=dev), H.dropout_desc(p, salt, dev))
        torch.cuda.synchronize()
        want = torch.from_numpy(R.drop_mask(seed, salt, p, torch.arange(n).numpy())).float().to(dev)
        assert torch.equal(got, want)


_REFUSALS = {       # feature set, batch, documented code (gt_hip.h / gt_gemm_desc.hip: make_plan, admit)
    "splitk+bias": (dict(bias=1, split_k=3), (1, 1), "GT_ENOTSUP"),
    "splitk+res": (dict(res=1, split_k=3), (1, 1), "GT_ENOTSUP"),
    "c_masked+batch": (dict(cm=0.1), (2, 1), "GT_ENOTSUP"),
    "c_masked+K2": (dict(cm=0.1, K2=8), (1, 1), "GT_ENOTSUP"),
    "silu2+dropout": (dict(act=R.ACT_SILU2, drop=0.2, pre=1), (1, 1), "GT_EINVAL"),
    "rp9": (dict(rp=9), (1, 1), "GT_EINVAL"),
    "K2+a_drop": (dict(K2=8, a_drop=0.2), (1, 1), "GT_ENOTSUP"),
}


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("what", sorted(_REFUSALS))
def test_refusals_leave_the_outputs_alone(H, gpu_device, monkeypatch, what, prec):
    feat, batch, code = _REFUSALS[what]
    monkeypatch.delenv("GT_GEMM_CFG", raising=False)
    case = R._case(f"refuse-{what}-{prec}", "stack", "tile", prec, 131, 200, 64, feat, batch=batch)
    H.set_seed(SEED, gpu_device)
    fields, outs = R.build_case(case, gpu_device)
    with pytest.raises(H.GtError, match=code) as ei:
        _launch(H, gpu_device, fields)
    assert isinstance(ei.value, H.GtNotSupported) == (code == "GT_ENOTSUP")
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert bool((b.bits() == R.SENTINEL).all()), (what, k, "a refused call wrote to an output")
