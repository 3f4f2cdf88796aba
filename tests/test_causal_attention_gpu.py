"""Causal linear attention on the GPU: the gt_causal_attn_* kernels through the binding, SimpleAttention('causal') (self and
(x, mem, mem)), ops.causal_linear_attention and GalerkinTransformerDecoderLayer, forward and backward against the float64
restatement of tests/_causal_ref.py.

Input condition: every parity case asserts, in float64, sum_d |(z_i[d] + eps) q_i[d]| / |den_i| <= 2 for all i
(_causal_ref.condition; positive Q', K' give exactly 1) before anything is compared.

Bar, per tensor, with err(t) = max |t - float64| / max |float64|: err(HIP) <= 8 err(float32 torch), the yardstick being
the float32 run on the CPU (torch, autograd) of the reference's arithmetic.  The reference function keeps running states
S_i, z_i, as the kernels do, and its backward cancels S_i g_i against c_i z_i; the tril closed form cancels per matrix entry
first and rounds less in exactly the tensors that are sums of such terms (the Q-path gradients behind a LayerNorm).  The
reference does not exist where these tests run, so its float32 run is made by the scan restatement
(_causal_ref.causal_ref_scan, held to the reference function's recorded float32 results by test_causal_attention_cpu), and
the yardstick is the larger of the two restatements' float32 errors.  The margin covers the different association of the
chunked prefix sums and the MFMA accumulation order.  A tensor whose float64 value is identically zero must be exactly zero.

Measured on MI355X (the figures the tests print): worst ratio err(HIP) / err(float32 torch), largest err(HIP), largest
err(float32 torch) per group
    kernels           out 1.37, 1.9e-07, 3.7e-07;  dq / dk 1.61 (n = 1, a cancelled quantity: 1.8e+01 against 4.8e+01);
                      dv 2.53, 5.9e-07, 9.2e-07
    operator          1.09, 7.8e-07, 1.3e-06
    SimpleAttention   out 1.30, 6.3e-07, 6.5e-07;  Q / K path gradients 3.87, 5.5e-03, 5.0e-03 (d norm_K bias);
                      other gradients 2.75, 2.6e-05, 1.7e-05
    decoder layer     out 1.00, 6.3e-07, 1.3e-06;  gradients 2.74, 6.4e-03, 8.8e-03 (d norm_K bias)
Against the tril form's float32 error alone the kernel-level ratios stay below 4.2, but the Q-path gradients of
SimpleAttention with norm=True (d linears.0, d norm_Q bias, d x of the cross call) reach 15 to 29: 1.4e-05 to 3.1e-05 against
1e-06, in the default and in the f32 GEMM arithmetic alike, where the scan form in float32 has 1.1e-05 to 3.7e-05."""
import pytest
import torch

from _causal_ref import (causal_grads, causal_yardstick, condition, decoder_layer_ref, err, ref_and_yardstick,
                         simple_attention_ref)

pytestmark = pytest.mark.gpu

MARGIN = 8.0
EPS = 1e-7
REAL = {16: 16, 20: 17, 64: 64, 100: 97}      # head tile width -> real columns of the kernel-level cases (pad columns: 20, 100)


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


def _check(what, names, got, ref64, yard):
    """The bar of the module docstring for every named tensor (yard: its float32 torch error); prints each figure before
    asserting."""
    bad = {}
    for k in names:
        r = ref64[k]
        if float(r.abs().max()) == 0.0:
            print(f"{what} {k}: identically zero")
            if float(got[k].abs().max()) != 0.0:
                bad[k] = "not exactly zero"
            continue
        e_hip, e_ref = err(got[k], r), yard[k]
        print(f"{what} {k}: hip {e_hip:.2e}  float32 torch {e_ref:.2e}  ratio {e_hip / max(e_ref, 1e-300):.2f}")
        if not e_hip <= MARGIN * e_ref:
            bad[k] = (e_hip, e_ref)
    assert not bad, (what, bad)


def _masks(B, n, gen):
    """None, and a mask with the leading keys and the last key dropped (n = 1: its only key)."""
    m = torch.rand(B, n, generator=gen) > 0.25
    m[:, :2] = False
    if n > 3:
        m[:, 2] = True
    m[:, -1] = False
    return (None, m)


def _tiles(t, DP):
    """[B, h, n, D] -> token-major head tiles [B*n, h, DP] with zero pad columns."""
    B, h, n, D = t.shape
    out = torch.zeros(B, n, h, DP)
    out[..., :D] = t.permute(0, 2, 1, 3)
    return out.reshape(B * n, h, DP)


def _untile(t, B, n, D):
    return t.reshape(B, n, t.shape[1], t.shape[2])[..., :D].permute(0, 2, 1, 3)


@pytest.mark.parametrize("BH", [(1, 1), (2, 3)])
@pytest.mark.parametrize("DP", [16, 20, 64, 100])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 257])
def test_kernels_match_float64(GT, gpu_device, n, DP, BH):
    from galerkin_transformer import _hip as H
    (B, h), D, dev = BH, REAL[DP], gpu_device
    gen = torch.Generator().manual_seed(1000 * n + 10 * DP + B)
    for kv_mask in _masks(B, n, gen):
        q, k = (torch.rand(B, h, n, D, generator=gen) + 0.5 for _ in range(2))
        v, cot = (torch.randn(B, h, n, D, generator=gen) for _ in range(2))
        assert condition(q.double(), k.double(), kv_mask) <= 2
        names = ("out", "dq", "dk", "dv")
        ref64 = dict(zip(names, causal_grads(q, k, v, kv_mask, cot, torch.float64)))
        ref32 = causal_yardstick(q, k, v, kv_mask, cot, ref64)
        Q, K, V, dO = (_tiles(t, DP).to(dev) for t in (q, k, v, cot))
        keep = None if kv_mask is None else kv_mask.to(dev).view(torch.uint8)

        def run():
            O, den, states = H.causal_attn_fwd(Q, K, V, keep, B, n, h, DP, EPS)
            dQ, dK, dV = H.causal_attn_bwd(dO, O, Q, K, V, keep, den, states, B, n, h, DP, D, EPS)
            return O, dQ, dK, dV, den
        first, second = run(), run()
        torch.cuda.synchronize()
        for a, b in zip(first, second):
            assert torch.equal(a, b)                                   # no atomics: bit-identical reruns
        O, dQ, dK, dV, den = first
        for t in (dQ, dK, dV):
            assert float(t[..., D:].abs().sum()) == 0.0                # pad columns stay exactly zero
        assert float(O[..., D:].abs().sum()) == 0.0
        got = dict(zip(names, (_untile(t, B, n, D) for t in (O, dQ, dK, dV))))
        if kv_mask is not None:
            drop = (~kv_mask)[:, None, :, None].expand(B, h, n, D)
            assert float(got["dk"].cpu()[drop].abs().sum()) == 0.0 and float(got["dv"].cpu()[drop].abs().sum()) == 0.0
            assert float(got["out"][:, :, :2].abs().sum()) == 0.0      # no kept key yet: rows exactly 0
        _check(f"kernel n={n} DP={DP} BH={B * h} mask={kv_mask is not None}", names, got, ref64, ref32)


def test_operator_matches_float64(GT, gpu_device):
    """ops.causal_linear_attention on [B, h, n, D] with D no multiple of 4 (pad columns made by the operator)."""
    dev, (B, h, n, D) = gpu_device, (2, 2, 130, 33)
    gen = torch.Generator().manual_seed(5)
    q, k = (torch.rand(B, h, n, D, generator=gen) + 0.5 for _ in range(2))
    v, cot = (torch.randn(B, h, n, D, generator=gen) for _ in range(2))
    names = ("out", "dq", "dk", "dv")
    for kv_mask in _masks(B, n, gen):
        assert condition(q.double(), k.double(), kv_mask) <= 2
        ref64 = dict(zip(names, causal_grads(q, k, v, kv_mask, cot, torch.float64)))
        ref32 = causal_yardstick(q, k, v, kv_mask, cot, ref64)
        qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
        k0 = kg.detach().clone()
        out, w = GT.ops.causal_linear_attention(qg, kg, vg, None if kv_mask is None else kv_mask.to(dev))
        assert w is None and torch.equal(kg.detach(), k0)              # the key is not written
        grads = torch.autograd.grad(out, (qg, kg, vg), cot.to(dev))
        _check(f"op mask={kv_mask is not None}", names, dict(zip(names, (out.detach(),) + grads)), ref64, ref32)


def _positive_attention(GT, pos_dim, norm, gen):
    """SimpleAttention('causal'), d_model 64, 2 heads, with Q', K' > 0: diagonal-dominant positive projections of positive
    inputs (norm=False) or the LayerNorm affine gamma = 0.25, beta = 2 (|LayerNorm| <= sqrt(d_k - 1) < 8)."""
    attn = GT.SimpleAttention(n_head=2, d_model=64, pos_dim=pos_dim, attention_type="causal", norm=norm, eps=1e-5)
    with torch.no_grad():
        for i, lin in enumerate(attn.linears):
            lin.weight.copy_(0.5 * torch.eye(64) + 0.01 * torch.rand(64, 64, generator=gen))
            lin.bias.copy_(0.1 * torch.rand(64, generator=gen))
            if i == 2:
                lin.weight.add_(0.1 * torch.randn(64, 64, generator=gen))
        if norm:
            for m in list(attn.norm_Q) + list(attn.norm_K):
                m.weight.fill_(0.25)
                m.bias.fill_(2.0)
        attn.fc.weight.copy_(0.2 * torch.randn(attn.fc.weight.shape, generator=gen))
        attn.fc.bias.copy_(0.1 * torch.randn(64, generator=gen))
    return attn


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("cross", [False, True])
def test_simple_attention_matches_float64(GT, gpu_device, cross, with_pos, norm):
    dev, (B, n) = gpu_device, (2, 130)
    gen = torch.Generator().manual_seed(17 + 4 * cross + 2 * with_pos + norm)
    attn = _positive_attention(GT, 1, norm, gen)
    sd = {k: v.detach().clone() for k, v in attn.state_dict().items()}
    x, mem = torch.rand(B, n, 64, generator=gen) + 0.5, torch.rand(B, n, 64, generator=gen) + 0.5
    pos = torch.rand(B, n, 1, generator=gen) if with_pos else None
    cot = torch.randn(B, n, 64, generator=gen)
    attn = attn.to(dev)
    for kv_mask in _masks(B, n, gen):
        probe = []

        def fn(p, x, mem=None, form="tril"):
            kv = x if mem is None else mem
            return simple_attention_ref(p, "", x, kv, kv, n_head=2, attention_type="causal", norm=norm, eps=1e-5,
                                        pos=None if pos is None else pos.to(x.dtype), mask=kv_mask, probe=probe, form=form)
        inputs = dict(x=x, mem=mem) if cross else dict(x=x)
        names, ref64, ref32 = ref_and_yardstick(fn, sd, inputs, cot)
        assert condition(probe[0][0], probe[0][1], kv_mask) <= 2 and probe[0][0].dtype == torch.float64
        assert ("d:fc.weight" in names) == with_pos and ("d:norm_Q.0.weight" in names) == norm
        ins = {k: v.to(dev).requires_grad_(True) for k, v in inputs.items()}
        kv = ins["mem"] if cross else ins["x"]
        mk = None if kv_mask is None else kv_mask.to(dev)
        out, w = attn(ins["x"], kv, kv, pos=None if pos is None else pos.to(dev), mask=mk)
        assert w is None and attn.attn_weight is None
        params = dict(attn.named_parameters())
        leaves = [("d:" + k, ins[k]) for k in ins] + [("d:" + k, params[k]) for k in params if "d:" + k in names]
        grads = torch.autograd.grad(out, [t for _, t in leaves], cot.to(dev))
        got = {"out": out.detach()}
        got.update({k: g for (k, _), g in zip(leaves, grads)})
        _check(f"attn cross={cross} pos={with_pos} norm={norm} mask={kv_mask is not None}", names, got, ref64, ref32)


def _decoder(GT, layer_norm, gen):
    """d_model 64, 2 heads, attn_norm with gamma = 0.25, beta = 2 on the causal block's Q, K: Q', K' > 0 whatever the sign of
    the layer-normed stream."""
    dec = GT.GalerkinTransformerDecoderLayer(64, 2, dim_feedforward=128, layer_norm=layer_norm, attn_norm=True)
    with torch.no_grad():
        for p in dec.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
        for m in list(dec.multihead_attn.norm_Q) + list(dec.multihead_attn.norm_K):
            m.weight.fill_(0.25)
            m.bias.fill_(2.0)
    return dec.eval()


def _decoder_case(GT, dev, layer_norm, masked):
    B, n = 2, 65
    gen = torch.Generator().manual_seed(31 + 2 * layer_norm + masked)
    dec = _decoder(GT, layer_norm, gen)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    x, mem = torch.rand(B, n, 64, generator=gen) + 0.5, torch.rand(B, n, 64, generator=gen) + 0.5
    cot = torch.randn(B, n, 64, generator=gen)
    kv_mask = _masks(B, n, gen)[1] if masked else None
    return dec.to(dev), sd, x, mem, cot, kv_mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layer_norm", [True, False])
def test_decoder_layer_matches_float64(GT, gpu_device, layer_norm, masked):
    dev = gpu_device
    dec, sd, x, mem, cot, kv_mask = _decoder_case(GT, dev, layer_norm, masked)
    probe = []

    def fn(p, x, mem, form="tril"):
        return decoder_layer_ref(p, x, mem, nhead=2, layer_norm=layer_norm, attn_norm=True, memory_mask=kv_mask, probe=probe,
                                 form=form)
    names, ref64, ref32 = ref_and_yardstick(fn, sd, dict(x=x, mem=mem), cot)
    assert condition(probe[0][0], probe[0][1], kv_mask) <= 2 and probe[0][0].dtype == torch.float64
    unused = set("d:" + k for k in sd) - set(names)
    assert all(k.split(":")[1].split(".")[0] in ("linear2",) or ".fc." in k for k in unused), unused
    xg, mg = x.to(dev).requires_grad_(True), mem.to(dev).requires_grad_(True)
    GT.set_attention_dropout("off")          # the galerkin self-attention block; the causal block draws none in any mode
    try:
        out = dec(xg, mg, memory_mask=None if kv_mask is None else kv_mask.to(dev))
        params = dict(dec.named_parameters())
        leaves = [("d:x", xg), ("d:mem", mg)] + [("d:" + k, params[k]) for k in params if "d:" + k in names]
        grads = torch.autograd.grad(out, [t for _, t in leaves], cot.to(dev))
    finally:
        GT.set_attention_dropout("reference")
    got = {"out": out.detach()}
    got.update({k: g for (k, _), g in zip(leaves, grads)})
    _check(f"decoder layer_norm={layer_norm} masked={masked}", names, got, ref64, ref32)


def test_causal_block_ignores_the_dropout_mode(GT, gpu_device):
    dev = gpu_device
    attn = _positive_attention(GT, 1, False, torch.Generator().manual_seed(3)).to(dev)
    x = torch.rand(2, 70, 64, device=dev) + 0.5
    outs = []
    for mode in ("reference", "off", "replay"):          # 'replay' with an empty queue would raise if it were consulted
        GT.set_attention_dropout(mode)
        try:
            outs.append(attn(x, x, x)[0])
        finally:
            GT.set_attention_dropout("reference")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_decoder_graph_capture_replays_eager(GT, gpu_device):
    dev = gpu_device
    dec, sd, x, mem, cot, kv_mask = _decoder_case(GT, dev, True, True)
    xg, mg = x.to(dev).requires_grad_(True), mem.to(dev).requires_grad_(True)
    cot, mk = cot.to(dev), kv_mask.to(dev)
    params = [p for k, p in dec.named_parameters() if not k.startswith("linear2") and ".fc." not in k]
    GT.set_attention_dropout("off")
    try:
        def step():
            return torch.autograd.grad(dec(xg, mg, memory_mask=mk), [xg, mg] + params, cot)
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
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
    finally:
        GT.set_attention_dropout("reference")
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
