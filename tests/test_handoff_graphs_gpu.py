"""The masked twins of galerkin_transformer.ops._handoff (the gradient handoff between encoder blocks) on autograd graphs in
which "exactly one consumer, nothing in between" is false.

Every scenario runs three ways on the same seed and parameters: (a) fold on, (b) fold off, (c) a float64 restatement on the
CPU built from oracle/galerkin_oracle.py pieces with the same extra consumers, hooks and cotangents, and with the dropout
masks of run (b) (drawn with gt_dropout_apply over ones for the (p, salt) pairs a spy around _hip.dropout_desc recorded, in
call order).  Bars: (a) == (b) bit for bit -- the twin stands down or fires exactly as in the plain chain; (a) against
float64 at TOL for the output and the input gradient and at max(TOL, 12 x the float32 CPU restatement's own distance from
float64) for parameter and captured gradients.  That a second consumer makes autograd sum into a fresh buffer is a property
of torch, not of the product: these tests are what notices if it stops holding."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from _util import TOL, rel_l2
from oracle import galerkin_oracle as O

pytestmark = pytest.mark.gpu

NOISE_CAP = 7e-5     # see _assert_f64
SEED = 20261020
B = 2


@pytest.fixture(scope="module")
def GT(gpu_device):
    import galerkin_transformer as gt
    from galerkin_transformer import _hip
    _hip.lib()
    return gt


@pytest.fixture(autouse=True)
def _attention_dropout_off(GT):
    GT.set_attention_dropout("off")
    try:
        yield
    finally:
        GT.set_attention_dropout("reference")


@contextlib.contextmanager
def _folds(on):
    from galerkin_transformer import ops
    old = ops._fold_masks[0], ops._gate_fold[0]
    ops._fold_masks[0] = ops._gate_fold[0] = bool(on)
    try:
        yield
    finally:
        ops._fold_masks[0], ops._gate_fold[0] = old


@contextlib.contextmanager
def _spy_dropout(log):
    """Records (p, salt) of every _hip.dropout_desc call with p > 0 while ``spy.on`` (the forward of a run)."""
    from galerkin_transformer import _hip
    orig = _hip.dropout_desc

    def spy(p, salt, device):
        if spy.on and log is not None and p:
            log.append((float(p), int(salt)))
        return orig(p, salt, device)

    spy.on = True
    _hip.dropout_desc = spy
    try:
        yield spy
    finally:
        _hip.dropout_desc = orig


def _rand(k, shape):
    """Tensor number k of the test data (float64, CPU): inputs and cotangents of every leg come from here."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(9000 + k), dtype=torch.float64)


def _randomise(model, seed):
    """Generic parameters: the constructors' small-gain inits would leave whole branches at rounding level."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "fourier_weight" in name:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[0] ** 0.5)
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return model


class _Leg:
    """One run of a scenario: ``x`` the input leaf, ``cot(k, t)`` cotangent k shaped like t, ``tap(i, t)`` (set by the
    scenario) is called on every block / layer output from a module forward hook, ``cap`` what hooks captured."""
    tap = None

    def cot(self, k, t):
        return _rand(100 + k, tuple(t.shape)).to(t)

    def fire(self, i, t):
        if self.tap is not None and t.requires_grad:
            self.tap(i, t)

    def close(self):
        pass


def _tap_hook(L):
    def tap(i, t):
        def hook(g):
            L.cap[f"g{i}"] = g.detach().clone()
            return 2 * g
        t.register_hook(hook)
    L.tap = tap


def _tap_retain(L):
    def tap(i, t):
        t.retain_grad()
        L.kept[f"g{i}"] = t
    L.tap = tap


def _backward(L, loss, leaves, names, twice, spy=None):
    """{name: gradient}; with ``twice`` the first of two backward passes under "1:"."""
    if spy is not None:
        spy.on = False
    res = {}
    for rnd in ((1, 2) if twice else (2,)):
        for t in leaves:
            t.grad = None
        loss.backward(retain_graph=twice and rnd == 1)
        pre = "1:" if rnd == 1 and twice else ""
        for n, t in zip(names, leaves):
            if t.grad is not None:
                res[pre + n] = t.grad.detach().clone()
        for k, t in getattr(L, "kept", {}).items():
            res[pre + "cap:" + k] = t.grad.detach().clone()
            t.grad = None
        for k, g in L.cap.items():
            res[pre + "cap:" + k] = g
        L.cap = {}
    return res


def _assert_equal(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (what, {k: rel_l2(a[k], b[k]) for k in bad})


def _assert_f64(got, r64, r32, what):
    assert sorted(got) == sorted(r64), (what, sorted(set(got) ^ set(r64)))
    errs = {k: rel_l2(got[k], r64[k]) for k in got}
    noise = {k: rel_l2(r32[k], r64[k]) for k in got}
    strict = lambda k: k.split(":")[-1] in ("out", "dx")
    # A gradient that vanishes in exact arithmetic would show here as float32 noise of order one and a bound that asks
    # nothing (it then needs _linear_ref.grad_errors' scaling).  None does at these shapes: the float32 restatement of a sum
    # without cancellation over at most B n f = 12800 terms stays within sqrt(12800) x 6e-8 = 7e-6 of float64; NOISE_CAP
    # leaves an order of magnitude and fails the test if a tensor starts to cancel.
    wn = max(noise, key=noise.get)
    print(f"{what}: largest float32 noise {wn} {noise[wn]:.2e}")
    assert noise[wn] < NOISE_CAP, (what, wn, noise[wn])
    bound = {k: TOL if strict(k) else max(TOL, 12.0 * noise[k]) for k in got}
    worst = max(errs, key=lambda k: errs[k] / bound[k])
    print(f"{what} vs float64: worst {worst} {errs[worst]:.2e} (bound {bound[worst]:.2e})")
    bad = {k: (errs[k], bound[k]) for k in got if not errs[k] < bound[k]}
    assert not bad, (what, bad)
    return errs


def _check_twice(res, what):
    for k in [k for k in res if k.startswith("1:")]:
        assert torch.equal(res[k], res[k[2:]]), (what, k)


# ===================================================================================== encoder stack: masked twins
ENC = dict(generic=dict(d=64, f=128, n=50, act="silu"), relu=dict(d=64, f=128, n=50, act="relu"),
           ln=dict(d=64, f=128, n=50, act="silu", ln=True), fused=dict(d=128, f=256, n=8211, act="relu"))
P_RES, P_FFN = 0.1, 0.05
_enc_cache = {}


def _enc_layers(GT, dev, key):
    if key not in _enc_cache:
        c = ENC[key]
        torch.manual_seed(3)
        layers = [_randomise(GT.SimpleTransformerEncoderLayer(
            d_model=c["d"], n_head=2, pos_dim=2, dim_feedforward=c["f"], attention_type="galerkin",
            layer_norm=bool(c.get("ln")), activation_type=c["act"], dropout=P_RES, ffn_dropout=P_FFN), 40 + i).to(dev).train()
            for i in range(3)]
        _enc_cache[key] = layers
    return _enc_cache[key]


class _EncDevice(_Leg):
    def __init__(self, layers, cfg, dev, x_grad=True):
        self.layers, self.cap, self.kept = layers, {}, {}
        shape = (B, cfg["n"], cfg["d"])
        self.x = _rand(0, shape).float().to(dev).requires_grad_(x_grad)
        self.other = _rand(1, shape).float().to(dev).requires_grad_(x_grad)
        self.pos = torch.rand(B, cfg["n"], 2, generator=torch.Generator().manual_seed(5)).to(dev)
        self.handles = [m.register_forward_hook(lambda mod, args, out, i=i: self.fire(i, out))
                        for i, m in enumerate(layers)]
        self.names = [f"dW:{i}.{n}" for i, m in enumerate(layers) for n, _ in m.named_parameters()]
        self.params = [p for m in layers for p in m.parameters()]

    def block(self, i, t):
        return self.layers[i](t, self.pos)

    def close(self):
        for h in self.handles:
            h.remove()


class _EncOracle(_Leg):
    """Blocks restated from the oracle's pieces with the recorded masks:  x1 = x + m1 . att(x);  x2 = x1 + m2 . ff(x1)  with
    the hidden mask inside ff; layer norms behind either when the stack has them."""

    def __init__(self, layers, cfg, masks, dtype, x_grad=True):
        self.cfg, self.cap, self.kept, self.dtype = cfg, {}, {}, dtype
        shape = (B, cfg["n"], cfg["d"])
        self.x = _rand(0, shape).float().to(dtype).requires_grad_(x_grad)
        self.other = _rand(1, shape).float().to(dtype).requires_grad_(x_grad)
        self.pos = torch.rand(B, cfg["n"], 2, generator=torch.Generator().manual_seed(5)).to(dtype)
        self.sds = [{n: p.detach().cpu().to(dtype).requires_grad_() for n, p in m.named_parameters()} for m in layers]
        self.names = [f"dW:{i}.{n}" for i, sd in enumerate(self.sds) for n in sd]
        self.params = [p for sd in self.sds for p in sd.values()]
        self.masks = iter(masks)

    def block(self, i, t):
        sd, ln, d = self.sds[i], bool(self.cfg.get("ln")), self.cfg["d"]
        m1, mh, m2 = (next(self.masks).to(self.dtype) for _ in range(3))
        att, _ = O.simple_attention(O._sub(sd, "attn."), t, self.pos, n_head=2, attention_type="galerkin", norm=not ln,
                                    eps=1e-5)
        t = t + m1.view(t.shape) * att
        if ln:
            t = F.layer_norm(t, (d,), sd["layer_norm1.weight"], sd["layer_norm1.bias"], 1e-5)
        h = F.silu(F.linear(t, sd["ff.lr1.weight"], sd["ff.lr1.bias"]))
        h = h * mh.view(h.shape)
        t = t + m2.view(t.shape) * F.linear(h, sd["ff.lr2.weight"], sd["ff.lr2.bias"])
        if ln:
            t = F.layer_norm(t, (d,), sd["layer_norm2.weight"], sd["layer_norm2.bias"], 1e-5)
        if torch.is_grad_enabled():
            self.fire(i, t)
        return t


# the scenarios (numbers: the issue's list).  Each returns (output to compare, loss)
def _e_plain(L):                                   # 1
    out = L.block(1, L.block(0, L.x))
    return out, (L.cot(0, out) * out).sum()


def _e_aux(L):                                     # 2: a loss on the tensor between the blocks
    x1 = L.block(0, L.x)
    out = L.block(1, x1)
    return out, (L.cot(0, out) * out).sum() + (L.cot(1, x1) * x1).sum()


def _e_auxhook(L):                                 # 2, the other order: a module forward hook on block 0 uses its output in
    terms = []                                     # an auxiliary loss BEFORE block 1 runs, so block 1's dx reaches autograd's

    def tap(i, t):                                 # buffer for d(x1) first -- the gradient a sum in place would land in
        if i == 0:
            terms.append((L.cot(1, t) * t).sum())
    L.tap = tap
    out = L.block(1, L.block(0, L.x))
    return out, (L.cot(0, out) * out).sum() + terms[0]


def _e_latent(L):                                  # 2, as return_latent collects them: every block output, .contiguous()
    lat, t = [], L.x
    for i in range(3):
        t = L.block(i, t)
        lat.append(t.contiguous())
    assert lat[-1] is t
    return t, sum((L.cot(i, v) * v).sum() for i, v in enumerate(lat))


def _e_fan(L):                                     # 4: one intermediate, two following blocks, results summed
    x1 = L.block(0, L.x)
    out = L.block(1, x1) + L.block(2, x1)
    return out, (L.cot(0, out) * out).sum()


def _e_hook(L):                                    # 5a: a tensor hook that returns a new gradient
    _tap_hook(L)
    return _e_plain(L)


def _e_retain(L):                                  # 5b
    _tap_retain(L)
    return _e_plain(L)


def _e_mul1(L):                                    # 6: a torch op between producer and consumer
    out = L.block(1, L.block(0, L.x) * 1.0)
    return out, (L.cot(0, out) * out).sum()


def _e_nograd(L):                                  # 7: a no_grad forward on other data between forward and backward
    out, loss = _e_plain(L)
    with torch.no_grad():
        L.block(1, L.block(0, L.other.detach()))
    return out, loss


def _e_two(L):                                     # 8: two forwards, one backward through both
    out = L.block(1, L.block(0, L.x))
    out2 = L.block(1, L.block(0, L.other))
    return out, (L.cot(0, out) * out).sum() + (L.cot(2, out2) * out2).sum()


def _enc_run(L, scen, twice=False, spy=None):
    out, loss = scen(L)
    leaves = [t for t in (L.x, L.other) if t.requires_grad] + L.params
    names = ["dx", "other:dx"][:len(leaves) - len(L.params)] + L.names
    res = _backward(L, loss, leaves, names, twice, spy)
    res["out"] = out.detach().clone()
    L.close()
    return res


def _enc_device(GT, dev, key, scen, fold, log=None, twice=False, x_grad=True):
    from galerkin_transformer import _hip
    layers, cfg = _enc_layers(GT, dev, key), ENC[key]
    _hip.set_seed(SEED, dev)
    with _folds(fold), _spy_dropout(log) as spy, _hip.Profile() as prof:
        res = _enc_run(_EncDevice(layers, cfg, dev, x_grad), scen, twice, spy)
    torch.cuda.synchronize()
    calls = {k: v["calls"] for k, v in prof.table().items()}
    return {k: v.cpu() for k, v in res.items()}, calls


def _enc_masks(dev, key, log):
    """The masks of a run, in call order: per block (residual of the attention, hidden, residual of the FeedForward)."""
    from galerkin_transformer import _hip
    cfg = ENC[key]
    assert len(log) % 3 == 0 and [p for p, _ in log[:3]] == [P_RES, P_FFN, P_RES], log[:6]
    _hip.set_seed(SEED, dev)
    T = B * cfg["n"]
    masks = []
    for i, (p, salt) in enumerate(log):
        width = cfg["f"] if i % 3 == 1 else cfg["d"]
        m = _hip.dropout_apply(torch.ones(T, width, device=dev), _hip.dropout_desc(p, salt, dev)).cpu()
        assert bool(torch.all((m == 0) | ((m * (1.0 - p) - 1.0).abs() < 1e-6))) and 0 < float((m == 0).float().mean()) < 3 * p
        masks.append(m)
    return masks


def _enc_three(GT, dev, key, scen, what, twice=False, x_grad=True, f64=True):
    log = []
    b, calls_b = _enc_device(GT, dev, key, scen, False, log, twice, x_grad)
    a, calls_a = _enc_device(GT, dev, key, scen, True, None, twice, x_grad)
    _assert_equal(a, b, what)                    # the twin stands down, or fires exactly as in the plain chain
    if twice:
        _check_twice(a, what)
    if f64:
        masks = _enc_masks(dev, key, log)
        r64 = _enc_run(_EncOracle(_enc_layers(GT, dev, key), ENC[key], masks, torch.float64, x_grad), scen, twice)
        r32 = _enc_run(_EncOracle(_enc_layers(GT, dev, key), ENC[key], masks, torch.float32, x_grad), scen, twice)
        _assert_f64(a, r64, r32, what)
    return calls_a, calls_b


def _drops(calls):
    return calls.get("gt_dropout_apply", 0)


@pytest.mark.parametrize("key", ("generic", "relu", "fused"))
def test_encoder_plain_chain_folds_and_matches(GT, gpu_device, key):
    """Scenario 1, and the sanity of every encoder scenario at that shape: in the plain chain the twins fire (fewer
    gt_dropout_apply launches with the fold on).  'relu' and 'fused' (gt_ffn_bwd writes the twin; T = 16422 = 256 x 64 + 38
    rows) compare with the unfolded run only."""
    from galerkin_transformer import _hip
    cfg = ENC[key]
    if key == "fused":
        assert _hip.ffn_fwd_supported(B * cfg["n"], cfg["d"], cfg["f"], _hip.ACT_RELU)
    else:
        assert not _hip.ffn_fwd_supported(B * cfg["n"], cfg["d"], cfg["f"], _hip.ACT_CODE[cfg["act"]])
    ca, cb = _enc_three(GT, gpu_device, key, _e_plain, f"enc {key} plain", f64=key == "generic")
    assert _drops(cb) - _drops(ca) == 3, (ca, cb)       # attention 0 <- ff 0 <- attention 1 <- ff 1
    if key == "fused":
        assert ca.get("gt_ffn_bwd", 0) == 2, ca


ENC_SCENARIOS = dict(aux=_e_aux, auxhook=_e_auxhook, latent=_e_latent, fan=_e_fan, hook=_e_hook, retain=_e_retain, mul1=_e_mul1, nograd=_e_nograd, two=_e_two)


@pytest.mark.parametrize("name", sorted(ENC_SCENARIOS))
def test_encoder_graphs_generic_route(GT, gpu_device, name):
    """Scenarios 2, 4, 5, 6, 7, 8 on the generic route against the unfolded run and float64.  Where the intermediate has a
    second consumer, a hook that replaces its gradient or an op behind it, the twin of block 0's output stands down (two
    launches saved, inside the layers, instead of the plain chain's three); a hook that only reads, or a forward elsewhere,
    changes nothing."""
    ca, cb = _enc_three(GT, gpu_device, "generic", ENC_SCENARIOS[name], f"enc generic {name}")
    saved = dict(aux=2, auxhook=2, hook=2, mul1=2, retain=3, nograd=3, two=6, fan=None, latent=None)[name]
    if saved is not None:
        assert _drops(cb) - _drops(ca) == saved, (name, ca, cb)


@pytest.mark.parametrize("name", ("aux", "auxhook", "hook", "fan"))
def test_encoder_graphs_fused_ffn_route(GT, gpu_device, name):
    """The same where gt_ffn_bwd writes the twin: against the unfolded run."""
    _enc_three(GT, gpu_device, "fused", ENC_SCENARIOS[name], f"enc fused {name}", f64=False)


def test_encoder_backward_twice(GT, gpu_device):
    """Scenario 3: both passes give the same gradients as each other, as the unfolded run and as float64."""
    _enc_three(GT, gpu_device, "generic", _e_plain, "enc twice", twice=True)
    _enc_three(GT, gpu_device, "generic", _e_aux, "enc aux twice", twice=True)


def test_encoder_layer_norm_stack(GT, gpu_device):
    """Scenario 6, second half: layer norms between the blocks (no tensor passes from one block straight to the next)."""
    ca, cb = _enc_three(GT, gpu_device, "ln", _e_plain, "enc layer_norm")
    assert _drops(ca) == _drops(cb) > 0, (ca, cb)       # every block's output goes through a norm first: no twin anywhere
    _enc_three(GT, gpu_device, "ln", _e_aux, "enc layer_norm aux")


def test_encoder_input_without_gradient(GT, gpu_device):
    """Scenario 9 (requires_grad=True is every other test)."""
    ca, cb = _enc_three(GT, gpu_device, "generic", _e_plain, "enc x no grad", x_grad=False)
    assert _drops(cb) - _drops(ca) == 3, (ca, cb)
    _enc_three(GT, gpu_device, "generic", _e_aux, "enc x no grad aux", x_grad=False)


def test_simple_transformer_return_latent(GT, gpu_device):
    """Scenario 2 with the latents a model hands out: SimpleTransformer(return_latent=True) returns the very tensors that sit
    between its blocks (x.contiguous() of a contiguous tensor), and a loss on them makes each a two-consumer tensor.
    Against the unfolded run; the float64 leg of this graph is the 'latent' scenario above.  Sanity: with a loss on the
    prediction alone the twins fire in this model."""
    from _util import Golden
    from galerkin_transformer import _hip
    dev = gpu_device
    cfg = dict(Golden("model_burgers_small").meta["config"])
    cfg.update(n_hidden=64, n_head=2, dim_feedforward=128, layer_norm=False, attn_norm=True, encoder_dropout=P_RES,
               ffn_dropout=P_FFN, dropout=0.0, decoder_dropout=0.0, decoder_type="pointwise", return_latent=True)
    torch.manual_seed(8)
    model = _randomise(GT.SimpleTransformer(**cfg), 70).to(dev).train()
    n = 50
    node = _rand(30, (B, n, 1)).float().to(dev).requires_grad_()
    pos = torch.linspace(0, 1, n)[None, :, None].repeat(B, 1, 1).to(dev)
    params = list(model.parameters())

    def run(fold, latents):
        _hip.set_seed(SEED, dev)
        with _folds(fold), _hip.Profile() as prof:
            res = model(node, None, pos)
            lat = res["preds_latent"]
            assert len(lat) == 3 and all(v.requires_grad for v in lat)
            loss = (_rand(31, tuple(res["preds"].shape)).float().to(dev) * res["preds"]).sum()
            if latents:
                loss = loss + sum((_rand(32 + i, tuple(v.shape)).float().to(dev) * v).sum() for i, v in enumerate(lat))
            grads = [g.clone() for g in torch.autograd.grad(loss, [node] + params)]
        torch.cuda.synchronize()
        return grads, prof.table().get("gt_dropout_apply", {}).get("calls", 0)

    (_, da), (_, db) = run(True, False), run(False, False)
    assert db - da == 3, (da, db)
    (a, da), (b, db) = run(True, True), run(False, True)
    assert db - da == 2, (da, db)                        # the twin between the layers stands down, those inside them fire
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _capture(step, reseed):
    """eager result and the result of a captured step after two replays (test_softmax_attention_gpu's recipe)."""
    reseed()
    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    reseed()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    return eager, captured


def test_encoder_second_consumer_under_graph_capture(GT, gpu_device):
    from galerkin_transformer import _hip
    dev = gpu_device
    layers, cfg = _enc_layers(GT, dev, "generic"), ENC["generic"]
    L = _EncDevice(layers, cfg, dev)
    L.close()
    cots = [_rand(100 + k, (B, cfg["n"], cfg["d"])).float().to(dev) for k in range(2)]

    def step():
        x1 = L.block(0, L.x)
        first = (cots[1] * x1).sum()                     # one auxiliary consumer before block 1, one after it
        out = L.block(1, x1)
        loss = (cots[0] * out).sum() + first + (cots[0] * x1).sum()
        return torch.autograd.grad(loss, [L.x] + L.params[:len(list(layers[0].parameters())) * 2])

    with _folds(True):
        eager, captured = _capture(step, lambda: _hip.set_seed(SEED, dev))
    for u, v in zip(eager, captured):
        assert torch.equal(u, v)
