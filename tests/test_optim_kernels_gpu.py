"""gt_grad_sqnorm and gt_adam_clip_step (csrc/gt_optim.hip) called directly through the C ABI, and optim.FlatClipAdam at the
shipped bucket size, against the float64 restatement of tests/_optim_ref.py -- per element, at the sizes where the vector
loop, the scalar tail and the second grid-stride trip of each kernel begin and end (-m gpu).

Every buffer is 16-byte aligned and carries 8 guard floats behind element n that must come back bit-identical.

Bars.
  Squared norm: 32 * 2^-24 = 1.9e-6 relative against scale^2 * sum g^2 in float64, derived in _optim_ref.norm_bar (every term
  is non-negative, fewer than 32 roundings in the longest chain); two calls give the same bits.  Measured: at most
  9.6e-8 (n = 2 220 832), 1.1e-9 at n <= 7.
  Adam step: err_p, err_m, err_v of _optim_ref.step_errors (per element, against float64) may be 4 x what the float32
  evaluation of the same restatement scores on the same data, computed in the test (the margin of test_batchnorm_gpu.py and
  test_instance_norm_gpu.py: it covers the rounding order of the clip coefficient and of the norm).  Worst measured
  value / allowance over all cases: err_p 2.6e-6 / 1.1e-5 (clip3-zero-wd), err_m 3.8e-7 / 1.9e-6 (t2-clip-half-wd-b1dev),
  err_v 3.6e-7 / 7.7e-7 (zero-n2220832); nearest to its allowance: err_v 2.5e-7 / 4.7e-7 (zero-n1023).  One step from zero
  moments at the twelve sizes: err_p <= 1.7e-7, err_m <= 1.5e-7, err_v <= 3.6e-7 against allowances of 1.9e-7 .. 1.1e-6.
  FlatClipAdam (three steps, bucket of 2 100 976): the same metrics over all tensors; grad_norm() within 16 * 2^-24 of the
  float64 norm (half of the bar for the square).  Measured: err_p 3.3e-6 / 1.5e-5, err_m 7.6e-7 / 3.6e-6, err_v 2.6e-7 /
  1.2e-6, grad_norm 3.2e-8 / 9.5e-7.
  Graph replay against eager calls, the all-zero gradient, the guards and the padding: bit for bit.
"""
import functools

import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -1234.5
EINVAL, EALIGN, EWS = -1, -2, -3
B2, EPS = R.f32r(R.BETA2), R.f32r(R.EPS)


@pytest.fixture(scope="module")
def H(gpu_device):
    from galerkin_transformer import _hip
    _hip.lib()
    return _hip


def call(H, sym, *args):
    """The entry point's return code; tensors go as their device pointers, the stream last.  A launch that is made is a
    record of an open _hip.Profile, a refused one is not."""
    fn = getattr(H.lib(), sym)
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    return H._timed(sym, 0.0, 0.0, lambda: fn(*a, H.stream_ptr()))


def guarded(host, dev):
    """host [n] -> device [n + GUARD] with the sentinel behind element n, on a 16-byte boundary."""
    n = host.numel()
    b = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    b[:n].copy_(host)
    assert b.data_ptr() % 16 == 0
    return b


def guards_intact(*bufs):
    want = torch.full((GUARD,), SENTINEL).view(torch.int32)
    return all(torch.equal(b[-GUARD:].cpu().view(torch.int32), want) for b in bufs)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Scalars:
    """The device scalars of one optimizer: lr, beta1, the step count and the squared norm, and the norm's workspace."""

    def __init__(self, H, dev):
        self.lr, self.beta1 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sq = torch.full((1,), float("nan"), device=dev)
        self.ws = torch.empty(H.lib().gt_grad_sqnorm_ws_bytes(), dtype=torch.uint8, device=dev)


def sqnorm(H, G, n, gscale, out, ws):
    return call(H, "gt_grad_sqnorm", G, n, gscale, out, ws, ws.numel())


def adam(H, case, P, G, M, V, n, s):
    """norm (when clipping) and step of `case` on the buffers, with the scalars s as they stand."""
    if case.h["max_norm"] > 0:
        assert sqnorm(H, G, n, case.h["gscale"], s.sq, s.ws) == 0
    rc = call(H, "gt_adam_clip_step", P, G, M, V, n, s.sq if case.h["max_norm"] > 0 else None, case.h["gscale"],
              case.h["max_norm"], s.lr, case.beta1_arg, B2, EPS, case.h["wd"], s.step, s.beta1 if case.beta1_dev else None)
    assert rc == 0


@functools.lru_cache(maxsize=2)
def three_step_reference():
    p, grads, m, v = R.THREE_STEP.data()
    return (p, grads, m, v), R.THREE_STEP.reference(p, grads, m, v, torch.float32), R.THREE_STEP.reference(p, grads, m, v, torch.float64)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_reference():
    yield
    three_step_reference.cache_clear()          # 150 MB of host memory the rest of the session has no use for


def references(case, k):
    if case is R.THREE_STEP:
        return three_step_reference()
    data = case.data(k)
    return data, case.reference(*data, torch.float32), case.reference(*data, torch.float64)


# ----------------------------------------------------------------------------------------------- squared norm
@pytest.mark.parametrize("n", R.SIZES)
def test_grad_sqnorm_against_float64(H, gpu_device, n):
    """gscale^2 * sum g^2 at gradient scales 1e-6, 1 and 1e4 (the squares stay inside float32) and gscale 1 and 0.5, within
    the derived bar; the same bits from a second call; the guards behind g untouched."""
    dev = gpu_device
    s = Scalars(H, dev)
    out2 = torch.full((1,), float("nan"), device=dev)
    worst = 0.0
    for scale in (1e-6, 1.0, 1e4):
        g = R.gradient(n, 20, scale)
        G = guarded(g, dev)
        sum64 = float(g.double().pow(2).sum())
        for gscale in (1.0, 0.5):
            assert sqnorm(H, G, n, gscale, s.sq, s.ws) == 0 and sqnorm(H, G, n, gscale, out2, s.ws) == 0
            got, again = s.sq.cpu(), out2.cpu()
            want = gscale ** 2 * sum64
            err = abs(float(got.double()) - want) / want
            worst = max(worst, err)
            assert err <= R.norm_bar(), (n, scale, gscale, float(got), want, err)
            assert torch.equal(bits(got), bits(again)), (n, scale, gscale)
        assert guards_intact(G)
    print(f"sqnorm n={n}: worst relative error {worst:.2e} (bar {R.norm_bar():.2e})")


# ----------------------------------------------------------------------------------------------- Adam step
@pytest.mark.parametrize("case", R.ALL_CASES, ids=repr)
def test_adam_clip_step_against_float64(H, gpu_device, case):
    """Every case of _optim_ref.ALL_CASES: the one-step case from zero moments at every tail and grid-stride size, and at
    2 102 275 clipping inactive / active (gscale 0.5) / off with sqnorm = NULL, wd 0 and 1e-2, beta1_dev given (and
    different from the argument) and NULL, t = 1, 2, 1000, 10^6 from non-zero moments, and three clipped steps."""
    dev, n = gpu_device, case.n
    s = Scalars(H, dev)
    got, f32 = [], []
    for k in range(case.draws):
        (p, grads, m, v), r32, r64 = references(case, k)
        P, M, V, G = (guarded(t, dev) for t in (p, m, v, grads[0]))
        for g, st in zip(grads, case.steps):
            G[:n].copy_(g)
            s.lr.fill_(st["lr"]), s.beta1.fill_(st["beta1"]), s.step.fill_(st["t"])
            adam(H, case, P, G, M, V, n, s)
        assert guards_intact(P, M, V, G), (case, k)
        got.append(case.errors(P[:n], M[:n], V[:n], r64))
        f32.append(case.errors(*r32[:3], r64))
    got, allow = case.worst(got), tuple(4 * e for e in case.worst(f32))
    print(f"adam {case.name}: err_p {got[0]:.2e} / {allow[0]:.2e}  err_m {got[1]:.2e} / {allow[1]:.2e}  "
          f"err_v {got[2]:.2e} / {allow[2]:.2e}  (measured / allowance)")
    assert all(a / 4 < R.CAP for a in allow), allow
    assert all(e <= a for e, a in zip(got, allow)), (case, got, allow)


@pytest.mark.parametrize("n", (1029, R.N_BIG))
def test_all_zero_gradient_is_a_fixed_point(H, gpu_device, n):
    """g = 0 with zero moments, clipping and wd = 0: p, m and v come back bit-identical, sqnorm is exactly 0 and nothing is
    NaN -- the clip coefficient is min(1, max_norm / 1e-6), not 0 / 0."""
    dev = gpu_device
    case = R.zero_case(n)
    p = R.params(n)
    z = torch.zeros(n)
    P, M, V, G = (guarded(t, dev) for t in (p, z, z, z))
    s = Scalars(H, dev)
    s.lr.fill_(R.f32r(R.LR)), s.step.fill_(1)
    adam(H, case, P, G, M, V, n, s)
    assert float(s.sq) == 0.0
    for b, t in ((P, p), (M, z), (V, z)):
        assert not torch.isnan(b).any()
        assert torch.equal(bits(b[:n]), bits(t))
    assert guards_intact(P, M, V, G)


# ----------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(H, gpu_device):
    """Null or misaligned operands, n = 0, clipping without a norm, a missing or short workspace: the documented code, no
    launch.  Every other argument is valid device memory, so a missing check would show as a wrong code."""
    dev = gpu_device
    n = 1029
    case = R.zero_case(n)
    big = [torch.zeros(n + 16, device=dev) for _ in range(4)]
    s = Scalars(H, dev)
    s.lr.fill_(R.f32r(R.LR)), s.step.fill_(1), s.sq.fill_(1.0)
    need = H.lib().gt_grad_sqnorm_ws_bytes()
    assert need == 1024 * 4

    def step(bufs=big, n=n, sq=s.sq, max_norm=0.99, lr=s.lr, cnt=s.step):
        return call(H, "gt_adam_clip_step", *bufs, n, sq, 1.0, max_norm, lr, case.beta1_arg, B2, EPS, 0.0, cnt, None)

    def norm(g=big[1], n=n, out=s.sq, ws=s.ws, ws_bytes=need):
        return call(H, "gt_grad_sqnorm", g, n, 1.0, out, ws, ws_bytes)

    refused = []
    for i in range(4):
        refused.append((f"adam null operand {i}", EINVAL, lambda i=i: step(bufs=big[:i] + [None] + big[i + 1:])))
        refused.append((f"adam operand {i} off by one float", EALIGN,
                        lambda i=i: step(bufs=big[:i] + [big[i][1:]] + big[i + 1:])))
    refused += [("adam null lr", EINVAL, lambda: step(lr=None)), ("adam null step", EINVAL, lambda: step(cnt=None)),
                ("adam n = 0", EINVAL, lambda: step(n=0)),
                ("adam max_norm > 0 without sqnorm", EINVAL, lambda: step(sq=None)),
                ("sqnorm null g", EINVAL, lambda: norm(g=None)), ("sqnorm null out", EINVAL, lambda: norm(out=None)),
                ("sqnorm n = 0", EINVAL, lambda: norm(n=0)),
                ("sqnorm g off by one float", EALIGN, lambda: norm(g=big[1][1:])),
                ("sqnorm null workspace", EWS, lambda: norm(ws=None)),
                ("sqnorm workspace one byte short", EWS, lambda: norm(ws_bytes=need - 1))]
    assert len(refused) == 18
    with H.Profile() as prof:
        for what, code, fn in refused:
            assert fn() == code, what
        assert prof.records == []
        assert norm() == 0 and step() == 0 and step(sq=None, max_norm=0.0) == 0        # and the valid calls are launches
        assert [r[0] for r in prof.records] == ["gt_grad_sqnorm", "gt_adam_clip_step", "gt_adam_clip_step"]
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- graph capture
def test_graph_replay_equals_eager(H, gpu_device):
    """gt_seed_advance, gt_grad_sqnorm and gt_adam_clip_step captured once on one stream (a single chain) and replayed three
    times, with the device lr / beta1 scalars and the gradient buffer rewritten in between: bit-identical to three eager
    calls on a twin set of buffers, and within the allowance of the three-step float64 restatement."""
    dev, case = gpu_device, R.THREE_STEP
    n = case.n
    (p, grads, m, v), r32, r64 = three_step_reference()
    gdev = [g.to(dev) for g in grads]

    def fresh():
        return [guarded(t, dev) for t in (p, grads[0], m, v)], Scalars(H, dev)

    def chain(bufs, s):
        assert call(H, "gt_seed_advance", s.step, 1) == 0
        adam(H, case, bufs[0], bufs[1], bufs[2], bufs[3], n, s)

    def load(bufs, s, i):
        bufs[1][:n].copy_(gdev[i])
        s.lr.fill_(case.steps[i]["lr"]), s.beta1.fill_(case.steps[i]["beta1"])

    eb, es = fresh()
    for i in range(3):
        load(eb, es, i)
        chain(eb, es)
    torch.cuda.synchronize()

    gb, gs = fresh()
    load(gb, gs, 0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(gb, gs)
    for i in range(3):
        load(gb, gs, i)
        graph.replay()
    torch.cuda.synchronize()
    assert int(gs.step) == 3 == int(es.step)
    for a, b in zip(gb + [gs.sq], eb + [es.sq]):
        assert torch.equal(bits(a), bits(b))
    assert guards_intact(*gb)
    got, allow = case.errors(gb[0][:n], gb[2][:n], gb[3][:n], r64), tuple(4 * e for e in case.errors(*r32[:3], r64))
    print(f"graph {case.name}: " + "  ".join(f"{e:.2e} / {a:.2e}" for e, a in zip(got, allow)))
    assert all(e <= a for e, a in zip(got, allow)), (got, allow)


# ----------------------------------------------------------------------------------------------- FlatClipAdam
def test_flat_clip_adam_at_the_shipped_bucket_size(gpu_device):
    """optim.FlatClipAdam on a synthetic parameter list (one 1448 x 1448 tensor and five small ones: a bucket of 2 100 976
    with padded slots, past the second trip of both kernels), three steps under OneCycleLR with max_norm 0.99, wd 1e-2 and
    one parameter whose .grad is None on the second step, against the float64 restatement over the concatenated tensors."""
    import galerkin_transformer as gt
    dev = gpu_device
    init, grads = R.flat_data()
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    opt = gt.FlatClipAdam(ps, lr=R.FLAT["lr"], betas=(R.BETA1, R.BETA2), eps=R.EPS, weight_decay=R.FLAT["wd"],
                          max_norm=R.FLAT["max_norm"])
    assert opt.numel == 2_100_976 and opt.numel % 4 == 0
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=R.FLAT["lr"], total_steps=R.FLAT["total_steps"])
    seen = []
    for gr in grads:
        seen.append((opt.param_groups[0]["lr"], opt.param_groups[0]["betas"][0]))
        for q, t in zip(ps, gr):
            q.grad = None if t is None else t.to(dev)
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    assert len({b for _, b in seen}) == 3 and len({l for l, _ in seen}) == 3        # the schedule moved both scalars

    r32, r64 = R.flat_reference(init, grads, seen, torch.float32), R.flat_reference(init, grads, seen, torch.float64)
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])
    kw = dict(lr=R.f32r(seen[-1][0]), beta1=R.f32r(seen[-1][1]), beta2=B2)
    ref = tuple(cat(x) for x in r64[:4])
    got = R.step_errors(cat(ps), cat([opt.state[q]["exp_avg"] for q in ps]), cat([opt.state[q]["exp_avg_sq"] for q in ps]),
                        ref, **kw)
    allow = tuple(4 * e for e in R.step_errors(cat(r32[0]), cat(r32[1]), cat(r32[2]), ref, **kw))
    norm64 = r64[4] ** 0.5
    norm_err = abs(opt.grad_norm() - norm64) / norm64
    print(f"flat: err_p {got[0]:.2e} / {allow[0]:.2e}  err_m {got[1]:.2e} / {allow[1]:.2e}  err_v {got[2]:.2e} / "
          f"{allow[2]:.2e}  (measured / allowance); grad_norm {norm_err:.2e} / {R.norm_bar() / 2:.2e}")
    assert all(a / 4 < R.CAP for a in allow), allow
    assert all(e <= a for e, a in zip(got, allow)), (got, allow)
    assert norm_err <= R.norm_bar() / 2

    pad = torch.ones(opt.numel, dtype=torch.bool)
    for q, o in zip(ps, opt.offsets):
        pad[o:o + q.numel()] = False
    assert int(pad.sum()) == opt.numel - sum(q.numel() for q in ps) == 8
    for name in ("flat_param", "exp_avg", "exp_avg_sq"):
        slots = getattr(opt, name).cpu()[pad]
        assert torch.equal(bits(slots), torch.zeros(8, dtype=torch.int32)), (name, slots)
