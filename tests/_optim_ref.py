"""Reference of the optimizer step (csrc/gt_optim.hip, optim.FlatClipAdam): clip_grad_norm_ + torch.optim.Adam restated in a
dozen lines of plain torch on the CPU, in the dtype the caller asks for; the per-element metrics; and the cases that
test_optim_ref_cpu.py (the float32 envelope) and test_optim_kernels_gpu.py (the kernels) share.

The float64 evaluation is the reference; the float32 evaluation of the same lines is the yardstick of the kernel tests.

Hyper-parameters.  The C ABI takes gscale, max_norm, beta1, beta2, eps and weight_decay as `float`, and lr / beta1_dev are
float32 device scalars, so the operation the kernel is asked for is Adam at those float32 VALUES (0.999f is 0.99899995...):
`hyper()` rounds every one of them through float32 once, and both evaluations of the restatement take the rounded values
as Python floats.  Otherwise 1 - 0.999f = 1.00005e-3 against 1 - 0.999 would show up as a 4.7e-5 error of `v` that no
float32 implementation behind this ABI could avoid.
"""
import math

import torch

BETA1, BETA2, EPS, LR = 0.9, 0.999, 1e-8, 3e-3
BETA1_DEV = 0.85          # differs from BETA1: where beta1_dev is given, the device value must win
CAP = 0.05                # the float32 envelope every case must stay inside (a condition on the data)
NORM_LINKS = 32           # longest chain of roundings of gt_grad_sqnorm at any size used here (see norm_bar)

# 1..1029: one block, tails 0..3, a partial wave; 1 048 575: last element of the norm kernel's first trip, tail 3;
# 1 048 582: one f32x4 in its second trip, tail 2; N_BIG: second trip of both kernels with partial blocks, tail 3;
# N_DARCY: the bucket of the Darcy model (2 220 829 parameters, every tensor padded to a multiple of four)
N_BIG, N_DARCY = 2_097_152 + 5 * 1024 + 3, 2_220_832
SIZES = (1, 2, 3, 4, 5, 7, 1023, 1029, 1_048_575, 1_048_582, N_BIG, N_DARCY)


def f32r(x: float) -> float:
    """x rounded to float32, as a Python float: the value a `float` argument or a float32 device scalar carries."""
    return float(torch.tensor(float(x), dtype=torch.float32).item())


def hyper(**kw):
    return {k: (f32r(v) if isinstance(v, float) else v) for k, v in kw.items()}


def adam_clip_step(p, g, m, v, *, t, lr, beta1, beta2, eps, wd, max_norm, gscale, dtype):
    """One step in `dtype` on copies: (p, m, v, ghat, sq).  `t` is the step count AFTER the increment (1 for the first)."""
    p, g, m, v = (x.detach().to("cpu", dtype).clone() for x in (p, g, m, v))
    sq = gscale ** 2 * (g * g).sum()
    coef = gscale * (min(1.0, max_norm / (math.sqrt(float(sq)) + 1e-6)) if max_norm > 0 else 1.0)
    ghat = coef * g + wd * p
    m = beta1 * m + (1 - beta1) * ghat
    v = beta2 * v + (1 - beta2) * ghat * ghat
    p = p - lr / (1 - beta1 ** t) * m / (v.sqrt() / math.sqrt(1 - beta2 ** t) + eps)
    return p, m, v, ghat, sq


def run_steps(p, grads, m, v, steps, *, dtype, beta2=BETA2, eps=EPS, wd, max_norm, gscale):
    """steps: one dict(t, lr, beta1) per gradient.  Returns (p, m, v, ghat of the last step) in `dtype`."""
    ghat = None
    for g, s in zip(grads, steps):
        p, m, v, ghat, _ = adam_clip_step(p, g, m, v, t=s["t"], lr=s["lr"], beta1=s["beta1"], beta2=beta2, eps=eps,
                                          wd=wd, max_norm=max_norm, gscale=gscale, dtype=dtype)
    return p, m, v, ghat


def step_errors(p, m, v, ref, *, lr, beta1, beta2=BETA2):
    """(err_p, err_m, err_v) of a result against ref = (p64, m64, v64, ghat64); lr and beta1 are the last step's.  The
    absolute floors (one update; one step's share of the moments) keep the elements whose effective gradient nearly
    cancels against wd * p from deciding the metric."""
    p64, m64, v64, gh = (x.double().cpu() for x in ref)
    rms = float(gh.pow(2).mean().sqrt())
    d = lambda a, b, floor: float(((a.detach().double().cpu() - b).abs() / (b.abs() + floor)).max())
    return d(p, p64, lr), d(m, m64, (1 - beta1) * rms), d(v, v64, (1 - beta2) * rms * rms)


def cancellation(p_old, ghat, m_old, p_new, m_new, *, beta1, wd):
    """By how much the worst element of one step cancels: sum of |terms| over |result| for the effective gradient
    (coef g + wd p) and the first moment, and the first moment's figure times |update| / |p_new| for the parameter.  Two
    correctly rounded evaluations of the step in different operation orders agree only to this factor times their
    rounding (the second moment is a sum of non-negative terms and inherits the gradient's figure)."""
    terms = (ghat - wd * p_old).abs() + wd * p_old.abs()
    k_g = terms / ghat.abs()
    k_m = (beta1 * m_old.abs() + (1 - beta1) * terms) / m_new.abs()
    k_p = k_m * (p_new - p_old).abs() / p_new.abs()
    return max(float(k_g.max()), float(k_m.max()), float(k_p.max()))


def norm_bar() -> float:
    """Relative bar of gt_grad_sqnorm against scale^2 * sum g^2 in float64, derived: every term is non-negative, and the
    longest chain of roundings for any size in SIZES has fewer than 32 links (at most 3 fused multiply-adds per thread,
    the tail, the 4-way, wave and block combines of both kernels, 4 partials per thread in the final kernel, and the two
    multiplications by scale), each of relative size 2^-24 at the most."""
    return NORM_LINKS * 2.0 ** -24


# ----------------------------------------------------------------------------------------------- data and cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gradient(n, seed, scale=1.0):
    """float32 [n] ~ scale * N(0, 1); the last seven elements are +-2 rms, so that a skipped tail cannot hide in a small
    gradient."""
    g = torch.randn(n, generator=_gen(seed))
    k = min(7, n)
    g[n - k:] = 2.0 * torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0])[7 - k:]
    return g * scale


def params(n, seed=1):
    return torch.randn(n, generator=_gen(seed))


def moments(n, seed=2):
    """Non-zero starting moments: m ~ 0.1 N(0, 1), v = m'^2 + 1e-4 (positive)."""
    g = _gen(seed)
    return 0.1 * torch.randn(n, generator=g), (0.1 * torch.randn(n, generator=g)) ** 2 + 1e-4


class Case:
    """One run of gt_adam_clip_step: n elements, starting state and one (gradient, t, lr, beta1) per step."""

    def __init__(self, name, n, *, t0=0, scales=(1.0,), wd=0.0, max_norm=0.0, gscale=1.0, beta1_dev=None, zero=False,
                 lrs=None, seed=0, draws=1):
        self.name, self.n, self.zero, self.seed, self.scales, self.draws = name, n, zero, seed, scales, draws
        self.beta1_dev = None if beta1_dev is None else [f32r(b) for b in beta1_dev]
        lrs = lrs or [LR] * len(scales)
        self.h = hyper(wd=float(wd), max_norm=float(max_norm), gscale=float(gscale))
        self.beta1_arg = f32r(BETA1)
        self.steps = [dict(t=t0 + i + 1, lr=f32r(lrs[i]), beta1=self.beta1_dev[i] if self.beta1_dev else self.beta1_arg)
                      for i in range(len(scales))]

    def data(self, k=0):
        """(p, [g per step], m, v) of draw k in float32 on the CPU; deterministic.  Every draw after the first scales its
        gradients by a factor of its own in [0.5, 2): at n <= 7 all elements are the +-2 rms of the tail, and only the
        scale tells two draws apart."""
        n, seed = self.n, self.seed + 1000 * k
        jitter = 1.0 if k == 0 else 0.5 + 1.5 * float(torch.rand(1, generator=_gen(seed)))
        m, v = (torch.zeros(n), torch.zeros(n)) if self.zero else moments(n, 2 + seed)
        return params(n, 1 + seed), [gradient(n, 10 + seed + i, s * jitter) for i, s in enumerate(self.scales)], m, v

    def worst(self, results):
        """Per-metric maximum over the draws: results yields one (err_p, err_m, err_v) per draw."""
        return tuple(max(col) for col in zip(*results))

    def reference(self, p, grads, m, v, dtype):
        return run_steps(p, grads, m, v, self.steps, dtype=dtype, beta2=f32r(BETA2), eps=f32r(EPS), **self.h)

    def errors(self, p, m, v, ref):
        return step_errors(p, m, v, ref, lr=self.steps[-1]["lr"], beta1=self.steps[-1]["beta1"], beta2=f32r(BETA2))

    def __repr__(self):
        return self.name


SMALL_DRAWS = 256


def zero_case(n):
    """One step from zero moments, wd = 0, clipped at 0.99: the case every tail and grid-stride size runs.  A maximum over
    fewer than a thousand elements is one roll of the rounding dice, not a yardstick (n = 4: err_m = 1.7e-9 for one draw,
    a thirtieth of an ulp), so the sizes up to 7 run SMALL_DRAWS independent draws and the metrics are maxima over all."""
    return Case(f"zero-n{n}", n, zero=True, max_norm=0.99, draws=SMALL_DRAWS if n < 1000 else 1)


# at N_BIG: clipping inactive / active / off (sqnorm = NULL), wd 0 and 1e-2, beta1_dev given and NULL, t = 1, 2, 1000, 10^6
BIG_CASES = (
    Case("t1-noclip", N_BIG, t0=0, max_norm=1e9),
    Case("t2-clip-half-wd-b1dev", N_BIG, t0=1, max_norm=0.05, gscale=0.5, wd=1e-2, beta1_dev=[BETA1_DEV]),
    Case("t2-clip-b1dev", N_BIG, t0=1, max_norm=0.05, beta1_dev=[BETA1_DEV]),
    Case("t1000-nonorm-wd", N_BIG, t0=999, max_norm=0.0, wd=1e-2),
    Case("t1e6-two-steps-wd-b1dev", N_BIG, t0=10 ** 6 - 1, scales=(1e-6, 1e4), max_norm=0.0, wd=1e-2,
         beta1_dev=[BETA1_DEV, 0.95]),
)
# the clipped three-step case from zero moments, lr and beta1 moving as under OneCycleLR: also what the graph test replays
THREE_STEP = Case("clip3-zero-wd", N_BIG, zero=True, scales=(1.0, 3.0, 0.1), max_norm=0.05, gscale=0.5, wd=1e-2,
                  beta1_dev=[0.95, BETA1_DEV, 0.9], lrs=[1.2e-4, 3e-3, 1.7e-3])

ALL_CASES = tuple(zero_case(n) for n in SIZES) + BIG_CASES + (THREE_STEP,)

# ----------------------------------------------------------------------------------------------- FlatClipAdam
FLAT_SHAPES = ((1448, 1448), (1,), (3,), (5, 7), (129,), (64, 64))      # 2 100 968 elements, bucket 2 100 976 (> 2 097 152)
FLAT = dict(lr=3e-3, wd=1e-2, max_norm=0.99, total_steps=8, n_steps=3, none_step=1, none_param=4)


def flat_data():
    """(initial tensors, [gradients per step]); the gradient of parameter `none_param` is None on step `none_step`."""
    g = _gen(5)
    init = [torch.randn(*s, generator=g) for s in FLAT_SHAPES]
    grads = [[torch.randn(*s, generator=g) * (3.0 if it % 2 else 0.1) for s in FLAT_SHAPES] for it in range(FLAT["n_steps"])]
    grads[FLAT["none_step"]][FLAT["none_param"]] = None
    return init, grads


def flat_reference(init, grads, sched, dtype):
    """The restatement over the concatenated tensors (a missing gradient is a zero gradient).  sched: (lr, beta1) per step,
    as OneCycleLR set them.  Returns per-tensor lists (p, m, v, ghat) and the last step's squared norm."""
    cat = lambda ts, like: torch.cat([(torch.zeros_like(l) if t is None else t).reshape(-1) for t, l in zip(ts, like)])
    p = cat(init, init)
    m, v, ghat, sq = torch.zeros_like(p), torch.zeros_like(p), None, None
    for t, (gr, (lr, b1)) in enumerate(zip(grads, sched), 1):
        p, m, v, ghat, sq = adam_clip_step(p, cat(gr, init), m, v, t=t, lr=f32r(lr), beta1=f32r(b1), beta2=f32r(BETA2),
                                           eps=f32r(EPS), wd=f32r(FLAT["wd"]), max_norm=f32r(FLAT["max_norm"]),
                                           gscale=1.0, dtype=dtype)
    split = lambda x: list(torch.split(x, [i.numel() for i in init]))
    return split(p), split(m), split(v), split(ghat), float(sq)
