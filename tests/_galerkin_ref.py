"""The Galerkin core's contract (include/gt_hip.h: gt_galerkin_ktv[_affine], gt_galerkin_finalize_fwd/bwd, gt_galerkin_dkv,
gt_galerkin_dkv_ln[_plain]) once, in float64, and the case list of the per-element matrix.

    ktv       slab q [b,h] = [pos | K']^T [pos | V'] over the tokens [q chunk, min(n, (q+1) chunk)), chunk = round4(ceil(n/S))
    finalize  M = mul .* (sum of slabs) / n_tokens on the leading Dr x Dr block, P = M W_h^T;  dM = mul .* (dP_h W_h) / n_tokens,
              dWfc[b] = dP_h^T M
    dkv       dK' = V' dM^T, dV' = K' dM;  dkv_ln: the per-head LayerNorm backward on their value columns

Plain torch index arithmetic, no operator of this project.  Every function takes `dtype`: with torch.float32 it is the float32
restatement (chains in index order, one rounded multiply and one rounded add per term) the per-element gate is calibrated
with.  Next to the values each returns the ENVELOPE E: the same formula with every operand replaced by its absolute value and
every cancellation by a sum of absolute values -- the magnitude one float32 rounding of any intermediate is relative to.

`mut` names a deliberate mistake (tests/test_galerkin_ref_cpu.py: the gate has to reject each of them); None is the contract.

`CASES` is the one case list: tests/test_galerkin_ref_cpu.py calibrates the gate on it, tests/test_galerkin_core_gpu.py runs
it on the device.  `build_case` makes a case's operands from a seed on the CPU (the GPU module moves them over)."""
import numpy as np
import torch

from _gemm_ref import U24, drop_mask

GATE = 4.0          # the device may accumulate in another order than index order: 4 x the float32 restatement's own error
# Largest normalised error of the float32 restatement per family, max |ref32 - ref64| / (2^-24 E) over the family's cases,
# as tests/test_galerkin_ref_cpu.py prints it (it holds each entry to what it measures).
R32 = {"ktv": 7.7, "fin_fwd": 4.7, "fin_bwd": 5.3, "dkv": 5.0, "dkv_ln": 2.7}


def round4(x):
    return (x + 3) // 4 * 4


def chunk_len(n, n_slabs):
    return round4(-(-n // n_slabs))


def chunks(n, n_slabs):
    """[(lo, hi)] per slab; an empty chunk has lo >= hi."""
    c = chunk_len(n, n_slabs)
    return [(q * c, min(n, (q + 1) * c)) for q in range(n_slabs)]


def ktv_staged(Kt, Vt, h, dk, p):
    """The launcher's own predicate (csrc/gt_galerkin.hip: gt_galerkin_ktv_affine): the LDS-staged kernel or the streaming one."""
    return h <= 4 and h * round4(dk + p) <= 256 and Kt.data_ptr() % 16 == 0 and Vt.data_ptr() % 16 == 0


def _chain(terms, n, like):
    """sum_{k<n} terms(k) in index order (one rounded add per term in float32)."""
    acc = torch.zeros_like(like)
    for k in range(n):
        acc = acc + terms(k)
    return acc


def _mm(a, b):
    """a [..., m, k] @ b [..., k, n]; in float32 a chain over k in index order."""
    if a.dtype != torch.float32:
        return a @ b
    acc = torch.zeros(torch.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]), dtype=a.dtype)
    for k in range(a.shape[-1]):
        acc = acc + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return acc


# ---------------------------------------------------------------------------------------------- K^T V slabs
def ktv_ref(Kt, Vt, B, n, h, dk, p, n_slabs, gamma=None, beta=None, dtype=torch.float64, mut=None):
    """Head tiles Kt, Vt [B n, h, DP] = [pos(p) | values(dk) | pad] -> (slabs, E) [n_slabs, B, h, DP, DP]."""
    DP, Dr = round4(dk + p), dk + p
    K4, V4 = Kt.reshape(B, n, h, DP).to(dtype), Vt.reshape(B, n, h, DP).to(dtype)
    pos = K4[..., :p]                                  # both operands carry the K tile's coordinates
    kv, vv = K4[..., p:Dr], V4[..., p:Dr]
    ke, ve = kv.abs(), vv.abs()
    if gamma is not None:
        g, bt = gamma.to(dtype), beta.to(dtype)
        gk, gv = (g[1], g[0]) if mut == "swap_gamma" else (g[0], g[1])
        ke, ve = gk.abs() * ke + bt[0].abs(), gv.abs() * ve + bt[1].abs()
        kv, vv = gk * kv + bt[0], gv * vv + bt[1]
    L, R = torch.cat([pos, kv], -1), torch.cat([pos, vv], -1)
    if mut == "v_pos":                                 # V's coordinates under K'^T P
        R = torch.cat([V4[..., :p], vv], -1)
    Le, Re = torch.cat([pos.abs(), ke], -1), torch.cat([pos.abs(), ve], -1)
    out = torch.zeros(n_slabs, B, h, DP, DP, dtype=dtype)
    E = torch.zeros(n_slabs, B, h, DP, DP, dtype=torch.float64)
    for q, (lo, hi) in enumerate(chunks(n, n_slabs)):
        toks = list(range(lo, hi))
        if mut == "overlap" and lo < hi < n:
            toks.append(hi)
        if mut == "drop_last" and toks and toks[-1] == n - 1:
            toks.pop()
        acc = torch.zeros(B, h, Dr, Dr, dtype=dtype)
        for t in toks:
            acc = acc + L[:, t, :, :, None] * R[:, t, :, None, :]
        out[q, :, :, :Dr, :Dr] = acc
        if lo < hi:
            E[q, :, :, :Dr, :Dr] = torch.einsum("bthi,bthj->bhij", Le[:, lo:hi].double(), Re[:, lo:hi].double())
    if mut == "slab_hb":                               # slab q written at (q, h, b)
        out = out.transpose(1, 2).contiguous().reshape(n_slabs, B, h, DP, DP)
    return out, E


# ---------------------------------------------------------------------------------------------- finalize
def fin_mul(B, h, DP, mask=None, drop=None, mut=None):
    """The multiplier behind 1/n_tokens, float64 [B, h, DP, DP]: ones, the explicit tensor, or the stateless mask of
    (seed, salt, p) at index ((b h + hh) DP + j) DP + c."""
    if mask is not None:
        return mask.double()
    if drop is None:
        return torch.ones(B, h, DP, DP, dtype=torch.float64)
    seed, salt, p = drop
    bh = np.arange(B * h, dtype=np.int64).reshape(B, h, 1, 1)
    j, c = np.arange(DP, dtype=np.int64).reshape(1, 1, DP, 1), np.arange(DP, dtype=np.int64).reshape(1, 1, 1, DP)
    if mut == "drop_jc":
        j, c = c, j
    return torch.from_numpy(drop_mask(seed, salt, p, (bh * DP + j) * DP + c))


def finalize_ref(slabs, Wfc, dPt, Mt_in, B, h, DP, Dr, d, pos_dim, n_tokens, mul, dtype=torch.float64, mut=None, n_alt=None):
    """slabs [S, B, h, DP, DP] (a view of any slab stride), Wfc [d, h Dr], dPt [B, d, h DP], Mt_in [B, h, DP, DP] (the
    backward's saved M), mul = fin_mul(...).  -> dict of (value, E): Mt, P [B, h DP, d], Pv [B, h (Dr - pos_dim), d],
    dM [B, h, DP, DP], dW [B, d, h Dr] (one slab per sample)."""
    S = slabs.shape[0]
    sl = slabs.to(dtype)
    ks = [k for k in range(S) if not (mut == "skip_slab" and k == S - 3)]
    s = _chain(lambda i: sl[ks[i]], len(ks), sl[0])
    se = slabs.double().abs().sum(0)
    inv = 1.0 / (n_alt if mut == "inv_n" else n_tokens)
    m = (mul * inv).to(dtype)
    live = torch.zeros(DP, DP, dtype=torch.bool)
    live[:Dr, :Dr] = True
    Mt = torch.where(live, s * m, torch.zeros_like(s))
    Mte = torch.where(live, se * m.double().abs(), torch.zeros_like(se))
    W = Wfc.to(dtype).reshape(d, h, Dr).permute(1, 2, 0)                   # [h, Dr, d]
    P = torch.zeros(B, h, DP, d, dtype=dtype)
    Pe = torch.zeros(B, h, DP, d, dtype=torch.float64)
    P[:, :, :Dr] = _mm(Mt[:, :, :Dr, :Dr], W[None])
    Pe[:, :, :Dr] = Mte[:, :, :Dr, :Dr] @ W[None].double().abs()
    dv = Dr - pos_dim
    out = {"Mt": (Mt, Mte), "P": (P.reshape(B, h * DP, d), Pe.reshape(B, h * DP, d)),
           "Pv": (P[:, :, pos_dim:Dr].reshape(B, h * dv, d), Pe[:, :, pos_dim:Dr].reshape(B, h * dv, d))}
    # backward: dP_h[j][c] = dPt[b][c][hh DP + j]
    dP = dPt.to(dtype).reshape(B, d, h, DP).permute(0, 2, 3, 1)            # [B, h, DP, d]
    Wt = W.transpose(1, 2)                                                 # [h, d, Dr]
    g = _mm(dP[:, :, :Dr], Wt[None])                                       # [B, h, Dr, Dr]
    ge = dP[:, :, :Dr].double().abs() @ Wt[None].double().abs()
    dM = torch.zeros(B, h, DP, DP, dtype=dtype)
    dMe = torch.zeros(B, h, DP, DP, dtype=torch.float64)
    dM[:, :, :Dr, :Dr] = g * m[:, :, :Dr, :Dr]
    dMe[:, :, :Dr, :Dr] = ge * m[:, :, :Dr, :Dr].double().abs()
    Mi = Mt_in.to(dtype)
    dW = _mm(dP[:, :, :Dr].transpose(2, 3), Mi[:, :, :Dr, :Dr])            # [B, h, d, Dr]
    dWe = dP[:, :, :Dr].transpose(2, 3).double().abs() @ Mi[:, :, :Dr, :Dr].double().abs()
    out["dM"] = (dM, dMe)
    out["dW"] = (dW.permute(0, 2, 1, 3).reshape(B, d, h * Dr), dWe.permute(0, 2, 1, 3).reshape(B, d, h * Dr))
    return out


# ---------------------------------------------------------------------------------------------- dK', dV'
def dkv_ref(Kt, Vt, dM, B, n, h, DP, dtype=torch.float64, mut=None):
    """dK'[t] = V'[t] dM^T, dV'[t] = K'[t] dM on whole tile rows -> {"dK": (v, E), "dV": (v, E)} [B n, h, DP]."""
    K4 = Kt.reshape(B, n, h, DP).to(dtype).transpose(1, 2)                 # [B, h, n, DP]
    V4 = Vt.reshape(B, n, h, DP).to(dtype).transpose(1, 2)
    D = dM.to(dtype)
    if mut == "dM_T":
        D = D.transpose(2, 3)
    back = lambda x: x.transpose(1, 2).reshape(B * n, h, DP)
    return {"dK": (back(_mm(V4, D.transpose(2, 3))), back(V4.double().abs() @ D.double().abs().transpose(2, 3))),
            "dV": (back(_mm(K4, D)), back(K4.double().abs() @ D.double().abs()))}


def head_stats(qkv, h, dk, eps):
    """[2, T, h, 2] = (mean, rstd) of the K and V head rows of qkv [T, 3 h dk], in float64, rounded to float32 once."""
    T = qkv.shape[0]
    x = qkv.double().reshape(T, 3, h, dk)[:, 1:].transpose(0, 1)            # [2, T, h, dk]
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return torch.cat([mu, rstd], -1).float().contiguous()


def dkv_ln_ref(Kt, Vt, dM, qkv, gamma, beta, stats, B, n, h, dk, p, dtype=torch.float64, mut=None):
    """The K and V blocks of d_qkv and dgamma, dbeta [2, h, dk].  beta=None: affine tiles (K', V' as stored; xh from qkv and
    stats).  beta given: plain tiles (xh as stored; K' = gamma_K xh + beta_K formed here).
    -> {"dx": (v, E) [2, T, h dk], "dgamma": (v, E), "dbeta": (v, E)}."""
    T, DP, Dr = B * n, round4(dk + p), dk + p
    K4, V4 = Kt.reshape(T, h, DP).to(dtype), Vt.reshape(T, h, DP).to(dtype)
    g = gamma.to(dtype)
    st = stats.to(dtype)
    Ke, Ve = K4.double().abs(), V4.double().abs()
    if beta is not None:
        bt = beta.to(dtype)
        xh = torch.stack([K4[..., p:Dr], V4[..., p:Dr]])
        K4, V4 = K4.clone(), V4.clone()
        Ke[..., p:Dr] = g[0].double().abs() * Ke[..., p:Dr] + bt[0].double().abs()
        Ve[..., p:Dr] = g[1].double().abs() * Ve[..., p:Dr] + bt[1].double().abs()
        K4[..., p:Dr] = g[0] * xh[0] + bt[0]
        V4[..., p:Dr] = g[1] * xh[1] + bt[1]
    else:
        x = qkv.to(dtype).reshape(T, 3, h, dk)[:, 1:].transpose(0, 1)
        xh = (x - st[..., 0:1]) * st[..., 1:2]
    D = dM.to(dtype)
    if mut == "dM_T":
        D = D.transpose(2, 3)
    Dabs = D.double().abs()
    shape5 = lambda x: x.reshape(B, n, h, DP).transpose(1, 2)               # [B, h, n, DP]
    back = lambda x: x.transpose(1, 2).reshape(T, h, dk)
    gy = torch.stack([back(_mm(shape5(V4), D.transpose(2, 3)[:, :, :, p:Dr])), back(_mm(shape5(K4), D[:, :, :, p:Dr]))])
    gye = torch.stack([back(shape5(Ve) @ Dabs.transpose(2, 3)[:, :, :, p:Dr]), back(shape5(Ke) @ Dabs[:, :, :, p:Dr])])
    gg, gge = gy * g[:, None], gye * g[:, None].double().abs()             # [2, T, h, dk]
    xa = xh.double().abs()
    inv = 1.0 / dk
    zero = torch.zeros(2, T, h, dtype=dtype)
    m1 = _chain(lambda c: gg[..., c], dk, zero) * inv
    m2 = _chain(lambda c: gg[..., c] * xh[..., c], dk, zero) * inv
    rstd = st[..., 1:2]
    dx = rstd * (gg - m1[..., None] - xh * m2[..., None])
    dxe = rstd.double() * (gge + gge.mean(-1, keepdim=True) + xa * (gge * xa).mean(-1, keepdim=True))
    zg = torch.zeros(2, h, dk, dtype=dtype)
    dg = _chain(lambda t: gy[:, t] * xh[:, t], T, zg)
    db = _chain(lambda t: gy[:, t], T, zg)
    return {"dx": (dx.reshape(2, T, h * dk), dxe.reshape(2, T, h * dk)),
            "dgamma": (dg, (gye * xa).sum(1)), "dbeta": (db, gye.sum(1))}


# ---------------------------------------------------------------------------------------------- the gate
def ratio(got, ref64, E):
    """max |got - ref64| / (2^-24 E) over the elements with E > 0 (0.0 if there are none)."""
    live = E > 0
    if not bool(live.any()):
        return 0.0
    return float(((got.double() - ref64).abs()[live] / (U24 * E[live])).max())


def gate_violation(got, ref64, E, fam):
    """None if `got` passes |got - ref64| <= 4 R32[fam] 2^-24 E per element with exact zeros where E == 0, else a message;
    a NaN anywhere fails."""
    got = got.double()
    if got.shape != ref64.shape:
        return f"shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    if bool(torch.isnan(got).any()):
        return f"{int(torch.isnan(got).sum())} NaN"
    dead = E == 0
    if bool((got[dead] != 0).any()):
        return f"{int((got[dead] != 0).sum())} non-zero where the contract has an exact zero"
    r = ratio(got, ref64, E)
    if not r <= GATE * R32[fam]:
        return f"ratio {r:.3g} > {GATE} x {R32[fam]}"
    return None


# ---------------------------------------------------------------------------------------------- cases
def _ktv(B, n, h, dk, p, S, route, mis=False):
    return dict(fam="ktv", id=f"ktv-{B}x{n}x{h}x{dk}x{p}-s{S}" + ("-mis" if mis else ""), B=B, n=n, h=h, dk=dk, p=p, S=S,
                route=route, mis=mis)


def _fin(B, h, DP, Dr, d, S, p, n_tokens, n_alt):
    return dict(fam="fin", id=f"fin-{B}x{h}x{DP}x{Dr}x{d}-s{S}", B=B, h=h, DP=DP, Dr=Dr, d=d, S=S, p=p, n_tokens=n_tokens,
                n_alt=n_alt)


def _dkv(B, n, h, dk, p):
    return dict(fam="dkv", id=f"dkv-{B}x{n}x{h}x{dk}x{p}", B=B, n=n, h=h, dk=dk, p=p)


CASES = [
    # (B, n, h, dk, p, n_slabs): the LDS-staged kernel ...
    _ktv(1, 1, 1, 16, 0, 1, "staged"), _ktv(1, 17, 2, 16, 1, 1, "staged"), _ktv(2, 130, 4, 32, 2, 3, "staged"),
    _ktv(1, 63, 3, 48, 2, 4, "staged"), _ktv(2, 65, 1, 96, 1, 2, "staged"), _ktv(2, 64, 4, 64, 0, 1, "staged"),
    _ktv(1, 100, 2, 16, 2, 7, "staged"), _ktv(1, 20, 2, 16, 2, 8, "staged"),
    # ... and the streaming one: h > 4, h DP > 256, or tiles off a 16-byte boundary
    _ktv(2, 70, 5, 16, 2, 2, "stream"), _ktv(1, 33, 8, 16, 1, 1, "stream"), _ktv(1, 50, 9, 16, 0, 3, "stream"),
    _ktv(2, 65, 6, 32, 0, 2, "stream"), _ktv(1, 40, 4, 64, 2, 2, "stream"), _ktv(1, 35, 3, 96, 1, 2, "stream"),
    _ktv(2, 130, 2, 32, 2, 3, "stream", mis=True),
    # (B, h, DP, Dr, d, n_slabs), then the coordinate columns, n_tokens and the other sequence's length (mutation "inv_n")
    _fin(2, 4, 36, 34, 128, 3, 2, 777, 771), _fin(1, 1, 100, 97, 96, 1, 1, 131, 129), _fin(3, 2, 52, 50, 192, 5, 2, 777, 770),
    _fin(1, 2, 16, 16, 24, 7, 0, 61, 59), _fin(64, 4, 20, 18, 16, 2, 2, 45, 47), _fin(60, 5, 20, 18, 24, 4, 2, 45, 47),
    _fin(128, 4, 20, 17, 16, 3, 1, 45, 47), _fin(128, 8, 20, 18, 16, 1, 2, 45, 47),
    # (B, n, h, dk, p)
    _dkv(1, 1, 1, 16, 2), _dkv(1, 15, 2, 16, 2), _dkv(2, 16, 4, 32, 2), _dkv(1, 17, 1, 48, 2), _dkv(2, 100, 5, 32, 2),
    _dkv(1, 37, 8, 16, 1), _dkv(2, 50, 4, 36, 0), _dkv(1, 17, 1, 16, 0), _dkv(300, 17, 4, 16, 2),
    # B h = 1 on a head tile the kernels take (DP = 16 of the case before is refused: GT_ENOTSUP, asserted on the device)
    _dkv(1, 17, 1, 16, 2),
]
DKV_DP = (20, 36, 52)       # head tiles gt_galerkin_dkv[_ln] take; others are refused


def _gen(case, salt=0):
    import zlib
    return torch.Generator().manual_seed((zlib.crc32(case["id"].encode()) + 7919 * salt) & 0x7FFFFFFF)


def build_case(case, seed=0, own_v_pos=False):
    """The operands of a case, float32 on the CPU, from (case, seed) alone.
    ktv / dkv:  qkv [T, 3 h dk]; gamma != beta rows for K and V ([2, h, dk], |beta| up to 2); pos in [0, 1); stats of qkv's own
                rows; affine tiles Kt, Vt = [pos | gamma xh + beta | 0] and plain tiles Kx, Vx = [pos | xh | 0], rounded once;
                dM [B, h, DP, DP] (no symmetry), dQp [T, h, DP].  own_v_pos: the V tiles carry coordinates of their own.
    fin:        slabs [S, B, h, DP, DP] (values in the pads too: the kernel must mask them), Wfc, dPt, an explicit mask."""
    g = _gen(case, seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    if case["fam"] == "fin":
        B, h, DP, Dr, d, S = (case[k] for k in ("B", "h", "DP", "Dr", "d", "S"))
        return dict(slabs=rn(S, B, h, DP, DP) * (1.0 + torch.arange(S).reshape(S, 1, 1, 1, 1)), Wfc=0.3 * rn(d, h * Dr),
                    dPt=rn(B, d, h * DP), mask=(torch.rand(B, h, DP, DP, generator=g) > 0.4).float() * 1.75)
    B, n, h, dk, p = (case[k] for k in ("B", "n", "h", "dk", "p"))
    T, DP, Dr, eps = B * n, round4(dk + p), dk + p, 1e-5
    qkv = rn(T, 3 * h * dk) * 1.5 + 0.25
    gamma = 1.0 + 0.5 * rn(2, h, dk)
    gamma[1] = -0.75 * gamma[1] - 0.5
    beta = (torch.rand(2, h, dk, generator=g) * 4.0 - 2.0)
    pos = torch.rand(T, p, generator=g)
    pos_v = torch.rand(T, p, generator=g) if own_v_pos else pos
    stats = head_stats(qkv, h, dk, eps)
    x = qkv.double().reshape(T, 3, h, dk)[:, 1:].transpose(0, 1)
    xh = (x - stats[..., 0:1].double()) * stats[..., 1:2].double()
    y = xh * gamma.double()[:, None] + beta.double()[:, None]
    tiles = []
    for src in (y, xh):
        for s, ps in ((0, pos), (1, pos_v)):
            t = torch.zeros(T, h, DP, dtype=torch.float64)
            t[..., :p] = ps.double()[:, None]
            t[..., p:Dr] = src[s]
            tiles.append(t.float().contiguous())
    return dict(qkv=qkv, gamma=gamma, beta=beta, stats=stats, Kt=tiles[0], Vt=tiles[1], Kx=tiles[2], Vx=tiles[3],
                dM=0.2 * rn(B, h, DP, DP), dQp=rn(T, h, DP))


SEED = 0x1234_5678_9ABC_DEF
DROP_P = 0.5
FIN_MODES = ("none", "mask", "drop")
# (family of R32, variants) per case family
VARIANTS = {"ktv": (("ktv", "affine"), ("ktv", "plain")),
            "fin": tuple(("fin", m) for m in FIN_MODES),
            "dkv": (("dkv", "tiles"), ("dkv_ln", "affine"), ("dkv_ln", "plain"))}


def fin_salt(case):
    import zlib
    return zlib.crc32(case["id"].encode()) & 0x7FFFFFFF


def fin_Mt_in(case, ops, mode):
    """The M the backward of a finalize case is given: the float64 forward's, rounded to float32 once."""
    mul = fin_mul(case["B"], case["h"], case["DP"], ops["mask"] if mode == "mask" else None,
                  (SEED, fin_salt(case), DROP_P) if mode == "drop" else None)
    r = finalize_ref(ops["slabs"], ops["Wfc"], ops["dPt"], torch.zeros_like(mul), case["B"], case["h"], case["DP"], case["Dr"],
                     case["d"], case["p"], case["n_tokens"], mul)
    return r["Mt"][0].float()


def evaluate(case, ops, kind, variant, dtype=torch.float64, mut=None):
    """{output: (value, E)} of one variant of a case -- ("ktv", "affine" | "plain"), ("fin", mode), ("dkv", "tiles"),
    ("dkv_ln", "affine" | "plain") -- with the R32 family of every output under "fam"."""
    if kind == "ktv":
        a = (ops["Kt"], ops["Vt"], None, None) if variant == "affine" else (ops["Kx"], ops["Vx"], ops["gamma"], ops["beta"])
        v, E = ktv_ref(a[0], a[1], case["B"], case["n"], case["h"], case["dk"], case["p"], case["S"], a[2], a[3], dtype, mut)
        return {"slabs": (v, E), "fam": {"slabs": "ktv"}}
    if kind == "fin":
        B, h, DP = case["B"], case["h"], case["DP"]
        mul = fin_mul(B, h, DP, ops["mask"] if variant == "mask" else None,
                      (SEED, fin_salt(case), DROP_P) if variant == "drop" else None, mut)
        r = finalize_ref(ops["slabs"], ops["Wfc"], ops["dPt"], fin_Mt_in(case, ops, variant), B, h, DP, case["Dr"], case["d"],
                         case["p"], case["n_tokens"], mul, dtype, mut, case["n_alt"])
        r["fam"] = {"Mt": "fin_fwd", "P": "fin_fwd", "Pv": "fin_fwd", "dM": "fin_bwd", "dW": "fin_bwd"}
        return r
    B, n, h, dk, p = (case[k] for k in ("B", "n", "h", "dk", "p"))
    if kind == "dkv":
        r = dkv_ref(ops["Kt"], ops["Vt"], ops["dM"], B, n, h, round4(dk + p), dtype, mut)
        r["fam"] = {"dK": "dkv", "dV": "dkv"}
        return r
    a = (ops["Kt"], ops["Vt"], None) if variant == "affine" else (ops["Kx"], ops["Vx"], ops["beta"])
    r = dkv_ln_ref(a[0], a[1], ops["dM"], ops["qkv"], ops["gamma"], a[2], ops["stats"], B, n, h, dk, p, dtype, mut)
    r["fam"] = {"dx": "dkv_ln", "dgamma": "dkv_ln", "dbeta": "dkv_ln"}
    return r
