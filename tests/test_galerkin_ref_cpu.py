"""Pins tests/_galerkin_ref.py without a GPU, on the very case list tests/test_galerkin_core_gpu.py runs: the yardstick of the
per-element gate (float32 restatement against float64, normalised by the envelope), the gate's teeth (nine deliberate
mistakes applied to the float64 reference, each of which the gate has to reject on every case it applies to), the chunk
partition and the stateless mask at the finalize index."""
import functools

import numpy as np
import pytest
import torch

import _galerkin_ref as R
from _gemm_ref import drop_key, drop_scale, drop_thresh


@functools.lru_cache(maxsize=None)
def _ops(cid, own_v_pos=False):
    return R.build_case(next(c for c in R.CASES if c["id"] == cid), own_v_pos=own_v_pos)


@functools.lru_cache(maxsize=None)
def _ref64(cid, kind, variant, own_v_pos=False):
    case = next(c for c in R.CASES if c["id"] == cid)
    return R.evaluate(case, _ops(cid, own_v_pos), kind, variant)


def _supported(case, kind):
    return kind == "ktv" or case["fam"] != "dkv" or R.round4(case["dk"] + case["p"]) in R.DKV_DP


# ---------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("fam", sorted(R.R32))
def test_float32_yardstick(fam):
    """r32 = max |ref32 - ref64| / (2^-24 E) per case and output: the GPU gate allows 4 x the family's largest (R.R32, which
    this test holds to what it measures)."""
    worst, worst_id = 0.0, None
    for case in R.CASES:
        for kind, variant in R.VARIANTS[case["fam"]]:
            if not _supported(case, kind):
                continue
            r64 = _ref64(case["id"], kind, variant)
            names = [k for k, f in r64["fam"].items() if f == fam]
            if not names:
                continue
            r32 = R.evaluate(case, _ops(case["id"]), kind, variant, dtype=torch.float32)
            for k in names:
                assert r32[k][0].dtype == torch.float32 and r64[k][0].dtype == torch.float64
                assert bool((r32[k][0][r64[k][1] == 0] == 0).all()), (case["id"], k)
                r = R.ratio(r32[k][0], r64[k][0], r64[k][1])
                print(f"r32 {fam:<8s} {case['id']:<28s} {variant:<7s} {k:<7s} {r:.2f}")
                if r > worst:
                    worst, worst_id = r, (case["id"], variant, k)
    print(f"r32 family {fam}: max {worst:.3f} {worst_id}, recorded {R.R32[fam]}")
    assert worst <= R.R32[fam], (fam, worst, worst_id)
    assert worst >= 0.5 * R.R32[fam], "R32 is a record of this measurement, not a free parameter"


# ---------------------------------------------------------------------------------------------- teeth
def _applies(mut, case, kind, variant):
    f = case["fam"]
    if mut == "overlap":
        return kind == "ktv" and any(lo < hi < case["n"] for lo, hi in R.chunks(case["n"], case["S"]))
    if mut == "drop_last":
        return kind == "ktv"
    if mut == "slab_hb":
        return kind == "ktv" and case["B"] > 1 and case["h"] > 1
    if mut == "swap_gamma":
        return kind == "ktv" and variant == "plain"
    if mut == "v_pos":
        return kind == "ktv" and case["p"] > 0
    if mut == "dM_T":
        return f == "dkv" and _supported(case, kind)
    if mut == "drop_jc":
        return f == "fin" and variant == "drop"
    if mut == "inv_n":
        return f == "fin"
    if mut == "skip_slab":
        return f == "fin" and case["S"] == 7
    raise KeyError(mut)


MUTATIONS = {
    "overlap": "the first token past each chunk end counted in that chunk as well",
    "drop_last": "the last token of the sample dropped",
    "slab_hb": "slab q written at (q, h, b) instead of (q, b, h)",
    "swap_gamma": "gamma_K and gamma_V swapped",
    "v_pos": "V's coordinates taken for K^T P",
    "dM_T": "dM transposed in dkv",
    "drop_jc": "the dropout index with j and c swapped",
    "inv_n": "1 / n_tokens replaced by 1 / n",
    "skip_slab": "one of 7 slabs not summed",
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_gate_rejects(mut):
    """The float64 reference with one deliberate mistake is the "got": the gate must refuse it on every case the mistake
    applies to.  Printed: the smallest ratio of the mistake's largest error to the gate, over those cases."""
    own = mut == "v_pos"                     # (the V tiles get coordinates of their own: with shared ones nothing can show)
    smallest, n_cases = float("inf"), 0
    for case in R.CASES:
        for kind, variant in R.VARIANTS[case["fam"]]:
            if not _applies(mut, case, kind, variant):
                continue
            r64 = _ref64(case["id"], kind, variant, own)
            bad = R.evaluate(case, _ops(case["id"], own), kind, variant, mut=mut)
            rejected, margin = False, 0.0
            for k, fam in r64["fam"].items():
                ref, E = r64[k]
                got = bad[k][0]
                if R.gate_violation(got, ref, E, fam) is not None:
                    rejected = True
                dead = E == 0
                margin = max(margin, float("inf") if bool((got[dead] != 0).any())
                             else R.ratio(got, ref, E) / (R.GATE * R.R32[fam]))
            n_cases += 1
            smallest = min(smallest, margin)
            assert rejected, (mut, case["id"], variant, margin)
    print(f"teeth {mut:<10s} ({MUTATIONS[mut]}): {n_cases} cases, smallest error / gate = {smallest:.3g}")
    assert n_cases > 0 and smallest > 1.0


def test_reference_passes_its_own_gate():
    """... and the unmutated reference, rounded to float32, passes (the gate is not simply refusing everything)."""
    for case in R.CASES[::3]:
        for kind, variant in R.VARIANTS[case["fam"]]:
            if not _supported(case, kind):
                continue
            r64 = _ref64(case["id"], kind, variant)
            for k, fam in r64["fam"].items():
                assert R.gate_violation(r64[k][0].float(), r64[k][0], r64[k][1], fam) is None, (case["id"], variant, k)


# ---------------------------------------------------------------------------------------------- sanity
def test_chunks_partition_the_tokens():
    seen = set()
    for case in R.CASES:
        if case["fam"] != "ktv":
            continue
        n, S = case["n"], case["S"]
        seen.add((n, S))
        c = R.chunk_len(n, S)
        assert c % 4 == 0 and c * S >= n and (c - 4) * S < n or c == 4
        toks = [t for lo, hi in R.chunks(n, S) for t in range(lo, hi)]
        assert toks == list(range(n)), (n, S)
    assert (130, 3) in seen and R.chunk_len(130, 3) == 44 and R.chunk_len(100, 7) == 16
    assert R.chunks(100, 7)[-1] == (96, 100)
    assert [hi > lo for lo, hi in R.chunks(20, 8)] == [True] * 5 + [False] * 3


def test_case_list_is_shared_and_covers_every_route():
    import test_galerkin_core_gpu as G
    assert G.R is R
    ids = [c["id"] for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for case in R.CASES:
        if case["fam"] == "ktv" and not case["mis"]:
            staged = case["h"] <= 4 and case["h"] * R.round4(case["dk"] + case["p"]) <= 256
            assert staged == (case["route"] == "staged"), case["id"]
    assert {c["dk"] // 16 for c in R.CASES if c["fam"] == "ktv" and c["route"] == "stream"} == {1, 2, 4, 6}
    # finalize backward: every parts count of the launcher (gt_galerkin_finalize_bwd), both row groupings of the forward
    parts = {max(4 if c["d"] >= 160 else 1, min(4, 1024 // (c["B"] * c["h"]))) for c in R.CASES if c["fam"] == "fin"}
    assert parts == {1, 2, 3, 4}
    assert {c["B"] * c["h"] >= 256 for c in R.CASES if c["fam"] == "fin"} == {True, False}


def test_inputs_are_not_tame():
    ops = _ops("dkv-2x16x4x32x2")
    g, b, dM = ops["gamma"], ops["beta"], ops["dM"]
    assert float((g[0] - g[1]).abs().min()) > 1e-3 and float((b[0] - b[1]).abs().max()) > 1.0
    assert float(b.abs().max()) > 1.5 and float(b.abs().max()) <= 2.0
    assert float((dM - dM.transpose(2, 3)).abs().max()) > 0.1
    assert torch.equal(ops["Kt"][..., :2], ops["Vt"][..., :2]) and 0 <= float(ops["Kt"][..., :2].min()) \
        and float(ops["Kt"][..., :2].max()) < 1
    assert not torch.equal(_ops("dkv-2x16x4x32x2", True)["Vt"][..., :2], ops["Kt"][..., :2])
    assert torch.equal(ops["stats"], R.head_stats(ops["qkv"], 4, 32, 1e-5))


def test_drop_mask_at_the_finalize_index():
    """fin_mul against a per-element evaluation of csrc/gt_common.h's drop_hash, one element at a time."""
    B, h, DP, salt, p = 2, 3, 8, 77, 0.5
    got = R.fin_mul(B, h, DP, drop=(R.SEED, salt, p))
    key, thr = int(drop_key(R.SEED, salt)), int(drop_thresh(p))

    def fmix(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    kept = 0
    for b in range(B):
        for hh in range(h):
            for j in range(DP):
                for c in range(DP):
                    idx = (b * h + hh) * DP * DP + j * DP + c
                    want = drop_scale(p) if fmix((idx * 0x9E3779B1 + key) & 0xFFFFFFFF) >= thr else 0.0
                    assert float(got[b, hh, j, c]) == want, (b, hh, j, c)
                    kept += want != 0
    assert 0.35 < kept / (B * h * DP * DP) < 0.65
    swapped = R.fin_mul(B, h, DP, drop=(R.SEED, salt, p), mut="drop_jc")
    assert torch.equal(swapped, got.transpose(2, 3)) and not torch.equal(swapped, got)
