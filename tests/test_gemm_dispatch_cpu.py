"""The descriptor layer of gt_gemm, pinned down without a GPU: for a fixed list of descriptors the answers of the four pure
host queries -- gt_gemm_plan, gt_gemm_kernel_name, gt_gemm_ws_bytes, gt_gemm_packed_b_bytes -- against the table recorded in
tests/golden/gemm_dispatch.json (which engine, which instance, how much scratch, how big a packed weight).

Pointer fields are plain integers (1 << 20 and up: aligned; + 4: off a 16-byte boundary; + 8: on an 8-byte one), never real
allocations.  This module therefore NEVER calls gt_gemm, gt_gemm_pack_b_many or anything else that launches: the queries
look at the addresses' low bits only and dereference nothing.

    python tests/test_gemm_dispatch_cpu.py --record      # rewrite the table from the library that is built
"""
import ctypes as C
import itertools
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_dispatch.json")

MB = 1 << 20
# one fake address per pointer field (distinct megabytes, all 16-byte aligned)
ADDR = {n: (i + 1) * MB for i, n in enumerate(
    ["A", "B", "C", "A2", "B2", "bias", "res", "add", "pre", "aux", "rp_a", "rp_b", "a_colsum", "c_masked", "b_packed", "w2", "b2",
     "out2", "g2", "dw2", "hn_gamma", "hn_beta", "hn_pos", "hn_out", "hn_stats", "seed"])}
F32, BF16X3, BF16X2, BF16, F16X2 = range(5)
EP_ROWDOT, EP_MLP_BWD, EP_HEADNORM = 1, 2, 3
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def gemm(M, N, K, la=0, lb=0, b0=1, b1=1, **kw):
    """Fields of a dense product (leading dimensions and batch strides of contiguous operands); kw overrides / adds.
    Pointer fields given as True take their fake address, as an int that offset from it; "X.p" sets a dropout's p (and seed)."""
    f = dict(M=M, N=N, K=K, layout_a=la, layout_b=lb, batch0=b0, batch1=b1,
             A=ADDR["A"], B=ADDR["B"], C=ADDR["C"], lda=M if la else K, ldb=N if lb else K, ldc=N)
    if b0 * b1 > 1:
        f.update(a_bs1=M * K, a_bs0=b1 * M * K, b_bs1=N * K, b_bs0=b1 * N * K, c_bs1=M * N, c_bs0=b1 * M * N)
    for k, v in kw.items():
        if k in ADDR and (v is None or isinstance(v, int)) and (v is None or v < MB):     # bool, NULL or an offset
            v = None if v is None or v is False else ADDR[k] + (0 if v is True else v)
        f[k] = v
    return f


def cases():
    """[(id, fields)]: fixed and deterministic.  One block per family of branches of the descriptor layer."""
    out = []

    def add(tag, f):
        out.append((f"{tag}#{len(out)}", f))

    # every precision (and an invalid one) x layout x split_k x batching, over shapes that land on every fp32 configuration,
    # the streamed kernel (K >= 256, aligned), the 32-deep stage (la = lb = 1, K >= 512) and the split-operand engine
    shapes = [(128, 128, 256), (200, 100, 130), (64, 48, 512), (64, 128, 512)]
    for prec, (la, lb), sk, (b0, b1), (M, N, K) in itertools.product([0, 1, 2, 3, 4, 7], LAYOUTS, [0, 1, 4],
                                                                     [(1, 1), (4, 1), (2, 3)], shapes):
        add("grid", gemm(M, N, K, la, lb, b0, b1, split_k=sk, precision=prec))

    # tall-skinny weight gradients: la = lb = 1, split_k 0, K >= 65536, M in {32..128} step 32, even N <= 32, 8-byte operands
    for M, N, off, cs in itertools.product([32, 64, 96, 128, 160], [2, 32, 34, 31], [0, 4, 8], [False, True]):
        add("tsmm", gemm(M, N, 65536, 1, 1, split_k=0, A=off, a_colsum=cs))
    for M in [32, 64, 96, 128]:
        add("tsmm", gemm(M, 16, 100000, 1, 1, split_k=0, precision=F16X2, a_colsum=True))
    add("tsmm", gemm(64, 16, 65532, 1, 1, split_k=0))
    add("tsmm", gemm(64, 16, 65536, 1, 1, split_k=0, lda=65))
    add("tsmm", gemm(64, 16, 65536, 1, 1, split_k=0, bias=True))
    add("tsmm", gemm(64, 16, 65536, 1, 1, split_k=0, b_packed=True))

    # automatic split-K: K >= 512, no epilogue, a small grid (la = lb = 1 on the split engine: whole groups of eight chunks)
    for prec, (la, lb), K, (M, N), extra in itertools.product(
            [F32, BF16X3, F16X2], LAYOUTS, [512, 16384, 200000], [(128, 128), (256, 384), (100, 36)],
            [{}, {"a_colsum": True}, {"bias": True}]):
        add("autosplit", gemm(M, N, K, la, lb, split_k=0, precision=prec, **extra))

    # widths just above a multiple of 128: two launches when the aligned part fills the chip
    for prec, lb, N, M, K, extra in itertools.product(
            [F32, BF16X3, F16X2], [0, 1], [144, 192, 200], [65536, 1024], [128],
            [{}, {"K2": 64, "A2": True, "B2": True, "lda2": 64, "ldb2": 64}, {"bias": True}, {"res": True, "ldr": 272},
             {"c_masked": True, "ldc_masked": 272}, {"b_packed": True}, {"rp": 2, "rp_a": True, "rp_b": True, "rp_lda": 2, "rp_ldb": 2}]):
        f = gemm(M, N, K, 0, lb, precision=prec, **extra)
        if "K2" in f and lb:
            f["ldb2"] = N
        add("width", f)
    for prec, N, M, K, sk in itertools.product([F32, BF16X3, F16X2], [144, 192], [256, 96], [65536, 4096], [0, 8]):
        add("width-ksplit", gemm(M, N, K, 1, 1, split_k=sk, precision=prec))
        add("width-ksplit", gemm(M, N, K, 1, 1, b0=16, split_k=sk, precision=prec))

    # QKV projection with the head-norm epilogue (48-wide heads run in 64-column slots)
    hn = dict(ep_mode=EP_HEADNORM, hn_out=True, hn_gamma=True, hn_beta=True, hn_stats=True, hn_pos=True, bias=True, hn_norm_mask=3,
              hn_eps=1e-5)
    for prec, dk, h, M, K, p, extra in itertools.product([F32, BF16X3, F16X2], [16, 32, 48, 64, 24], [4], [16384, 4096],
                                                         [128], [0, 2],
                                                         [{}, {"b_packed": True}, {"C": None, "hn_skip_raw_mask": 7, "hn_plain": 1}]):
        add("headnorm", gemm(M, 3 * h * dk, K, precision=prec, hn_h=h, hn_dk=dk, hn_p=p, **hn, **extra))

    # fused two-layer head: whole rows in one block
    for prec, ep, N, no, M, K in itertools.product([F32, F16X2], [EP_ROWDOT, EP_MLP_BWD], [32, 64, 100, 128, 160], [1, 4],
                                                   [1000], [32, 128]):
        add("head", gemm(M, N, K, precision=prec, ep_mode=ep, n_out=no, w2=True, ldw2=N, b2=True, out2=True, g2=True, dw2=True,
                         bias=True, act=1))

    # implicit 3x3 convolution, forward / data gradient: channel counts, narrow and wide outputs, pixel pitches below and above cv_c
    for prec, c, N, (b, h, w), pitch, extra in itertools.product(
            [0, 1, 2, 4], [16, 64, 8], [32, 64, 96], [(4, 32, 32), (1, 16, 16), (16, 64, 64)], [0, 16, 2],
            [{}, {"b_packed": True}]):
        if extra and prec != F16X2:
            continue
        lda = {0: 0, 16: c + 16, 2: c + 2}[pitch]
        add("conv", gemm(b * h * w, N, 9 * c, precision=prec, cv_h=h, cv_w=w, cv_c=c, lda=lda, **extra))

    # ... and its weight gradient: nine taps as the batch, the library cuts K
    for prec, c, M, (b, h, w), pitch in itertools.product([0, 1, 4], [16, 128], [64, 128], [(4, 32, 32), (16, 32, 16), (4, 32, 8)],
                                                         [0, 1, 16]):
        ldb = {0: 0, 1: c, 16: c + 16}[pitch]
        add("convw", gemm(M, c, b * h * w, 1, 1, b0=9, split_k=0, precision=prec, cv_h=h, cv_w=w, cv_c=c, cv_wgrad=1, ldb=ldb,
                          c_bs0=M * c))

    # narrow token products on the packed-B kernels (M >= 16384, N 16..95), misaligned A, odd lda, K % 4 != 0
    for prec, M, N, K, lb, extra in itertools.product(
            [F16X2, BF16X3, BF16X2], [16384, 8192], [16, 64, 96], [64, 130], [0, 1],
            [{}, {"A": 4}, {"lda": 131}, {"b_packed": True}, {"a_colsum": True}, {"bias": True, "act": 2}]):
        if lb and extra:
            continue
        add("narrow", gemm(M, N, K, 0, lb, precision=prec, **extra))

    # two-term fp16 weight gradients (K >= 16384, M and N multiples of 32)
    for prec, K, M, N, extra in itertools.product(
            [F16X2, BF16X3], [16384, 65536, 8192], [32, 384, 100], [32, 192],
            [{}, {"a_colsum": True}, {"A": 4}, {"A": 8}, {"a_drop.p": 0.1}]):
        add("wgrad16", gemm(M, N, K, 1, 1, split_k=0, precision=prec, **extra))

    # misaligned A, odd lda, K % 4 != 0 on both engines; a_colsum with either layout
    for prec, (la, lb), K, off, dl in itertools.product([F32, BF16X3], LAYOUTS, [512, 510], [0, 4, 8], [0, 1, 4]):
        f = gemm(512, 256, K, la, lb, precision=prec, A=off, a_colsum=(off == 0 and dl == 0))
        f["lda"] += dl
        add("align", f)

    # what the plan itself refuses, and the activations
    for act in [-1, 0, 1, 2, 3, 4, 5, 6]:
        add("act", gemm(300, 256, 128, act=act))
        add("act", gemm(300, 256, 128, act=act, **{"drop.p": 0.1}))
    add("bad", gemm(0, 128, 128))
    add("bad", gemm(128, 128, -1))
    add("bad", gemm(128, 128, 128, b0=300, b1=300))
    add("bad", gemm(128, 128, 128, b0=0))
    for prec in [F32, BF16X3]:
        add("split", gemm(256, 256, 4096, split_k=4, precision=prec, bias=True))
        add("split", gemm(256, 256, 4096, split_k=2000, precision=prec))
        add("split", gemm(256, 256, 0, split_k=0, precision=prec))
        add("split", gemm(256, 256, 4096, 1, 1, split_k=4, precision=prec, a_colsum=True))
    return out


def _hip():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "galerkin-transformer_amd"))
    from galerkin_transformer import _hip as H
    return H


def query(H, fields):
    """(plan rc, bm, bn, split, name rc, name, ws bytes, packed bytes) of one descriptor.  Queries only: nothing launches."""
    L = H.lib()
    d = H.GtGemmDesc()
    L.gt_gemm_desc_init(C.byref(d))
    for k, v in fields.items():
        if k.endswith(".p"):
            drop = getattr(d, k[:-2])
            drop.p, drop.salt, drop.seed = v, 3, ADDR["seed"]
        else:
            setattr(d, k, v)
    bm, bn, sp = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    prc = L.gt_gemm_plan(C.byref(d), C.byref(bm), C.byref(bn), C.byref(sp))
    buf = C.create_string_buffer(160)
    nrc = L.gt_gemm_kernel_name(C.byref(d), buf, 160)
    return [prc, bm.value, bn.value, sp.value, nrc, buf.value.decode() if nrc == 0 else "",
            int(L.gt_gemm_ws_bytes(C.byref(d))), int(L.gt_gemm_packed_b_bytes(C.byref(d)))]


def table(H):
    """{"names": [...], "tags": [[family, count], ...], "rows": [[plan rc, bm, bn, split, name rc, index into names, ws, packed]]},
    rows and families in the order of cases()."""
    for k in [k for k in os.environ if k.startswith("GT_GEMM_")]:
        del os.environ[k]
    names, tags, rows = [], [], []
    for cid, f in cases():
        r = query(H, f)
        if r[5] not in names:
            names.append(r[5])
        r[5] = names.index(r[5])
        rows.append(r)
        if not tags or tags[-1][0] != cid.split("#")[0]:
            tags.append([cid.split("#")[0], 0])
        tags[-1][1] += 1
    return {"names": names, "tags": tags, "rows": rows}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    g["rows"] = [g["answers"][i] for i in g["rows"]]
    return g


def test_dispatch_table_matches_the_recording(golden, monkeypatch):
    for k in [k for k in os.environ if k.startswith("GT_GEMM_")]:
        monkeypatch.delenv(k)
    got = table(_hip())
    assert got["tags"] == golden["tags"], "the case list changed: record again from the parent library"
    bad = []
    for (cid, fields), want, have in zip(cases(), golden["rows"], got["rows"]):
        w = want[:5] + [golden["names"][want[5]]] + want[6:]
        h = have[:5] + [got["names"][have[5]]] + have[6:]
        if w != h:
            bad.append(f"{cid} {fields}\n    recorded {w}\n    now      {h}")
    assert not bad, f"{len(bad)} of {len(golden['rows'])} descriptors changed:\n" + "\n".join(bad[:20])


def test_recording_reaches_every_engine_and_branch(golden):
    """The table would pin nothing down if the list missed an engine: every family of instances, both refusal codes of the
    plan, packed weights of one and of two launches, scratch of each kind."""
    names, rows = golden["names"], golden["rows"]
    tags = [t for t, n in golden["tags"] for _ in range(n)]
    assert len(rows) == len(tags) > 2000
    used = {names[r[5]] for r in rows if r[4] == 0}
    patterns = [r"gemm_kernel<\d, \d, \d, \d, \d, \d, 16, 0>", r"gemm_kernel<\d, \d, \d, \d, \d, \d, 32, 0>",
                r"gemm_kernel<0, 0, \d, \d, \d, \d, 16, 1>", r"gemm_kernel<0, 0, \d, \d, \d, \d, 16, 4>",
                r"gemm_stream_kernel<\d, \d, 4>", r"gemm_stream_kernel<\d, \d, 2>",
                r"tsmm_kernel<1, 8>", r"tsmm_kernel<2, 4>", r"tsmm_kernel<3, 2>", r"tsmm_kernel<4, 2>",
                r"gemm_x3_kernel<", r"gemm_x3p_kernel<", r"gemm_x3w_kernel<",
                r"gemm_x3r_kernel<\d, \d, \d, 3, 0, 0>", r"gemm_x3r_kernel<\d, \d, \d, 3, 0, 1>", r"gemm_x3r_kernel<\d, \d, \d, 3, 0, 2>",
                r"gemm_x3r_kernel<0, 0, 3, 3, 16, 0>", r"gemm_x3r_kernel<0, 0, 3, 3, 32, 0>", r"gemm_x3r_kernel<0, 0, 3, 3, 64, 0>",
                r"gemm_x3h_kernel<\d, \d+, \d, 64>", r"gemm_x3h_kernel<\d, \d+, \d, 128>"]
    for pat in patterns:
        assert any(re.search(pat, n) for n in used), pat
    assert {-1, -4} <= {r[0] for r in rows}
    tagged = list(zip(tags, rows))
    assert any(r[7] > 0 for t, r in tagged if t == "narrow")                                # one packed-B launch
    assert any(r[7] > 0 for t, r in tagged if t == "width" and r[0] == 0)                   # two of them
    assert any(r[6] > 0 and r[3] > 1 for t, r in tagged if t in ("grid", "autosplit"))      # split-K slabs
    assert any(r[6] > 0 and "tsmm_kernel" in names[r[5]] for r in rows)
    assert any(r[6] > 0 and r[7] == 0 for t, r in tagged if t == "head")                    # MLP_BWD's dw2 partials


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    t = table(_hip())
    with open(GOLDEN, "w") as fh:
        # many descriptors share an answer: the distinct answers once, then one index per descriptor
        uniq = sorted({tuple(r) for r in t["rows"]})
        ans = [json.dumps(u, separators=(",", ":")) for u in uniq]
        idx = [str(uniq.index(tuple(r))) for r in t["rows"]]
        fh.write('{"names": ' + json.dumps(t["names"], indent=1) + ',\n "tags": ' + json.dumps(t["tags"]) + ',\n "answers": [\n')
        fh.write(",\n".join(",".join(ans[i:i + 6]) for i in range(0, len(ans), 6)))
        fh.write('\n],\n "rows": [\n' + ",\n".join(",".join(idx[i:i + 40]) for i in range(0, len(idx), 40)) + "\n]}\n")
    print(f"{len(t['rows'])} descriptors, {len(t['names'])} names -> {GOLDEN}")
