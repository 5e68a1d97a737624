"""-m gpu: the row kernels of slamkit_amd/csrc/elementwise.hip through the C ABI, held PER ELEMENT to float64 at the rounding
bound (tests/row_exact_ref.py has the rule, the references and the derivation of DELTA = 2^-16; nothing here widens it):

    bf16 outputs:  bf16_rne(ref - DELTA S) <= got <= bf16_rne(ref + DELTA S)          fp32 outputs:  |got - ref| <= DELTA S

with DELTA_SUM = M 2^-24 + 2^-16 for sums over M rows, the table bound for the RoPE tables and bit equality wherever a result
is exact (zeros, untouched columns, position 0, constant LayerNorm rows, integer column sums, saved inputs).

Every output is a NaN-filled window between 256-element bands of a bit pattern no kernel produces; every workspace has exactly
the byte count its *_workspace function returns (rounded up to 16) with a band behind it; every operand, weight vectors
included, sits between such bands too; a buffer rewritten in place (qkv, dqkv, the fp32 decode rows, gu) is an output: its bands
are checked after every launch, and so are those of the column sums' X, whose bits (NaN beyond N included) must survive.
Every launch runs twice and must give the same bits. Each case prints the share of
elements that differ from bf16_rne(ref) and the worst |err| / S of its fp32 outputs. The float64 references of the large norm
shapes are computed on the device (the reference functions are plain torch), once per shape.

Which kernel and template instantiation each shape reaches, and what the runs measured: profiles/row_exact.md."""
import functools

import pytest
import torch

from tests import row_exact_ref as R
from tests.gpu_util import lib, ptr, stream, sync

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
V_BITS = 0x7FC3          # what the columns a kernel must leave alone hold (a NaN: reading one poisons the result)


def operand(t, dtype=BF16):
    """device copy of `t` between bands (a read outside the window meets NaN)"""
    return R.guarded(tuple(t.shape), dtype, DEV, fill=t.to(DEV))[0]


def inplace(t, dtype=BF16):
    """an in-place output: device copy of `t` between bands, WITH the check of those bands -> (payload, check)"""
    return R.guarded(tuple(t.shape), dtype, DEV, fill=t.to(DEV))


def same_bits(name, a, b):
    assert torch.equal(R.bits(a), R.bits(b)), f"{name}: {int((R.bits(a) != R.bits(b)).sum())} of {a.numel()} elements differ in bits"


def twice(name, launch):
    """launch() -> (dict of output tensors, list of band checks); run it twice: same bits, bands intact. Returns the outputs."""
    first, checks = launch()
    sync()
    for c in checks:
        c(name)
    first = {k: v.clone() for k, v in first.items()}
    second, checks = launch()
    sync()
    for c in checks:
        c(name + " (second run)")
    for k in first:
        same_bits(f"{name} {k}: run 1 vs run 2", first[k], second[k])
    return first


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for cached in (norm_inputs, ce_inputs):
        cached.cache_clear()
    torch.cuda.empty_cache()


# =============================================================================================== RMSNorm, LayerNorm
NARROW_H = [8, 64, 504, 512, 520, 1016, 1024, 1032, 1536, 1544, 2040, 2048]
WIDE_H = [2056, 3072, 3080, 4088, 4096]
RMS_CASES = ([(M, H) for H in NARROW_H for M in (1, 5)] + [(17, 512), (17, 2048), (8195, 64)]
             + [(M, H) for H in WIDE_H for M in (1, 2, 3, 35)] + [(8195, 2056)]
             + [(33, 2056), (33, 4096)])   # 3 blocks of 6, 6 and 5 iterations (at M = 35 all three run 6, the last pair idle in its last)
LN_CASES = [(M, H) for H in NARROW_H for M in (1, 5, 17)] + [(8195, 64)]


@functools.lru_cache(maxsize=2)
def norm_inputs(kind, M, H):
    special = M in (5, 35)
    x = (R.ln_rows if kind == "ln" else R.norm_rows)(M, H, 1, special)
    return {"x": x.to(DEV), "w": R.norm_weight(H, 2).to(DEV), "b": R.rnd(H, seed=5, scale=0.1).to(DEV),
            "dy": R.rnd(M, H, seed=3).to(DEV), "dres": R.rnd(M, H, seed=4).to(DEV), "special": special}


@pytest.mark.parametrize("M,H", RMS_CASES)
def test_rmsnorm_fwd_bwd(M, H):
    L, c = lib(), norm_inputs("rms", M, H)
    x, w, dy, dres = c["x"], c["w"], c["dy"], c["dres"]
    assert float(x.abs().max()) <= 2.0 ** 40
    xd, wd, dyd, dresd = operand(x), operand(w), operand(dy), operand(dres)
    tag = f"rmsnorm {M}x{H}"

    def fwd():
        y, cy = R.guarded((M, H), BF16, DEV)
        rstd, cr = R.guarded(M, F32, DEV)
        assert L.slam_op_rmsnorm_fwd(ptr(xd), ptr(wd), ptr(y), ptr(rstd), M, H, R.EPS_RMS, stream()) == 0
        return {"y": y, "rstd": rstd}, [cy, cr]
    o = twice(tag + " fwd", fwd)
    y_ref, Sy, rstd_ref = R.rmsnorm_fwd(x, w)
    assert R.accept_f32(tag + " rstd", o["rstd"], rstd_ref, rstd_ref) == 0
    assert R.accept_bf16(tag + " y", o["y"], y_ref, Sy) == 0
    if c["special"]:
        assert bool((o["y"][0] == 0).all()) and bool((o["y"][M - 1] == 0).all())      # all-zero and -0.0 rows: +-0, nothing else
    rstd = o["rstd"]                                                                  # the backward's input, as the forward left it
    nbytes = L.slam_op_rmsnorm_bwd_workspace(M, H)
    for use_res in (False, True):
        def bwd():
            dx, cx = R.guarded((M, H), BF16, DEV)
            dw, cw = R.guarded(H, F32, DEV)                                            # NaN: dw is stored, not accumulated
            ws, cws = R.workspace(nbytes, DEV)
            assert L.slam_op_rmsnorm_bwd(ptr(dyd), ptr(xd), ptr(wd), ptr(rstd), ptr(dresd) if use_res else None, ptr(dx), ptr(dw),
                                         ptr(ws), M, H, stream()) == 0
            return {"dx": dx, "dw": dw}, [cx, cw, cws]
        o2 = twice(f"{tag} bwd res={use_res}", bwd)
        dx_ref, Sdx, dw_ref, Sdw = R.rmsnorm_bwd(dy, x, w, rstd.double(), dres if use_res else None)
        assert R.accept_bf16(f"{tag} dx res={use_res}", o2["dx"], dx_ref, Sdx) == 0
        assert R.accept_f32(f"{tag} dw res={use_res}", o2["dw"], dw_ref, Sdw, R.delta_sum(M)) == 0


@pytest.mark.parametrize("M,H", LN_CASES)
def test_layernorm_fwd_bwd(M, H):
    L, c = lib(), norm_inputs("ln", M, H)
    x, w, b, dy, dres = c["x"], c["w"], c["b"], c["dy"], c["dres"]
    xd, wd, bd, dyd, dresd = operand(x), operand(w), operand(b), operand(dy), operand(dres)
    tag = f"layernorm {M}x{H}"

    def fwd():
        y, cy = R.guarded((M, H), BF16, DEV)
        mean, cm = R.guarded(M, F32, DEV)
        rstd, cr = R.guarded(M, F32, DEV)
        assert L.slam_op_layernorm_fwd(ptr(xd), ptr(wd), ptr(bd), ptr(y), ptr(mean), ptr(rstd), M, H, R.EPS_LN, stream()) == 0
        return {"y": y, "mean": mean, "rstd": rstd}, [cy, cm, cr]
    o = twice(tag + " fwd", fwd)
    y_ref, Sy, mean_ref, Smean, rstd_ref = R.layernorm_fwd(x, w, b)
    assert R.accept_f32(tag + " mean", o["mean"], mean_ref, Smean) == 0
    assert R.accept_f32(tag + " rstd", o["rstd"], rstd_ref, rstd_ref) == 0
    assert R.accept_bf16(tag + " y", o["y"], y_ref, Sy) == 0
    if c["special"]:   # the constant row: its sums are exact (8 bits times at most 2048 terms), so mean == c and y == b, bit for bit
        assert float(o["mean"][0]) == 3.5
        same_bits(tag + " constant row: y == b", o["y"][0], bd)
        same_bits(tag + " all-zero row: y == b", o["y"][M - 1], bd)
    mean, rstd = o["mean"], o["rstd"]
    nbytes = L.slam_op_layernorm_bwd_workspace(M, H)
    for use_res in (False, True):
        def bwd():
            dx, cx = R.guarded((M, H), BF16, DEV)
            dw, cw = R.guarded(H, F32, DEV)
            db, cb = R.guarded(H, F32, DEV)
            ws, cws = R.workspace(nbytes, DEV)
            assert L.slam_op_layernorm_bwd(ptr(dyd), ptr(xd), ptr(wd), ptr(mean), ptr(rstd), ptr(dresd) if use_res else None, ptr(dx),
                                           ptr(dw), ptr(db), ptr(ws), M, H, stream()) == 0
            return {"dx": dx, "dw": dw, "db": db}, [cx, cw, cb, cws]
        o2 = twice(f"{tag} bwd res={use_res}", bwd)
        dx_ref, Sdx, dw_ref, Sdw, db_ref, Sdb = R.layernorm_bwd(dy, x, w, mean.double(), rstd.double(), dres if use_res else None)
        assert R.accept_bf16(f"{tag} dx res={use_res}", o2["dx"], dx_ref, Sdx) == 0
        assert R.accept_f32(f"{tag} dw res={use_res}", o2["dw"], dw_ref, Sdw, R.delta_sum(M)) == 0
        assert R.accept_f32(f"{tag} db res={use_res}", o2["db"], db_ref, Sdb, R.delta_sum(M)) == 0


def test_layernorm_refuses_wide_rows():
    """LayerNorm has no wide form: H = 2056 is refused by both entry points before any launch (nothing is written)."""
    L, M, H = lib(), 3, 2056
    x, w = operand(R.rnd(M, H, seed=1)), operand(R.norm_weight(H, 2))
    y, cy = R.guarded((M, H), BF16, DEV)
    st, cs = R.guarded(2 * M, F32, DEV)
    dwb, cd = R.guarded(2 * H, F32, DEV)
    ws, cws = R.workspace(max(L.slam_op_layernorm_bwd_workspace(M, H), 16), DEV)
    before = [R.bits(t).clone() for t in (y, st, dwb, ws)]
    assert L.slam_op_layernorm_fwd(ptr(x), ptr(w), ptr(w), ptr(y), ptr(st), ptr(st[M:]), M, H, R.EPS_LN, stream()) != 0
    assert L.slam_op_layernorm_bwd(ptr(x), ptr(x), ptr(w), ptr(st), ptr(st[M:]), None, ptr(y), ptr(dwb), ptr(dwb[H:]), ptr(ws), M, H,
                                   stream()) != 0
    sync()
    for t, b in zip((y, st, dwb, ws), before):
        assert torch.equal(R.bits(t), b)
    for chk in (cy, cs, cd, cws):
        chk("layernorm refusal")


# =============================================================================================== RoPE tables
def packed_positions(M):
    """positions with two resets"""
    a, b = max(M // 4, 1), max(M // 2, 1)
    if M < 3:
        return torch.zeros(M, dtype=torch.int64)
    return torch.cat([torch.arange(a), torch.arange(b), torch.arange(M - a - b)])


def check_tables(tag, ws, pos, M, hd, theta, with_q):
    """The tables the kernel built, read back from the workspace: cos | sin (| cos q | sin q), [M][hd / 2] fp32 each. Held to
    float64 cos / sin of the float64 angle within the table bound; the q tables to fp32(table) * qscale within one fp32 ulp.
    Returns them as float64 (the rotation's reference uses the kernel's own table values)."""
    half = hd // 2
    n = M * half
    t = ws[: (4 if with_q else 2) * n].clone().view(-1, M, half)
    ang = R.rope_angles(pos, hd, theta).to(DEV)
    bound = R.table_bound(ang)
    for name, got, ref in (("cos", t[0], torch.cos(ang)), ("sin", t[1], torch.sin(ang))):
        err = (got.double() - ref).abs()
        print(f"[row-exact] {tag} {name} table: worst err / bound = {float((err / bound).max()):.3e}, max angle {float(ang.max()):.1f}")
        assert bool((err <= bound).all()), f"{tag}: {name} table off by {float((err - bound).max()):.3e} beyond the bound"
    if with_q:
        qs = R.qscale(hd)
        for name, got, base in (("cos q", t[2], t[0]), ("sin q", t[3], t[1])):
            want = base.double() * qs
            _, e = torch.frexp(want.abs())
            ulp = torch.ldexp(torch.ones_like(want), e - 24)
            assert bool(((got.double() - want).abs() <= torch.where(want == 0, torch.zeros_like(ulp), ulp)).all()), f"{tag}: {name} table"
    return tuple(x.double() for x in t)


# =============================================================================================== Qwen3 q/k norm
@pytest.mark.parametrize("packed", [False, True], ids=["modT", "packed"])
@pytest.mark.parametrize("M", [1, 5, 37])
@pytest.mark.parametrize("nH,nKV", [(1, 1), (3, 1), (14, 2)])
@pytest.mark.parametrize("hd", [64, 128])
def test_qknorm(hd, nH, nKV, M, packed):
    L = lib()
    nQK, ld, half, T, theta = nH + nKV, (nH + 2 * nKV) * hd, hd // 2, 13, 10000.0
    tag = f"qknorm hd={hd} {nH}/{nKV} M={M} {'packed' if packed else 'modT'}"
    x = R.rnd(M, nQK, hd, seed=1)
    x[0, 0], x[M - 1, nQK - 1] = 0.0, 0.0                                 # a zero head first and last in the batch
    wq, wk = R.norm_weight(hd, 2), R.norm_weight(hd, 3)
    pos = packed_positions(M) if packed else torch.arange(M) % T
    posd = pos.to(DEV) if packed else None
    wqd, wkd = operand(wq), operand(wk)
    vcols = torch.full((M, ld - nQK * hd), V_BITS, dtype=torch.int16).view(BF16)
    full = torch.cat([x.reshape(M, nQK * hd).to(BF16), vcols], 1)
    nws = 4 * M * half * 4

    def fwd(save=True):
        qkv, c0 = inplace(full)
        raw, c1 = R.guarded((M, nQK * hd), BF16, DEV)
        rstd, c2 = R.guarded((M, nQK), F32, DEV)
        ws, c3 = R.workspace(nws, DEV)
        assert L.slam_op_qknorm_rope_fwd(ptr(qkv), ptr(wqd), ptr(wkd), ptr(posd), theta, R.EPS_RMS, M, T, nH, nKV, hd,
                                         ptr(raw) if save else None, ptr(rstd) if save else None, ptr(ws), stream()) == 0
        return {"qkv": qkv, "raw": raw, "rstd": rstd, "ws": ws}, [c0, c1, c2, c3]
    o = twice(tag + " fwd", fwd)
    tabs = tuple(t.cpu() for t in check_tables(tag, o["ws"], pos, M, hd, theta, True))
    ref, S, rstd_ref = R.qknorm_fwd(x, wq, wk, nH, tabs)
    assert R.accept_f32(tag + " rstd", o["rstd"].cpu(), rstd_ref, rstd_ref) == 0
    assert R.accept_bf16(tag + " y", o["qkv"][:, : nQK * hd].cpu().reshape(M, nQK, hd), ref, S) == 0
    same_bits(tag + " raw_out", o["raw"].cpu(), full[:, : nQK * hd])
    same_bits(tag + " v columns", o["qkv"][:, nQK * hd:].cpu(), vcols)
    assert bool((o["qkv"][0, :hd] == 0).all()) and bool((o["qkv"][M - 1, (nQK - 1) * hd: nQK * hd] == 0).all())
    nul, checks = fwd(save=False)                                        # raw_out = rstd_out = NULL: the same rotation, nothing saved
    sync()
    for chk in checks:
        chk(tag + " NULL outputs")
    same_bits(tag + " qkv with NULL outputs", nul["qkv"], o["qkv"])
    assert bool(torch.isnan(nul["raw"]).all()) and bool(torch.isnan(nul["rstd"]).all())

    # backward: dy in the q|k columns, the forward's raw and rstd as inputs
    dy = R.rnd(M, nQK, hd, seed=4)
    dfull = torch.cat([dy.reshape(M, nQK * hd).to(BF16), vcols], 1)
    raw, rstd = o["raw"], o["rstd"]
    nb = L.slam_op_qknorm_bwd_workspace(M, nH, nKV, hd)
    assert nb > 0

    def bwd():
        d, c0 = inplace(dfull)
        dwq, c1 = R.guarded(hd, F32, DEV)
        dwk, c2 = R.guarded(hd, F32, DEV)
        ws, c3 = R.workspace(nb, DEV)
        assert L.slam_op_qknorm_bwd(ptr(d), ptr(raw), ptr(rstd), ptr(wqd), ptr(wkd), ptr(dwq), ptr(dwk), ptr(ws), M, nH, nKV, hd,
                                    stream()) == 0
        return {"d": d, "dwq": dwq, "dwk": dwk}, [c0, c1, c2, c3]
    ob = twice(tag + " bwd", bwd)
    dx, Sdx, dwq, Sq, dwk, Sk = R.qknorm_bwd(dy, x, rstd.cpu().double(), wq, wk, nH)
    assert R.accept_bf16(tag + " dx", ob["d"][:, : nQK * hd].cpu().reshape(M, nQK, hd), dx, Sdx) == 0
    same_bits(tag + " bwd v columns", ob["d"][:, nQK * hd:].cpu(), vcols)
    assert R.accept_f32(tag + " dw_q", ob["dwq"].cpu(), dwq, Sq, R.delta_sum(M * nH)) == 0
    assert R.accept_f32(tag + " dw_k", ob["dwk"].cpu(), dwk, Sk, R.delta_sum(M * nKV)) == 0

    # the decode-time form on fp32 rows
    f32full = torch.cat([x.reshape(M, nQK * hd).float(), torch.full((M, ld - nQK * hd), 0x7FC00003, dtype=torch.int32).view(F32)], 1)

    def rows():
        q, c0 = inplace(f32full, F32)
        assert L.slam_op_qknorm_rows_f32(ptr(q), ptr(wqd), ptr(wkd), R.EPS_RMS, M, nH, nKV, hd, stream()) == 0
        return {"q": q}, [c0]
    orow = twice(tag + " rows_f32", rows)
    yr, Sr = R.qknorm_rows(x, wq, wk, nH)
    assert R.accept_f32(tag + " rows_f32", orow["q"][:, : nQK * hd].cpu().reshape(M, nQK, hd), yr, Sr) == 0
    same_bits(tag + " rows_f32 v columns", orow["q"][:, nQK * hd:].cpu(), f32full[:, nQK * hd:])


# =============================================================================================== RoPE
ROPE_POS = {"M1": (1, 1, None), "M5-packed": (5, 5, torch.tensor([0, 1, 0, 0, 1])), "M150-T75": (150, 75, None),
            "M150-packed": (150, 75, torch.cat([torch.arange(40), torch.arange(60), torch.arange(50)])),
            "M5-far": (5, 5, torch.tensor([0, 8191, 4096, 1, 8190]))}


@pytest.mark.parametrize("where", list(ROPE_POS))
@pytest.mark.parametrize("nrot", [1, 3, 6])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope(hd, nrot, where):
    L = lib()
    M, T, pos = ROPE_POS[where]
    theta, half, ld = 10000.0, hd // 2, (nrot + 2) * hd                    # 2 more heads behind the rotated ones: never touched
    tag = f"rope hd={hd} nrot={nrot} {where}"
    posd = pos.to(DEV) if pos is not None else None
    pos_ref = pos if pos is not None else torch.arange(M) % T
    x = R.rnd(M, nrot, hd, seed=1)
    rest = torch.full((M, 2 * hd), V_BITS, dtype=torch.int16).view(BF16)
    full = torch.cat([x.reshape(M, nrot * hd).to(BF16), rest], 1)
    for backward in (0, 1):
        def run():
            q, c0 = inplace(full)
            ws, c = R.workspace(2 * M * half * 4, DEV)
            assert L.slam_op_rope(ptr(q), ld, M, T, nrot, hd, ptr(posd), theta, backward, ptr(ws), stream()) == 0
            return {"q": q, "ws": ws}, [c0, c]
        o = twice(f"{tag} backward={backward}", run)
        cs, sn = (t.cpu() for t in check_tables(tag, o["ws"], pos_ref, M, hd, theta, False))
        ref, S = R.rotate(x, cs[:, None], sn[:, None], -1.0 if backward else 1.0)   # backward: the transpose rotation of ITS input
        got = o["q"].cpu()
        assert R.accept_bf16(f"{tag} backward={backward}", got[:, : nrot * hd].reshape(M, nrot, hd), ref, S) == 0
        same_bits(tag + " unrotated heads", got[:, nrot * hd:], rest)
        at0 = (pos_ref == 0).nonzero()[:, 0]                                # cos = 1, sin = 0 exactly: the input bits come back
        same_bits(tag + " position 0", got[at0, : nrot * hd], full[at0, : nrot * hd])


# =============================================================================================== SwiGLU
@pytest.mark.parametrize("M", [1, 3, 7])
@pytest.mark.parametrize("I", [8, 40, 4864])
def test_swiglu(I, M):
    L, tag = lib(), f"swiglu {M}x{I}"
    g, u, d = R.swiglu_inputs(M, I, 1)
    assert float(g.abs().max()) <= 60
    gu = torch.cat([g, u], 1)
    gud, dd = operand(gu), operand(d)

    def fwd():
        act, c = R.guarded((M, I), BF16, DEV)
        assert L.slam_op_swiglu_fwd(ptr(gud), ptr(act), M, I, stream()) == 0
        return {"act": act}, [c]
    o = twice(tag + " fwd", fwd)
    a, Sa = R.swiglu_fwd(g, u)
    act = o["act"].cpu()
    assert R.accept_bf16(tag + " act", act, a, Sa) == 0
    assert bool((act[:, :2] == 0).all()) and bool((act[:, 5] == 0).all())   # silu(+-0) u and silu(g) 0 are zeros

    def bwd():
        buf, c = R.guarded((M, 2 * I), BF16, DEV, fill=gu.to(DEV))            # rewritten whole: only its bands are guarded
        assert L.slam_op_swiglu_bwd(ptr(buf), ptr(dd), M, I, stream()) == 0
        return {"dgu": buf}, [c]
    ob = twice(tag + " bwd", bwd)["dgu"].cpu()
    dg, Sg, du, Su = R.swiglu_bwd(g, u, d)
    assert R.accept_bf16(tag + " dgate", ob[:, :I], dg, Sg) == 0
    assert R.accept_bf16(tag + " dup", ob[:, I:], du, Su) == 0
    assert bool((ob[:, I: I + 2] == 0).all())                                 # dup at g = +-0
    assert bool((ob[:, 5] == 0).all())                                        # dgate at u = 0


# =============================================================================================== cross entropy
CE_SHAPES = [(1, 512), (8, 512), (500, 512), (502, 512), (505, 512), (512, 512),       # ce_kernel: one wave per row
             (513, 520), (520, 520), (700, 768), (2041, 2048), (2049, 2056), (4100, 4104)]  # ce_big_kernel


@functools.lru_cache(maxsize=None)
def ce_inputs(B, T, V, Vp):
    z, lab, under = R.ce_case(B, T, V, Vp, 1)
    keep = torch.ones(B * T, dtype=torch.bool)
    keep[under] = False
    others = z[keep][:, :V]
    assert float((others.max(-1, keepdim=True).values - others).max()) <= 80
    return z, lab, keep


@pytest.mark.parametrize("num_items", [0.0, 57.0])
@pytest.mark.parametrize("eps", [0.0, R.EPS_SMOOTH], ids=["plain", "smooth"])
@pytest.mark.parametrize("B,T", [(3, 7), (1, 2)])
@pytest.mark.parametrize("V,Vp", CE_SHAPES)
def test_cross_entropy(V, Vp, B, T, eps, num_items):
    ce_protocol(V, Vp, B, T, eps, num_items)


def ce_protocol(V, Vp, B, T, eps, num_items, delta=R.DELTA):
    """The whole cross-entropy protocol at one shape; `delta` is DELTA for every case of this file (tests/test_gpu_far_rows.py
    runs the same protocol at the real vocabulary under R.delta_steps of its step count)."""
    L, M = lib(), B * T
    tag = f"ce V={V} Vp={Vp} {B}x{T} eps={eps:.1f} items={num_items:.0f}"
    z, lab, keep = ce_inputs(B, T, V, Vp)
    r = R.cross_entropy(z, lab, V, num_items, eps)
    labd = lab.to(DEV)

    def launch(zd, dl, rl, rs, sc):
        if eps:
            return L.slam_op_cross_entropy_smooth(ptr(zd), ptr(labd), num_items, ptr(dl), ptr(rl), ptr(rs), ptr(sc), B, T, Vp, V,
                                                  eps, stream())
        return L.slam_op_cross_entropy(ptr(zd), ptr(labd), num_items, ptr(dl), ptr(rl), ptr(sc), B, T, Vp, V, stream())

    def run(pad=0.0, alias=False, null=False):
        zz = z.clone()
        zz[:, V:] = pad
        zd, cz = R.guarded((M, Vp), BF16, DEV, fill=zz.to(DEV))
        dl, cd = (zd, cz) if alias else R.guarded((M, Vp), BF16, DEV)
        rl, c1 = R.guarded(M, F32, DEV)
        rs, c2 = R.guarded(M, F32, DEV)
        sc, c3 = R.guarded(2, F32, DEV)
        assert launch(zd, None if null else dl, rl, rs, sc) == 0
        return {"z": zd, "dl": dl, "rl": rl, "rs": rs, "sc": sc}, [cz, cd, c1, c2, c3]
    o = {k: v.cpu() for k, v in twice(tag, run).items()}
    ref, S = r["dlogits"]
    dl = o["dl"]
    assert float(o["sc"][0]) == r["denom"]
    assert R.accept_bf16(tag + " dlogits", dl[keep], ref[keep], S[keep], delta) == 0
    if not bool(keep.all()):
        assert R.accept_bf16(tag + " dlogits, saturated rows", dl[~keep], ref[~keep], S[~keep], delta, underflow=True) == 0
    assert bool((R.bits(dl[:, V:]) == 0).all()), "pad columns of dlogits must be +0"
    assert bool((R.bits(dl[~r["valid"]]) == 0).all()), "ignored and out-of-range rows of dlogits must be +0"
    assert R.accept_f32(tag + " row_loss", o["rl"], *r["row_loss"], delta) == 0
    assert bool((o["rl"][~r["valid"]] == 0).all())
    if eps:
        assert R.accept_f32(tag + " row_smooth", o["rs"], *r["row_smooth"], delta) == 0
    assert R.accept_f32(tag + " loss", o["sc"][1:], *r["loss"], R.delta_sum(M) + (delta - R.DELTA)) == 0
    # the pad columns are outside the softmax whatever they hold; dlogits may alias logits; dlogits may be NULL
    for name, kw in (("NaN pads", {"pad": NAN}), ("3e38 pads", {"pad": 3.0e38}), ("aliased", {"alias": True}), ("NULL dlogits", {"null": True})):
        v, checks = run(**kw)
        sync()
        for chk in checks:
            chk(f"{tag} {name}")
        same_bits(f"{tag} {name}: row_loss", v["rl"].cpu(), o["rl"])
        same_bits(f"{tag} {name}: loss", v["sc"].cpu(), o["sc"])
        if eps:
            same_bits(f"{tag} {name}: row_smooth", v["rs"].cpu(), o["rs"])
        if kw.get("null"):
            same_bits(f"{tag} {name}: logits untouched", v["z"].cpu(), o["z"])
            assert bool(torch.isnan(v["dl"]).all())
        else:
            same_bits(f"{tag} {name}: dlogits", v["dl"].cpu(), dl)


# =============================================================================================== column sums
@pytest.mark.parametrize("extra", [0, 64], ids=["ld=N", "ld=N+64"])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 1025, 8200])
@pytest.mark.parametrize("N", [8, 120, 128, 136, 896])
def test_colsum(N, M, extra):
    L, ld, tag = lib(), N + extra, f"colsum {M}x{N} ld={N + extra}"
    nbytes = L.slam_op_colsum_workspace(M, N)
    g = torch.Generator().manual_seed(1)
    ints = torch.randint(-3, 4, (M, N), generator=g).double()
    init = torch.randint(-3, 4, (N,), generator=g).float()
    for kind, X in (("ints", ints), ("normal", R.rnd(M, N, seed=2))):
        full = torch.full((M, ld), NAN, dtype=F64)                           # the columns beyond N hold NaN: never read
        full[:, :N] = X
        Xd, cX = inplace(full)                                               # read-only: its bits and its bands must survive
        Xbits = R.bits(Xd).clone()
        for acc in (0, 1):
            def run():
                out, c = R.guarded(N, F32, DEV, fill=init.to(DEV) if acc else None)   # accumulate = 0 stores onto NaN
                ws, cw = R.workspace(nbytes, DEV)
                assert L.slam_op_colsum(ptr(Xd), ld, M, N, ptr(out), acc, ptr(ws), stream()) == 0
                return {"out": out}, [c, cw, cX]
            out = twice(f"{tag} {kind} acc={acc}", run)["out"].cpu()
            assert torch.equal(R.bits(Xd), Xbits), f"{tag}: X (the NaN columns beyond N included) changed"
            ref, S = R.colsum(X)
            if acc:
                ref, S = ref + init.double(), S + init.double().abs()
            if kind == "ints":      # every partial sum is an integer below 2^24: exact in any order
                assert torch.equal(out.double(), ref), f"{tag}: {int((out.double() != ref).sum())} integer column sums differ"
            else:
                assert R.accept_f32(f"{tag} acc={acc}", out, ref, S, R.delta_sum(M)) == 0
