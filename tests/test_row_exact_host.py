"""Host checks of tests/row_exact_ref.py (no GPU): the float64 references against torch float64 forward and autograd of the
plain formulas, an fp32 restatement of every formula with STRICTLY SEQUENTIAL reductions through the acceptance rule (0
violations: DELTA is a property of the reference, not of the kernels), the rule's power to reject five mutants - and what
tests/gpu_util.check makes of the same mutants at the tolerances of tests/test_gpu_ops.py (profiles/row_exact.md has the table).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import row_exact_ref as R

F64, BF16 = torch.float64, torch.bfloat16


def close(name, a, b, tol=1e-12):
    a, b = a.double(), b.double()
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{name}: {err:.3e} > {tol} * {scale:.3e}"


# ------------------------------------------------------------------------------------------------ bf16_rne
def test_bf16_rne_rounds_once():
    u = 2.0 ** -7                                            # bf16 spacing in [1, 2)
    big = (2.0 - 2.0 ** -7) * 2.0 ** 127                     # largest finite bf16
    cases = [(1.0 + u / 2, 1.0), (1.0 + 3 * u / 2, 1.0 + 2 * u),      # ties go to even
             (1.0 + u / 2 + 2.0 ** -40, 1.0 + u), (1.0 + u / 2 - 2.0 ** -40, 1.0),
             (1.0 + u / 2 + 2.0 ** -30, 1.0 + u),                      # fp32 would round this ONTO the tie, then down
             (1.0 + 3 * u / 2 - 2.0 ** -30, 1.0 + u),                  # ... and this one onto the tie, then up
             (2.0 - u / 2, 2.0), (2.0 - u / 2 - 2.0 ** -40, 2.0 - u), (2.0 + u, 2.0), (2.0 + u + 2.0 ** -40, 2.0 + 2 * u),
             (big, big), (big + 2.0 ** 119, float("inf")), (big + 2.0 ** 119 - 2.0 ** 80, big), (-big - 2.0 ** 119, float("-inf")),
             (1e300, float("inf")), (2.0 ** -133, 2.0 ** -133), (2.0 ** -134, 0.0), (1.5 * 2.0 ** -134, 2.0 ** -133),
             (1e-300, 0.0)]
    x = torch.tensor([c[0] for c in cases], dtype=F64)
    want = torch.tensor([c[1] for c in cases], dtype=F64)
    for sign in (1.0, -1.0):
        got = R.bf16_rne(sign * x)
        assert got.dtype == BF16
        assert torch.equal(got.double(), sign * want), (sign, got.double().tolist(), want.tolist())
    z = R.bf16_rne(torch.tensor([0.0, -0.0, -1e-300], dtype=F64))
    assert R.bits(z).tolist() == [0, -32768, -32768]         # the sign of a zero survives
    assert bool(torch.isnan(R.bf16_rne(torch.tensor([float("nan")], dtype=F64))).all())
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    fin = every[torch.isfinite(every.float())]
    assert torch.equal(R.bits(R.bf16_rne(fin.double())), R.bits(fin))   # every bf16 number is a fixed point


# ------------------------------------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize("M,H", [(5, 520), (3, 2056)])
def test_rmsnorm_reference_is_hf_rmsnorm(M, H):
    x, w, dy, dres = R.norm_rows(M, H, 1, M >= 5), R.norm_weight(H, 2), R.rnd(M, H, seed=3), R.rnd(M, H, seed=4)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = wr * (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + R.EPS_RMS))
    yr.backward(dy)
    y, S, rstd = R.rmsnorm_fwd(x, w)
    close("y", y, yr.detach())
    dx, Sdx, dw, Sdw = R.rmsnorm_bwd(dy, x, w, rstd, dres)
    for i in range(M):                                      # row by row: the rows' scales differ by 1e20
        close(f"dx row {i}", dx[i], xr.grad[i] + dres[i], 1e-11)
    close("dw", dw, wr.grad)
    assert bool((S >= y.abs()).all()) and bool((Sdx >= dx.abs() * (1 - 1e-12)).all()) and bool((Sdw >= dw.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("M,H", [(5, 520), (17, 2048)])
def test_layernorm_reference_is_torch_layer_norm(M, H):
    x, w, b = R.ln_rows(M, H, 1, True), R.norm_weight(H, 2), R.rnd(H, seed=5, scale=0.1)
    dy, dres = R.rnd(M, H, seed=3), R.rnd(M, H, seed=4)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = F.layer_norm(xr, (H,), wr, br, R.EPS_LN)
    yr.backward(dy)
    y, S, mu, Smu, rstd = R.layernorm_fwd(x, w, b)
    close("y", y, yr.detach())
    close("mean", mu, x.mean(-1))
    dx, Sdx, dw, Sdw, db, Sdb = R.layernorm_bwd(dy, x, w, mu, rstd, dres)
    for i in range(M):
        close(f"dx row {i}", dx[i], xr.grad[i] + dres[i], 1e-9 if i == 2 else 1e-11)  # row 2: mean 1024, deviations 8
    close("dw", dw, wr.grad, 1e-10)
    close("db", db, br.grad)
    for ref, s in ((y, S), (mu, Smu), (dx, Sdx), (dw, Sdw), (db, Sdb)):
        assert bool((s >= ref.abs() * (1 - 1e-12)).all())
    assert torch.equal(mu[0], torch.tensor(3.5, dtype=F64)) and torch.equal(y[0], b)   # the constant row


def _rot_half(t):
    h = t.shape[-1] // 2
    return torch.cat([-t[..., h:], t[..., :h]], -1)


@pytest.mark.parametrize("hd", [64, 128])
def test_rotation_and_qknorm_references(hd):
    M, nH, nKV = 5, 3, 1
    pos = torch.tensor([0, 1, 2, 0, 8191])
    ang = R.rope_angles(pos, hd, 10000.0)
    c, s = torch.cos(ang), torch.sin(ang)
    x = R.rnd(M, nH + nKV, hd, seed=1)
    cc, ss = torch.cat([c, c], -1)[:, None], torch.cat([s, s], -1)[:, None]
    out, S = R.rotate(x, c[:, None], s[:, None])
    close("rope", out, x * cc + _rot_half(x) * ss)
    back, _ = R.rotate(out, c[:, None], s[:, None], -1.0)
    close("transpose", back, x)
    assert bool((S >= out.abs() * (1 - 1e-12)).all())
    wq, wk = R.norm_weight(hd, 2), R.norm_weight(hd, 3)
    qs = R.qscale(hd)
    xr, wqr, wkr = (t.clone().requires_grad_(True) for t in (x, wq, wk))
    w = torch.cat([wqr.expand(nH, -1), wkr.expand(nKV, -1)], 0)
    yr = w * (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + R.EPS_RMS))
    scale = torch.cat([torch.full((nH,), qs, dtype=F64), torch.ones(nKV, dtype=F64)])[None, :, None]
    ref = (yr * cc + _rot_half(yr) * ss) * scale
    o, So, rstd = R.qknorm_fwd(x, wq, wk, nH, (c, s, c * qs, s * qs))
    close("qknorm fwd", o, ref.detach())
    dy = R.rnd(M, nH + nKV, hd, seed=4)
    yr.backward(dy)
    dx, Sdx, dwq, Sq, dwk, Sk = R.qknorm_bwd(dy, x, rstd, wq, wk, nH)
    close("qknorm dx", dx, xr.grad, 1e-11)
    close("dw_q", dwq, wqr.grad)
    close("dw_k", dwk, wkr.grad)
    yrow, _ = R.qknorm_rows(x, wq, wk, nH)
    close("rows", yrow, yr.detach())
    for ref_, s_ in ((o, So), (dx, Sdx), (dwq, Sq), (dwk, Sk)):
        assert bool((s_ >= ref_.abs() * (1 - 1e-12)).all())


def test_swiglu_reference_is_silu_times_up():
    g, u, d = R.swiglu_inputs(3, 40, 1)
    gr, ur = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    ref = F.silu(gr) * ur
    ref.backward(d)
    a, Sa = R.swiglu_fwd(g, u)
    dg, Sg, du, Su = R.swiglu_bwd(g, u, d)
    close("act", a, ref.detach())
    close("dgate", dg, gr.grad, 1e-11)
    close("dup", du, ur.grad)
    assert bool((Sg >= dg.abs() * (1 - 1e-12)).all())
    assert bool((a[:, :2] == 0).all()) and bool((du[:, :2] == 0).all()) and bool((a[:, 5] == 0).all())
    R.assert_normal("g = -60", a[:, 3][a[:, 3] != 0])        # 60 e^-60 u is far above 2^-120


@pytest.mark.parametrize("V,Vp", [(502, 512), (2049, 2056)])
@pytest.mark.parametrize("eps", [0.0, R.EPS_SMOOTH])
@pytest.mark.parametrize("num_items", [0.0, 57.0])
def test_cross_entropy_reference_is_torch_cross_entropy(V, Vp, eps, num_items):
    B, T = 3, 7
    z, lab, _ = R.ce_case(B, T, V, Vp, 1, pad=float("nan"))
    r = R.cross_entropy(z, lab, V, num_items, eps)
    tgt = r["tgt"].clone()
    tgt[tgt < 0] = -100
    zr = z[:, :V].clone().requires_grad_(True)
    tot = F.cross_entropy(zr, tgt, ignore_index=-100, reduction="sum", label_smoothing=eps)
    (tot / r["denom"]).backward()
    close("loss", r["loss"][0], (tot / r["denom"]).detach().reshape(1))
    close("dlogits", r["dlogits"][0][:, :V], zr.grad, 1e-11)
    assert bool((r["dlogits"][0][:, V:] == 0).all())
    nll = F.cross_entropy(z[:, :V], tgt, ignore_index=-100, reduction="none")
    close("row_loss", r["row_loss"][0], nll)
    assert r["denom"] == (57.0 if num_items else float(((tgt != -100).sum()) + 2)) == (57.0 if num_items else 10.0)  # the two out-of-range labels count
    for k in ("dlogits", "row_loss", "row_smooth", "loss"):
        assert bool((r[k][1] >= r[k][0].abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------------------------------------ fp32 restatements
def f32(t):
    return t.numpy().astype(np.float32)


def seqsum(a, axis=-1, keepdims=False):
    """strictly sequential fp32 sum"""
    s = np.take(np.cumsum(a.astype(np.float32), axis=axis, dtype=np.float32), -1, axis=axis)
    return np.expand_dims(s, axis) if keepdims else s


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32).copy())


def as_bf16(a):
    """fp32 array -> bf16 with one rounding (fp32 -> bf16 in torch is a single RNE)."""
    return t64(a).to(BF16)


@pytest.mark.parametrize("M,H", [(5, 520), (35, 2056)])
def test_fp32_rmsnorm_meets_the_rule(M, H):
    x, w, dy, dres = R.norm_rows(M, H, 1, True), R.norm_weight(H, 2), R.rnd(M, H, seed=3), R.rnd(M, H, seed=4)
    xf, wf, dyf, drf = f32(x), f32(w), f32(dy), f32(dres)
    r = (np.float32(1) / np.sqrt(seqsum(xf * xf) / np.float32(H) + np.float32(R.EPS_RMS))).astype(np.float32)
    yf = xf * r[:, None] * wf
    y, S, rstd = R.rmsnorm_fwd(x, w)
    assert R.accept_bf16("fp32 rmsnorm y", as_bf16(yf), y, S) == 0
    assert R.accept_f32("fp32 rstd", t64(r), rstd, rstd) == 0
    xh, g = xf * r[:, None], dyf * wf
    dot = seqsum(g * xh, keepdims=True) / np.float32(H)
    dxf = r[:, None] * (g - xh * dot) + drf
    dwf = seqsum(dyf * xh, axis=0)
    dx, Sdx, dw, Sdw = R.rmsnorm_bwd(dy, x, w, t64(r).double(), dres)
    assert R.accept_bf16("fp32 rmsnorm dx", as_bf16(dxf), dx, Sdx) == 0
    assert R.accept_f32("fp32 rmsnorm dw", t64(dwf), dw, Sdw, R.delta_sum(M)) == 0


@pytest.mark.parametrize("M,H", [(5, 520), (17, 2048)])
def test_fp32_layernorm_meets_the_rule(M, H):
    x, w, b = R.ln_rows(M, H, 1, True), R.norm_weight(H, 2), R.rnd(H, seed=5, scale=0.1)
    dy, dres = R.rnd(M, H, seed=3), R.rnd(M, H, seed=4)
    xf, wf, bf, dyf, drf = f32(x), f32(w), f32(b), f32(dy), f32(dres)
    mu = seqsum(xf, keepdims=True) / np.float32(H)
    r = (np.float32(1) / np.sqrt(seqsum((xf - mu) * (xf - mu), keepdims=True) / np.float32(H) + np.float32(R.EPS_LN))).astype(np.float32)
    yf = (xf - mu) * r * wf + bf
    y, S, m64, Sm, rstd = R.layernorm_fwd(x, w, b)
    assert R.accept_bf16("fp32 ln y", as_bf16(yf), y, S) == 0
    assert R.accept_f32("fp32 ln mean", t64(mu[:, 0]), m64, Sm) == 0
    assert R.accept_f32("fp32 ln rstd", t64(r[:, 0]), rstd, rstd) == 0
    xh, g = (xf - mu) * r, dyf * wf
    gm, c2 = seqsum(g, keepdims=True) / np.float32(H), seqsum(g * xh, keepdims=True) / np.float32(H)
    dxf = r * (g - gm - xh * c2) + drf
    dx, Sdx, dw, Sdw, db, Sdb = R.layernorm_bwd(dy, x, w, t64(mu[:, 0]).double(), t64(r[:, 0]).double(), dres)
    assert R.accept_bf16("fp32 ln dx", as_bf16(dxf), dx, Sdx) == 0
    assert R.accept_f32("fp32 ln dw", t64(seqsum(dyf * xh, axis=0)), dw, Sdw, R.delta_sum(M)) == 0
    assert R.accept_f32("fp32 ln db", t64(seqsum(dyf, axis=0)), db, Sdb, R.delta_sum(M)) == 0


@pytest.mark.parametrize("hd", [64, 128])
def test_fp32_qknorm_and_rope_meet_the_rule(hd):
    M, nH, nKV, half = 37, 3, 1, hd // 2
    pos = torch.arange(M) % 13
    ang = R.rope_angles(pos, hd, 10000.0)
    cf, sf = np.cos(f32(ang)), np.sin(f32(ang))          # fp32 tables: the reference takes them as they are
    qs = np.float32(R.qscale(hd))
    tabs = tuple(t64(a).double() for a in (cf, sf, cf * qs, sf * qs))
    x, wq, wk = R.rnd(M, nH + nKV, hd, seed=1), R.norm_weight(hd, 2), R.norm_weight(hd, 3)
    x[0, 0], x[M - 1, nH] = 0.0, 0.0
    xf = f32(x)
    wf = np.concatenate([np.repeat(f32(wq)[None], nH, 0), np.repeat(f32(wk)[None], nKV, 0)], 0)
    r = (np.float32(1) / np.sqrt(seqsum(xf * xf) / np.float32(hd) + np.float32(R.EPS_RMS))).astype(np.float32)
    yf = xf * r[..., None] * wf

    def rot(y, c, s):
        lo, hi = y[..., :half], y[..., half:]
        return np.concatenate([lo * c - hi * s, hi * c + lo * s], -1)
    of = np.concatenate([rot(yf[:, :nH], (cf * qs)[:, None], (sf * qs)[:, None]), rot(yf[:, nH:], cf[:, None], sf[:, None])], 1)
    o, So, rstd = R.qknorm_fwd(x, wq, wk, nH, tabs)
    assert R.accept_bf16("fp32 qknorm fwd", as_bf16(of), o, So) == 0
    assert R.accept_f32("fp32 qknorm rstd", t64(r), rstd, rstd) == 0
    yr, Sr = R.qknorm_rows(x, wq, wk, nH)
    assert R.accept_f32("fp32 qknorm rows", t64(yf), yr, Sr) == 0
    dy = R.rnd(M, nH + nKV, hd, seed=4)
    dyf = f32(dy)
    xh, g = xf * r[..., None], dyf * wf
    dot = seqsum(g * xh, keepdims=True) / np.float32(hd)
    dxf = r[..., None] * (g - xh * dot)
    dx, Sdx, dwq, Sq, dwk, Sk = R.qknorm_bwd(dy, x, t64(r).double(), wq, wk, nH)
    assert R.accept_bf16("fp32 qknorm dx", as_bf16(dxf), dx, Sdx) == 0
    t = (dyf * xh)
    assert R.accept_f32("fp32 dw_q", t64(seqsum(t[:, :nH].reshape(-1, hd), axis=0)), dwq, Sq, R.delta_sum(M * nH)) == 0
    assert R.accept_f32("fp32 dw_k", t64(seqsum(t[:, nH:].reshape(-1, hd), axis=0)), dwk, Sk, R.delta_sum(M * nKV)) == 0
    for sign in (1.0, -1.0):                              # plain RoPE, forward and transpose
        ref, S = R.rotate(x, tabs[0][:, None], tabs[1][:, None], sign)
        assert R.accept_bf16("fp32 rope", as_bf16(rot(xf, cf[:, None], sf[:, None] * np.float32(sign))), ref, S) == 0
    # the fp32 tables themselves meet the table bound
    assert bool(((tabs[0] - torch.cos(ang)).abs() <= R.table_bound(ang)).all())
    assert bool(((tabs[1] - torch.sin(ang)).abs() <= R.table_bound(ang)).all())


def test_fp32_swiglu_meets_the_rule():
    g, u, d = R.swiglu_inputs(7, 4864, 1)
    gf, uf, df = f32(g), f32(u), f32(d)
    sg = (np.float32(1) / (np.float32(1) + np.exp(-gf))).astype(np.float32)
    a, Sa = R.swiglu_fwd(g, u)
    dg, Sg, du, Su = R.swiglu_bwd(g, u, d)
    assert R.accept_bf16("fp32 swiglu act", as_bf16(gf * sg * uf), a, Sa) == 0
    assert R.accept_bf16("fp32 swiglu dup", as_bf16(df * (gf * sg)), du, Su) == 0
    assert R.accept_bf16("fp32 swiglu dgate", as_bf16(df * uf * sg * (np.float32(1) + gf * (np.float32(1) - sg))), dg, Sg) == 0


def _fp32_ce(zf, tgt, V, denom, eps):
    zz = zf[:, :V]
    mx = zz.max(-1, keepdims=True)
    e = np.exp(zz - mx).astype(np.float32)
    s = seqsum(e, keepdims=True)
    lse = (mx + np.log(s)).astype(np.float32)
    oh = np.zeros_like(zz)
    rows = np.nonzero(tgt >= 0)[0]
    oh[rows, tgt[rows]] = 1
    p = e * (np.float32(1) / s)
    e32 = np.float32(eps)
    d = np.zeros_like(zf)
    d[:, :V] = (p - e32 / np.float32(V) - (np.float32(1) - e32) * oh) * (np.float32(1) / np.float32(denom))
    d[tgt < 0] = 0
    valid = (tgt >= 0).astype(np.float32)
    rl = (lse[:, 0] - seqsum(zz * oh)) * valid
    rs = (lse[:, 0] - seqsum(zz) / np.float32(V)) * valid
    return d, rl, rs


@pytest.mark.parametrize("V,Vp", [(502, 512), (2049, 2056)])
@pytest.mark.parametrize("eps", [0.0, R.EPS_SMOOTH])
def test_fp32_cross_entropy_meets_the_rule(V, Vp, eps):
    B, T = 3, 7
    z, lab, under = R.ce_case(B, T, V, Vp, 1)
    r = R.cross_entropy(z, lab, V, 57.0, eps)
    d, rl, rs = _fp32_ce(f32(z), r["tgt"].numpy(), V, 57.0, eps)
    keep = torch.ones(B * T, dtype=torch.bool)
    keep[under] = False
    ref, S = r["dlogits"]
    assert R.accept_bf16("fp32 ce dlogits", as_bf16(d)[keep], ref[keep], S[keep]) == 0
    assert R.accept_bf16("fp32 ce dlogits, saturated rows", as_bf16(d)[~keep], ref[~keep], S[~keep], underflow=True) == 0
    assert R.accept_f32("fp32 ce row_loss", t64(rl), *r["row_loss"]) == 0
    assert R.accept_f32("fp32 ce row_smooth", t64(rs), *r["row_smooth"]) == 0


def test_fp32_colsum_meets_the_rule():
    X = R.rnd(1025, 136, seed=1)
    ref, S = R.colsum(X)
    assert R.accept_f32("fp32 colsum", t64(seqsum(f32(X), axis=0)), ref, S, R.delta_sum(1025)) == 0


# ------------------------------------------------------------------------------------------------ mutants
def _check_passes(name, got, ref, rms, mx):
    from tests.gpu_util import check
    try:
        check(name, got, ref, rms, mx)
        return True
    except AssertionError:
        return False


def test_the_rule_rejects_mutants_and_check_is_recorded():
    """Each mutant is applied to the float64 reference, rounded once, and must fail the rule. tests/gpu_util.check at the
    tolerances tests/test_gpu_ops.py uses for the same output is run on it too; whether it lets the mutant through is printed
    and kept in profiles/row_exact.md. Mutants 1 and 2 are asserted to PASS `check` (they are why this file exists); for 3 - 5
    the outcome is recorded only."""
    M, H = 16, 2048
    x, w = R.rnd(M, H, seed=1), R.norm_weight(H, 2)
    y, S, rstd = R.rmsnorm_fwd(x, w)
    good = R.bf16_rne(y)
    assert R.accept_bf16("unmutated", good, y, S) == 0
    seen = {}
    # 1. double rounding: the fp32 value truncated to 12 mantissa bits, then rounded to bf16
    t = (y.float().view(torch.int32) & ~0x7FF).view(torch.float32)
    m1 = t.to(BF16)
    assert R.accept_bf16("mutant 1 double rounding", m1, y, S) > 0
    seen[1] = _check_passes("m1", m1.float(), y, 3e-3, 1e-2)
    # 2. one 8-column chunk dropped from the row statistic
    r2 = ((x.pow(2).sum(-1) - x[:, 512:520].pow(2).sum(-1)) / H + R.EPS_RMS).pow(-0.5)
    m2 = R.bf16_rne(x * r2[:, None] * w)
    assert R.accept_bf16("mutant 2 dropped chunk", m2, y, S) > 0
    seen[2] = _check_passes("m2", m2.float(), y, 3e-3, 1e-2)
    # 3. the neighbouring row's rstd
    m3 = R.bf16_rne(x * rstd.roll(1)[:, None] * w)
    assert R.accept_bf16("mutant 3 neighbour rstd", m3, y, S) > 0
    seen[3] = _check_passes("m3", m3.float(), y, 3e-3, 1e-2)
    # 4. p in place of p - 1 at the target
    B, T, V, Vp = 3, 41, 502, 512
    z = R.logits_rows(B * T, V, Vp, 1, scale=3.0)
    lab = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(2))
    r = R.cross_entropy(z, lab, V, 0.0)
    d, Sd = r["dlogits"]
    rows = r["valid"].nonzero()[:, 0]
    d4 = d.clone()
    d4[rows, r["tgt"][rows]] += 1.0 / r["denom"]
    assert R.accept_bf16("unmutated ce", R.bf16_rne(d), d, Sd) == 0
    m4 = R.bf16_rne(d4)
    assert R.accept_bf16("mutant 4 p for p - 1", m4, d, Sd) > 0
    seen[4] = _check_passes("m4", m4.float()[:, :V], d[:, :V], 5e-3, 2e-2)
    # 5. the RoPE partner shifted by one column
    hd = 64
    q = R.rnd(150, 6, hd, seed=3)
    ang = R.rope_angles(torch.arange(150) % 75, hd, 10000.0)
    c, s = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
    ref, Sr = R.rotate(q, c, s)
    lo, hi = q[..., :hd // 2], q[..., hd // 2:]
    m5 = R.bf16_rne(torch.cat([lo * c - hi.roll(1, -1) * s, hi * c + lo.roll(1, -1) * s], -1))
    assert R.accept_bf16("mutant 5 shifted partner", m5, ref, Sr) > 0
    seen[5] = _check_passes("m5", m5.float(), ref, 3e-3, 1e-2)
    print("[row-exact] mutants that tests/gpu_util.check lets through:", {k: v for k, v in seen.items()})
    assert seen[1] and seen[2], seen
