"""Float64 references, input generators and the acceptance rule for the row kernels of slamkit_amd/csrc/elementwise.hip
(RMSNorm narrow and wide, LayerNorm, Qwen3's q/k norm, RoPE, SwiGLU, the two cross-entropy kernels, the column sums).
No GPU is needed to import or run anything here except `guarded`, which only allocates on the device it is given.

THE RULE. These kernels read bf16, compute in fp32 and round once. Write the float64 value of an output element as a sum of
terms, ref = sum_i t_i (most outputs are one product; the ones that cancel have several), and S = sum_i |t_i|. The kernel's
fp32 value is ref + e with |e| <= DELTA S, followed by ONE round-to-nearest-even to bf16. Rounding is monotonic, so

    lo = bf16_rne(ref - DELTA S),  hi = bf16_rne(ref + DELTA S),  lo <= got <= hi      for every element

is exact: no tolerance on the bf16 side at all. fp32 outputs (rstd, mean, dw, db, row_loss, row_smooth, the loss, the column
sums, qknorm_rows_f32) are held to |got - ref| <= DELTA S with the same S; for a sum over rows S is the sum of the absolute
terms.

DELTA = 2^-16 for every kernel. The budget: fp32 unit roundoff is 2^-24; a row reduction is at most 32 sequential adds per
lane, 6 butterfly steps and the LDS adds, under 48 roundoffs = 2.9e-6; rsqrtf, rcp, v_exp_f32 and logf cost one or two ulp
each; __expf(x) and fast_sigmoid(x) multiply the argument by log2(e) first, which costs |x| 1.44 2^-24 ln 2 = 5e-6 at
|x| = 83 (below that the result is under 2^-120). The sum is about 1e-5 < 2^-16 = 1.5e-5. Sums over M rows (column sums,
dw, db) use DELTA_SUM = M 2^-24 + 2^-16, the strictly sequential worst case - legitimate because S is the sum of absolute
terms. DELTA is a property of this reference, not of the kernels: tests/test_row_exact_host.py runs an fp32 restatement of
every formula with strictly sequential reductions through the same rule and requires 0 violations.

Rows longer than that budget (the real vocabulary: Vp = 152,320 is 75 steps of 8 columns for each of ce_big_kernel's 256
threads) get DELTA as a function of the per-lane step count n, delta_steps(n), derived the same way. A step of 8 columns costs
a lane's running value at most 8 roundoffs: the plain sums (the smoothing term sum_v z_v) add 8 terms, and the online softmax
sum pays 8 adds inside the step for the terms that join and, for the ones already there, one product with exp(old max - new
max), one add and the two ulp of that exp (4 <= 8; the ARGUMENT errors of the rescaling exps telescope: old max - new max summed
over the steps is at most row max - z, the argument the single exp of the budget above already pays for). So a lane pays at
most 8 n roundoffs where the budget above carries 32, and delta_steps(n) = DELTA + max(0, 8 n - 32) 2^-24: DELTA itself up to
n = 4 (every case of test_gpu_row_exact.py: Vp <= 4104 is 3 steps), 2^-16 + 568 2^-24 = 4.9e-5 at n = 75. Legitimate for the same
reason as DELTA_SUM: S is the sum of the absolute terms, and every term of these sums passes through at most that many
roundings. tests/test_far_rows_host.py proves it the way test_row_exact_host.py proves DELTA: an fp32 restatement with every
lane strictly sequential, at Vp = 152,320, 0 violations.

One term the budget above does not carry, found by the -3e4 cross-entropy row: a kernel that forms p = exp(z - lse) with
lse = max + log(sum) rounded to fp32 pays half an ulp of |lse| in the EXPONENT, i.e. a relative error ulp(|lse|) / 2 in p.
That is 1.9e-6 at |lse| < 64 (inside the budget) and 1e-3 at |lse| = 3e4 (not). The rule does not grow to admit it; the
kernel must form p = exp(z - max) / sum (profiles/row_exact.md).

Underflow: where |ref| < 2^-120 the kernel's exp may flush, so any |got| <= 2^-120 passes - only in the cases that ask for it
(`underflow=True`: the saturated softmax rows). Every other call asserts ON THE REFERENCE that no non-zero element is that
small; the generators keep normal outputs away from it (logits within 60 of the row max, gate pre-activations within 60).

Inputs: all bf16-representable. Norm rows have magnitude at most 2^40: above 2^63 the sum of squares overflows fp32 in the
kernel and in HF alike - that is the contract, not a finding.

bf16_rne rounds the float64 value ONCE. (torch's double -> bfloat16 cast goes through fp32 first and so rounds twice; a value
just above a bf16 tie can land on the tie in fp32 and then round the wrong way. bf16_rne goes through fp32 with round-to-odd,
which keeps the information the second rounding needs.)"""
import math

import numpy as np
import torch

DELTA = 2.0 ** -16
TINY = 2.0 ** -120
GUARD = 256                                   # elements in each band
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS_RMS = float(np.float32(1e-6))             # the kernels take eps as a float
EPS_LN = float(np.float32(1e-5))
EPS_SMOOTH = float(np.float32(0.1))
BAND_BITS = {BF16: 0x7FD5, F32: 0x7FD5AAAA}   # NaN payloads no kernel produces


def delta_sum(M):
    return M * 2.0 ** -24 + DELTA


def delta_steps(n):
    """DELTA for a row whose lanes run n sequential steps of 8 columns (the module docstring derives it); DELTA up to n = 4."""
    return DELTA + max(0, 8 * int(n) - 32) * 2.0 ** -24


def ce_big_steps(Vp):
    """Steps per thread of ce_big_kernel: 16-byte chunks of a row dealt round-robin to 256 threads."""
    return -(-(Vp // 8) // 256)


# ------------------------------------------------------------------------------------------------ rounding and the rule
def bf16_rne(x64):
    """float64 -> bfloat16 with a single round-to-nearest-even (NaN stays NaN, overflow goes to inf); on x64's device."""
    x = x64.detach().to(F64).contiguous()
    f = x.to(F32)                                       # RNE to fp32; inf beyond the fp32 range
    b = f.view(torch.int32).clone()
    fx = f.double()
    nan = torch.isnan(x)
    away = (fx.abs() > x.abs()) & ~nan                  # fp32 rounded away from zero (inf included): step back to the truncation
    b = torch.where(away, b - 1, b)                     # (the sign bit is the top bit: - 1 shrinks the magnitude for either sign)
    inexact = (fx != x) & ~nan
    b = torch.where(inexact, b | 1, b)                  # round to odd: the sticky bit survives
    u = b.long() & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(nan, torch.full_like(r, 0x7FC0), r)
    r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
    return r.view(BF16).reshape(x64.shape)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_normal(name, ref):
    small = (ref != 0) & (ref.abs() < TINY)
    assert not bool(small.any()), f"{name}: {int(small.sum())} reference elements are non-zero below 2^-120 outside an underflow case"


def accept_bf16(name, got, ref, S, delta=DELTA, underflow=False, report=True):
    """The rule for a bf16 output. Returns the number of violations (0 to pass); prints the flip share."""
    ref, S = ref.detach().to(F64), S.detach().to(F64, copy=False).to(ref.device)
    got = got.detach().to(ref.device)
    assert got.dtype == BF16 and got.shape == ref.shape == S.shape, (name, got.dtype, got.shape, ref.shape, S.shape)
    assert bool((S >= ref.abs() * (1 - 1e-12)).all()), f"{name}: S < |ref|"
    if not underflow:
        assert_normal(name, ref)
    g = got.double()
    lo, hi = bf16_rne(ref - delta * S).double(), bf16_rne(ref + delta * S).double()
    ok = (lo <= g) & (g <= hi)
    if underflow:
        ok |= (ref.abs() < TINY) & (g.abs() <= TINY)
    bad = int((~ok).sum())
    if report:
        flips = float((g != bf16_rne(ref).double()).double().mean())
        two = float((lo != hi).double().mean())
        msg = f"[row-exact] {name}: n={got.numel()} flips={flips:.3e} two-member={two:.3e} violations={bad}"
        if bad:
            i = int((~ok).reshape(-1).nonzero()[0])
            msg += (f" first at flat {i}: got {float(g.reshape(-1)[i])!r} not in [{float(lo.reshape(-1)[i])!r}, "
                    f"{float(hi.reshape(-1)[i])!r}] ref {float(ref.reshape(-1)[i])!r} S {float(S.reshape(-1)[i])!r}")
        print(msg)
    return bad


def accept_f32(name, got, ref, S, delta=DELTA, report=True):
    """The rule for an fp32 output: |got - ref| <= delta S. Returns the number of violations; prints the worst |err| / S."""
    ref, S = ref.detach().to(F64), S.detach().to(F64, copy=False).to(ref.device)
    got = got.detach().to(ref.device)
    assert got.dtype == F32 and got.shape == ref.shape == S.shape, (name, got.dtype, got.shape, ref.shape, S.shape)
    assert bool((S >= ref.abs() * (1 - 1e-12)).all()), f"{name}: S < |ref|"
    err = (got.double() - ref).abs()
    ok = err <= delta * S                              # NaN fails
    bad = int((~ok).sum())
    if report:
        nz = S > 0
        worst = float((err[nz] / S[nz]).max()) if bool(nz.any()) else 0.0
        print(f"[row-exact] {name}: n={got.numel()} worst |err|/S={worst:.3e} (bound {delta:.3e}) violations={bad}")
    return bad


# ------------------------------------------------------------------------------------------------ buffers
def guarded(shape, dtype, device, fill=None):
    """A payload of `shape` inside one flat allocation with GUARD-element bands before and behind it, every band element
    holding BAND_BITS. The payload starts as NaN (`fill` = a tensor to copy in instead: a poisoned operand).
    Returns (payload view, check); check(name) raises if a band changed."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(math.prod(shape))
    it = {BF16: torch.int16, F32: torch.int32}[dtype]
    sent = BAND_BITS[dtype] if dtype == F32 else BAND_BITS[dtype] - 0x10000 * (BAND_BITS[dtype] >= 0x8000)
    buf = torch.full((n + 2 * GUARD,), sent, dtype=it, device=device)
    payload = buf[GUARD:GUARD + n].view(dtype).view(shape)
    if fill is None:
        payload.fill_(float("nan"))
    else:
        payload.copy_(fill.to(dtype))

    def check(name):
        assert bool((buf[:GUARD] == sent).all()), f"{name}: the band before the buffer was written"
        assert bool((buf[GUARD + n:] == sent).all()), f"{name}: the band behind the buffer was written"
    return payload, check


def workspace(nbytes, device):
    """fp32 workspace of exactly nbytes rounded up to 16, NaN-filled, between bands."""
    return guarded(((int(nbytes) + 15) // 16) * 4, F32, device)


# ------------------------------------------------------------------------------------------------ generators
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16).double()


def norm_rows(M, H, seed, special):
    """N(0,1) rows with per-row scales 1e-3, 1, 50; with `special`: an all-zero row first, a 2^-60 row and a row with one
    2^20 element inside, a row of -0.0 last (M >= 5)."""
    x = rnd(M, H, seed=seed)
    sc = torch.tensor([1.0, 1e-3, 50.0], dtype=F64)[torch.arange(M) % 3].to(BF16).double()
    x = (x * sc[:, None]).to(BF16).double()
    if special:
        assert M >= 5
        x[0] = 0.0
        x[2] = 2.0 ** -60
        x[3] = rnd(H, seed=seed + 100)
        x[3, (H // 2) | 1 if H > 1 else 0] = 2.0 ** 20
        x[M - 1] = -0.0
    return x


def ln_rows(M, H, seed, special):
    """As norm_rows, with LayerNorm's special rows: a constant row first, a row from {1016, 1024, 1032} inside (large mean,
    small variance), an all-zero row last."""
    x = rnd(M, H, seed=seed)
    sc = torch.tensor([1.0, 1e-3, 50.0], dtype=F64)[torch.arange(M) % 3].to(BF16).double()
    x = (x * sc[:, None] + sc[:, None] * 0.5).to(BF16).double()
    if special:
        assert M >= 5
        x[0] = 3.5
        g = torch.Generator().manual_seed(seed + 7)
        x[2] = 1016.0 + 8.0 * torch.randint(0, 3, (H,), generator=g).double()
        x[M - 1] = 0.0
    return x


def norm_weight(H, seed):
    return (1.0 + 0.1 * rnd(H, seed=seed)).to(BF16).double()


def logits_rows(M, V, Vp, seed, scale=8.0, clamp=30.0, pad=0.0):
    """bf16 logits [M][Vp]: valid columns N(0, scale) clamped to +-clamp (every |z - max| <= 2 clamp = 60), pads = `pad`."""
    z = torch.full((M, Vp), float(pad), dtype=F64)
    z[:, :V] = rnd(M, V, seed=seed, scale=scale).clamp(-clamp, clamp)
    return z


# ------------------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_fwd(x, w, eps=EPS_RMS):
    """-> (y, S_y, rstd). y = x rstd w (one term); rstd = (mean x^2 + eps)^-1/2 (S = rstd)."""
    rstd = (x.pow(2).mean(-1) + eps).pow(-0.5)
    y = x * rstd[..., None] * w
    return y, y.abs(), rstd


def rmsnorm_bwd(dy, x, w, rstd, dres=None):
    """rstd is an INPUT (the forward's fp32 value, as float64). -> (dx, S_dx, dw, S_dw).
    dx terms: rstd dy w, -rstd xhat dot, dres with dot = mean(dy w xhat); dw = sum_m dy xhat."""
    r = rstd[..., None]
    xh, g = x * r, dy * w
    dot = (g * xh).mean(-1, keepdim=True)
    t1, t2 = r * g, -r * xh * dot
    dx, S = t1 + t2, t1.abs() + t2.abs()
    if dres is not None:
        dx, S = dx + dres, S + dres.abs()
    lead = tuple(range(dy.dim() - 1))
    return dx, S, (dy * xh).sum(lead), (dy * xh).abs().sum(lead)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, w, b, eps=EPS_LN):
    """-> (y, S_y, mean, S_mean, rstd). y terms: x rstd w, -mu rstd w, b; mean terms x_i / H."""
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).pow(-0.5)
    y = (x - mu) * rstd * w + b
    S = (x.abs() + mu.abs()) * rstd * w.abs() + b.abs()
    return y, S, mu[..., 0], x.abs().mean(-1), rstd[..., 0]


def layernorm_bwd(dy, x, w, mean, rstd, dres=None):
    """mean, rstd are INPUTS. -> (dx, S_dx, dw, S_dw, db, S_db).
    dx terms: rstd g, -rstd mean(g), -rstd xhat mean(g xhat), dres; the two terms of x - mu are carried through xhat."""
    mu, r = mean[..., None], rstd[..., None]
    xh, xh_abs = (x - mu) * r, (x.abs() + mu.abs()) * r
    g = dy * w
    gm, c2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dx = r * (g - gm - xh * c2)
    S = r * g.abs() + r * gm.abs() + r * xh_abs * c2.abs()
    if dres is not None:
        dx, S = dx + dres, S + dres.abs()
    return dx, S, (dy * xh).sum(0), (dy.abs() * xh_abs).sum(0), dy.sum(0), dy.abs().sum(0)


# ------------------------------------------------------------------------------------------------ rotate-half, RoPE, q/k norm
def rope_angles(pos, hd, theta):
    """float64 angles [M][hd/2] = pos theta^(-2 d / hd)."""
    d = torch.arange(hd // 2, dtype=F64)
    return pos.double()[:, None] * torch.pow(torch.tensor(float(theta), dtype=F64), -2.0 * d / hd)[None, :]


def table_bound(angle):
    """|table - cos/sin(angle)|: powf at 2 ulp, the divide and the product at half an ulp each, sincosf at 2 ulp."""
    return angle.abs() * 2.0 ** -22 + 2.0 ** -22


def rotate(y, c, s, sign=1.0):
    """y [..., hd], c / s [..., hd/2] (broadcastable). -> (out, S). lo' = lo c - hi s, hi' = hi c + lo s (sign = -1: transpose).
    Terms: y c and partner s."""
    half = y.shape[-1] // 2
    lo, hi = y[..., :half], y[..., half:]
    s = s * sign
    out = torch.cat([lo * c - hi * s, hi * c + lo * s], -1)
    S = torch.cat([(lo * c).abs() + (hi * s).abs(), (hi * c).abs() + (lo * s).abs()], -1)
    return out, S


def qscale(hd):
    """head_dim^-0.5 log2(e) as the entry point forms it in fp32."""
    return float(np.float32(1.44269504088896340736) / np.sqrt(np.float32(hd)))


def qknorm_fwd(x, wq, wk, nH, tabs, eps=EPS_RMS):
    """x [M][nH + nKV][hd]; tabs = (cs, sn, csq, snq) [M][hd/2] as the kernel built them (float64 of its fp32 values).
    -> (out, S, rstd [M][nH + nKV])."""
    cs, sn, csq, snq = tabs
    rstd = (x.pow(2).mean(-1) + eps).pow(-0.5)
    w = torch.cat([wq.expand(nH, -1), wk.expand(x.shape[1] - nH, -1)], 0)
    y = x * rstd[..., None] * w
    oq, Sq = rotate(y[:, :nH], csq[:, None], snq[:, None])
    ok, Sk = rotate(y[:, nH:], cs[:, None], sn[:, None])
    return torch.cat([oq, ok], 1), torch.cat([Sq, Sk], 1), rstd


def qknorm_bwd(dy, raw, rstd, wq, wk, nH):
    """dy, raw [M][nQK][hd], rstd [M][nQK] an INPUT. -> (dx, S, dwq, S_dwq, dwk, S_dwk)."""
    w = torch.cat([wq.expand(nH, -1), wk.expand(raw.shape[1] - nH, -1)], 0)
    dx, S, _, _ = rmsnorm_bwd(dy, raw, w, rstd)
    t = dy * raw * rstd[..., None]
    return dx, S, t[:, :nH].sum((0, 1)), t[:, :nH].abs().sum((0, 1)), t[:, nH:].sum((0, 1)), t[:, nH:].abs().sum((0, 1))


def qknorm_rows(x, wq, wk, nH, eps=EPS_RMS):
    """fp32 rows: y = x rstd w, no rotation. -> (y, S)."""
    rstd = (x.pow(2).mean(-1) + eps).pow(-0.5)
    w = torch.cat([wq.expand(nH, -1), wk.expand(x.shape[1] - nH, -1)], 0)
    y = x * rstd[..., None] * w
    return y, y.abs()


# ------------------------------------------------------------------------------------------------ SwiGLU
def swiglu_fwd(g, u):
    a = g * torch.sigmoid(g) * u
    return a, a.abs()


def swiglu_bwd(g, u, d):
    """-> (dgate, S_dgate, dup, S_dup). dgate terms: d u sg and d u sg g (1 - sg)."""
    sg = torch.sigmoid(g)
    one_m = torch.sigmoid(-g)                      # 1 - sg without cancellation
    t1 = d * u * sg
    t2 = t1 * g * one_m
    du = d * g * sg
    return t1 + t2, t1.abs() + t2.abs(), du, du.abs()


def swiglu_inputs(M, I, seed):
    """gate N(0, 3) clamped to +-60, up N(0, 1); in every row (I >= 8) columns 0..5 hold g = 0, -0.0, 60, -60, -1.2785 (the zero
    of the dgate factor) and u = 0."""
    g = rnd(M, I, seed=seed, scale=3.0).clamp(-60, 60)
    u = rnd(M, I, seed=seed + 1)
    sp = torch.tensor([0.0, -0.0, 60.0, -60.0, -1.2785], dtype=F64).to(BF16).double()
    g[:, :5] = sp
    u[:, 5] = 0.0
    return g, u, rnd(M, I, seed=seed + 2)


# ------------------------------------------------------------------------------------------------ cross entropy
def ce_targets(labels, V):
    """labels [B][T] -> (tgt [B*T] with -1 where the row is not scored, denom count): row m = (b, t) is scored against
    labels[b][t + 1]; the last position of a batch row never is. A label outside [0, V) gives a zero row; the count of valid
    targets counts every label that is not -100, as the kernel does."""
    B, T = labels.shape
    nxt = torch.full((B, T), -100, dtype=torch.int64)
    nxt[:, :-1] = labels[:, 1:]
    count = int((nxt != -100).sum())
    tgt = torch.where((nxt >= 0) & (nxt < V), nxt, torch.full_like(nxt, -1))
    return tgt.reshape(-1), count


def cross_entropy_rows(z, tgt, V, denom, eps=0.0):
    """The per-row part of `cross_entropy` for any run of rows, on z's device: z [rows][Vp] float64, tgt [rows] (ce_targets'
    numbering: -1 = not scored), denom fixed beforehand. -> dict of (ref, S) pairs: dlogits, row_loss, row_smooth; valid."""
    M, Vp = z.shape
    tgt = tgt.to(z.device)
    valid = tgt >= 0
    zz = z[:, :V]
    mx = zz.max(-1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(zz - mx).sum(-1, keepdim=True)))[:, 0]
    p = torch.exp(zz - lse[:, None])
    onehot = torch.zeros(M, V, dtype=F64, device=z.device)
    rows = valid.nonzero()[:, 0]
    onehot[rows, tgt[rows]] = 1.0
    zy = (zz * onehot).sum(-1)
    d = torch.zeros(M, Vp, dtype=F64, device=z.device)
    Sd = torch.zeros(M, Vp, dtype=F64, device=z.device)
    if denom > 0:
        d[:, :V] = (p - (1.0 - eps) * onehot - eps / V) / denom
        Sd[:, :V] = (p + (1.0 - eps) * onehot + eps / V) / denom
    d[~valid], Sd[~valid] = 0.0, 0.0
    v = valid.double()
    row_loss, S_rl = (lse - zy) * v, (lse.abs() + zy.abs()) * v
    zm = zz.mean(-1)
    row_smooth, S_rs = (lse - zm) * v, (lse.abs() + zm.abs()) * v
    return {"dlogits": (d, Sd), "row_loss": (row_loss, S_rl), "row_smooth": (row_smooth, S_rs), "valid": valid}


def cross_entropy(z, labels, V, num_items, eps=0.0):
    """z [M][Vp] float64 (columns >= V are outside the softmax, whatever they hold).
    -> dict of (ref, S) pairs: dlogits [M][Vp], row_loss, row_smooth, loss; and denom (exact)."""
    tgt, count = ce_targets(labels, V)
    denom = float(num_items) if num_items > 0 else float(count)
    r = cross_entropy_rows(z, tgt, V, denom, eps)
    (d, Sd), (row_loss, S_rl), (row_smooth, S_rs), valid = r["dlogits"], r["row_loss"], r["row_smooth"], r["valid"]
    if denom > 0:
        loss = ((1.0 - eps) * row_loss.sum() + eps * row_smooth.sum()) / denom
        S_loss = ((1.0 - eps) * S_rl.sum() + eps * S_rs.sum()) / denom
    else:
        loss, S_loss = torch.zeros((), dtype=F64), torch.zeros((), dtype=F64)
    return {"dlogits": (d, Sd), "row_loss": (row_loss, S_rl), "row_smooth": (row_smooth, S_rs),
            "loss": (loss.reshape(1), S_loss.reshape(1)), "denom": denom, "valid": valid, "tgt": tgt}


def ce_case(B, T, V, Vp, seed, pad=0.0):
    """Logits [B T][Vp], labels [B][T] and the underflow rows of a cross-entropy case.
    (3, 7): batch row 0 has a -100 run (rows 1, 2), a label >= V (row 4) and a negative label other than -100 (row 5): zero rows;
    batch row 2 is ignored whole; batch row 1 (rows 7 .. 12) holds the special rows, with targets 0, V - 1 and the column just
    before a chunk boundary (2047, the last column of every thread's first chunk round, when V > 2048; else 7):
      row 7  all logits equal (p = 1 / V);
      row 8  saturated, target at +40 the rest at -40 (underflow; p_target - 1 cancels);
      row 9  saturated, the target NOT the max (underflow; row_loss about 80);
      row 10 the row max in the last valid column;
      row 11 every logit -30080 (bf16 spacing there is 128, so a constant row is the only one within 80 of its max);
      row 12 the row max in a column of the last wave's share (2000 when V > 2000, else V - 2).
    Any other (B, T): random rows, every label valid."""
    z = logits_rows(B * T, V, Vp, seed, pad=pad)
    lab = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(seed + 1))
    if (B, T) != (3, 7):
        return z, lab, []
    lab[0, 2:4] = -100
    lab[0, 5], lab[0, 6] = V, -7
    lab[2, :] = -100
    before = 2047 if V > 2048 else min(V - 1, 7)
    lab[1, 1:7] = torch.tensor([0, V - 1, before, V // 2, 3 % V, 5 % V])
    r0 = T
    z[r0, :V] = 1.5
    z[r0 + 1, :V] = -40.0
    z[r0 + 1, V - 1] = 40.0
    z[r0 + 2, :V] = -40.0
    z[r0 + 2, (before + 1) % V] = 40.0
    z[r0 + 3, V - 1] = 31.0
    z[r0 + 4, :V] = -30080.0
    z[r0 + 5, 2000 if V > 2000 else max(V - 2, 0)] = 31.0
    return z, lab, [r0 + 1, r0 + 2]


# ------------------------------------------------------------------------------------------------ column sums
def colsum(X):
    """X [M][N] -> (sum over rows, S)."""
    return X.sum(0), X.abs().sum(0)
