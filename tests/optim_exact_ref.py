"""Float64 reference, designed inputs and the acceptance rule for the optimizer kernels of slamkit_amd/csrc/optimizer.hip
(AdamW in its three state precisions and every kernel form, the chunked gradient norm, the clip coefficient). No GPU is needed
to import or run anything here; every function works on the device its tensors are on. bf16_rne, accept_bf16, accept_f32, bits
and the band bit patterns are tests/row_exact_ref.py's.

THE REFERENCE is one step of torch.optim.AdamW in float64 from the STORED values (p, m, v as the buffers hold them, g times the
fp32 clip coefficient) with the hyper-parameters AS THE KERNELS RECEIVE THEM (adam_hyper in optimizer.hip): lr, b1, b2, eps, wd
rounded to fp32, bc1 = f32(1 - b1^t) and bc2s = f32(sqrt(1 - b2^t)) computed in double from the double betas:

    m' = b1 m + (1 - b1) g      v' = b2 v + (1 - b2) g^2      den = sqrt(v') / bc2s + eps
    p' = p (1 - lr wd) - (lr / bc1) m' / den

(with the unrounded doubles instead, 6 % of a million designed elements fall outside the bar below - a property of that
reference, not of a kernel). The absolute-term sums:

    S_m = |b1 m| + |(1 - b1) g|            master form (modes 0 and 1: b1 m + (1 - b1) g)
        = |m| + (1 - b1) (|g| + |m|)       lerp form (mode 2: m + (1 - b1) (g - m))
    S_v = v'
    S_p = |p (1 - lr wd)| + (lr / bc1) / den S_m       the moment's own cancellation is carried into the step

THE RULE, DELTA_OPT = 2^-20: fp32 outputs (the master; m and v of mode 0) |got - ref| <= DELTA_OPT S; bf16 outputs (p of mode 2;
m and v of modes 1 and 2) bf16_rne(ref - DELTA_OPT S) <= got <= bf16_rne(ref + DELTA_OPT S), no tolerance on the bf16 side.
The budget: a moment costs at most 4 to 5 fp32 roundoffs of its S (the product g cs, two products, the sum or the subtraction
and the fused add); the parameter adds the square root, two divisions, the add of eps, 1 - lr wd, two multiplies and the final
add: about 12 in the worst case, so 16 roundoffs = 2^-20 covers it. DELTA_OPT is a property of this reference:
tests/test_optim_exact_host.py runs fp32 restatements of both expressions of adam_elem (every operation rounded separately, and
every multiply-add fused) through the rule and requires 0 violations. It never moves because a GPU run was outside it.

Stochastic rounding: the stored bf16 value is one of the bf16 neighbours of the interval - from the bf16 value at or below
ref - DELTA_OPT S up to the one at or above ref + DELTA_OPT S. Which of the two belongs to tests/test_gpu_sr.py.

Non-finite gradients: the element takes the NaN / inf pattern of the float64 formula (checked on bits of the pattern, outside
the interval rule, whose S is not a number there); its neighbours are ordinary elements of the rule.

Underflow: only the elements of the underflow class (v' below 2^-126) are accepted with underflow=True (any |got| <= 2^-120
where |ref| < 2^-120); every other element asserts on the reference that nothing non-zero is that small."""
import math

import numpy as np
import torch

from tests import row_exact_ref as R

DELTA_OPT = 2.0 ** -20
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GRAD_CHUNK = 8192

CLASSES = ("ordinary", "still", "eps-dominated", "cancelling", "first-step", "tiny", "underflow", "non-finite")
ORD, STILL, EPSD, CANC, FIRST, TINYC, UNDER, NONF = range(8)
# the class of element i is _TABLE[i % 37]: 37 is prime to 8, so every class meets every position i % 8 within 296 elements, and
# every class occurs in every run of 37 - in every tensor of a model, vectors included. The non-finite elements are placed per
# tensor on top of it.
_TABLE = torch.tensor([ORD, EPSD, ORD, CANC, ORD, FIRST, ORD, STILL, ORD, TINYC, ORD, UNDER, ORD, EPSD, ORD, CANC, ORD, FIRST, ORD,
                       STILL, ORD, TINYC, ORD, UNDER, ORD, EPSD, CANC, FIRST, ORD, EPSD, CANC, FIRST, STILL, TINYC, UNDER, ORD, ORD],
                      dtype=torch.int8)
assert _TABLE.numel() == 37
FLIP_CLASSES = (ORD, EPSD, CANC, FIRST)   # at least half of their elements move to another bf16 value in mode 2

# (lr, b1, b2, eps, wd, t): the first step; a late one; one where both corrections are 1.0f exactly; one whose decay and step
# are large enough to show in bf16
HYPERS = [(1e-3, .9, .999, 1e-8, .01, 1), (1e-3, .9, .999, 1e-8, .01, 1000), (1e-3, .9, .999, 1e-8, 0.0, 100000),
          (.1, .8, .95, 1e-6, .1, 3)]
CLIPS = (1.0, float(np.float32(0.37)))


def f32(x):
    return float(np.float32(x))


def hyper(lr, b1, b2, eps, wd, t):
    """The hyper-parameters as adam_hyper hands them to the kernels (float64 values of the fp32 numbers)."""
    return {"lr": f32(lr), "b1": f32(b1), "b2": f32(b2), "eps": f32(eps), "wd": f32(wd), "t": int(t),
            "bc1": f32(1.0 - math.pow(b1, float(t))), "bc2s": f32(math.sqrt(1.0 - math.pow(b2, float(t))))}


def hyper_exact(lr, b1, b2, eps, wd, t):
    """The same in unrounded doubles: torch.optim.AdamW's own numbers (the cross-check of the reference, nothing else)."""
    return {"lr": lr, "b1": b1, "b2": b2, "eps": eps, "wd": wd, "t": int(t), "bc1": 1.0 - b1 ** t, "bc2s": math.sqrt(1.0 - b2 ** t)}


# ------------------------------------------------------------------------------------------------ designed inputs
def store(x64, bf):
    """float64 -> the float64 value of what a bf16 (bf) or fp32 buffer holds"""
    return R.bf16_rne(x64).double() if bf else x64.to(F32).double()


def design(ranges, mode, g16, seed=0, nonfinite=True):
    """p, m, v, g (float64 CPU, each representable in the storage type of `mode` / of the gradient buffer) and cls (int8) for a flat
    buffer made of the tensors `ranges` = [(lo, hi)], contiguous from 0, bounds multiples of 8, each at least 64 elements.
      ordinary       p ~ 0.02 N, g ~ 1e-2 N, m ~ 3e-3 N, v ~ 1e-5 chi^2
      still          g = m = v = 0: pure decay, 0 / eps
      eps-dominated  |g| log-uniform in [1e-10, 1e-7], v in {0, g^2}, m = g / 2: den ~ eps
      cancelling     g = -9 m (1 + 1e-3 N): m' ~ 0
      first-step     |g| log-uniform in [1e2, 1e4], m = v = 0: the update is lr sign(g) at t = 1
      tiny           |g| log-uniform in [1e-15, 1e-12], m = v = 0: v' ~ 1e-33 .. 1e-27
      underflow      |g| = 2^-70, m = v = 0: v' below 2^-126
      non-finite     per tensor one inf, one -inf, one NaN gradient, each alone in its group of 8, at a position i % 8 that moves
                     with the tensor's index"""
    n = ranges[-1][1]
    assert ranges[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ranges[:-1], ranges[1:]))
    gen = torch.Generator().manual_seed(seed)
    N = lambda: torch.randn(n, generator=gen, dtype=F64)                       # noqa: E731
    U = lambda: torch.rand(n, generator=gen, dtype=F64)                        # noqa: E731
    sign = lambda: torch.where(U() < 0.5, -1.0, 1.0).to(F64)                   # noqa: E731
    cls = _TABLE[torch.arange(n) % 37].clone()
    zero = torch.zeros(n, dtype=F64)
    p = 0.02 * N()
    m_ord, v_ord = 3e-3 * N(), 1e-5 * N() ** 2
    g = 1e-2 * N()
    m, v = m_ord.clone(), v_ord.clone()
    g_eps = sign() * 10.0 ** (-10.0 + 3.0 * U())
    g_can = -9.0 * m_ord * (1.0 + 1e-3 * N())
    g_first = sign() * 10.0 ** (2.0 + 2.0 * U())
    g_tiny = sign() * 10.0 ** (-15.0 + 3.0 * U())
    g_under = sign() * 2.0 ** -70
    half = U() < 0.5
    for c, gc, mc, vc in ((STILL, zero, zero, zero), (EPSD, g_eps, g_eps / 2, torch.where(half, zero, g_eps ** 2)),
                          (CANC, g_can, m_ord, v_ord), (FIRST, g_first, zero, zero), (TINYC, g_tiny, zero, zero),
                          (UNDER, g_under, zero, zero)):
        k = cls == c
        g, m, v = torch.where(k, gc, g), torch.where(k, mc, m), torch.where(k, vc, v)
    if nonfinite:
        for ti, (lo, hi) in enumerate(ranges):
            assert lo % 8 == 0 and hi - lo >= 64, (lo, hi)
            for j, val in enumerate((float("inf"), float("-inf"), float("nan"))):
                i = lo + 8 * (1 + 2 * j) + (ti + 3 * j) % 8
                g[i], cls[i] = val, NONF
    return {"p": store(p, mode == 2), "m": store(m, mode != 0), "v": store(v, mode != 0), "g": store(g, g16), "cls": cls}


def check_design(ranges, d):
    """The generator's own conditions: every class at every position i % 8, every class in every tensor, every non-finite
    gradient alone in its group of 8."""
    cls, n = d["cls"], d["cls"].numel()
    pos = torch.arange(n) % 8
    for c in range(len(CLASSES)):
        if c == NONF and not bool((cls == NONF).any()):
            continue
        have = set(pos[cls == c].tolist())
        assert have == set(range(8)), f"class {CLASSES[c]} misses positions {sorted(set(range(8)) - have)}"
        for lo, hi in ranges:
            assert bool((cls[lo:hi] == c).any()), f"class {CLASSES[c]} does not occur in tensor [{lo}, {hi})"
    bad = ~torch.isfinite(d["g"])
    assert torch.equal(bad, cls == NONF)
    assert int(bad.view(-1, 8).sum(1).max()) <= 1, "two non-finite gradients share a group of 8"
    for k in "pmv":
        assert bool(torch.isfinite(d[k]).all())


def check_reference(tag, d, ref, cancel_moves, report=True):
    """The conditions a bf16-state (mode 2) case must meet, on the reference alone: at least half of the ordinary, eps-dominated
    and first-step elements - and of the four moving classes together - have bf16_rne(ref p') != p; so do the cancelling ones
    where the clip coefficient or the betas undo their cancellation (cancel_moves; with m' ~ 0 and lr wd = 1e-5 a cancelling element
    cannot leave its bf16 value: that is what the class is for, and its m is where it shows); over the whole case (p, m, v) at most
    5 % of the intervals hold two bf16 values; nothing non-zero below 2^-120 outside the underflow class, whose v' is below 2^-126."""
    cls, p1 = d["cls"], ref["p"][0]
    fin = torch.isfinite(p1)
    assert torch.equal(~fin, cls == NONF), tag
    flip = (R.bf16_rne(p1).double() != d["p"]) & fin
    share = {c: float(flip[cls == c].double().mean()) for c in FLIP_CLASSES}
    union = float(flip[(cls == ORD) | (cls == EPSD) | (cls == CANC) | (cls == FIRST)].double().mean())
    two = {}
    for k in "pmv":
        r, S = ref[k][0][fin], ref[k][1][fin]
        two[k] = float((R.bf16_rne(r - DELTA_OPT * S).double() != R.bf16_rne(r + DELTA_OPT * S).double()).double().mean())
        R.assert_normal(f"{tag} {k}", torch.where(cls[fin] == UNDER, torch.zeros_like(r), r))
    case = sum(two.values()) / 3
    if report:
        print(f"[optim-exact] {tag}: moved to another bf16 value: " + ", ".join(f"{CLASSES[c]} {x:.3f}" for c, x in share.items())
              + f", together {union:.3f}; two-member share " + ", ".join(f"{k} {t:.4f}" for k, t in two.items()) + f", whole case {case:.4f}")
    for c in (ORD, EPSD, FIRST):
        assert share[c] >= 0.5, (tag, CLASSES[c], share[c])
    assert union >= 0.5, (tag, union)
    if cancel_moves:
        assert share[CANC] >= 0.5, (tag, share[CANC])
    assert case <= 0.05, (tag, case)
    under = cls == UNDER
    assert bool((ref["v"][0][under] < 2.0 ** -126).all()) and bool((ref["v"][0][under] > 0).all()), tag


# ------------------------------------------------------------------------------------------------ the reference
def adam_ref(p, m, v, g, cs, h, lerp, wd=None):
    """One AdamW step in float64. cs: the clip coefficient (the float64 value of the fp32 number; 1.0 without a norm_out); wd: None
    = h's, or a per-element tensor (the no-decay mask). lerp: S_m of the lerp form (mode 2). -> {"p" | "m" | "v": (ref, S)}"""
    wd = h["wd"] if wd is None else wd
    ge = g * cs
    b1, b2, k = h["b1"], h["b2"], h["lr"] / h["bc1"]
    m1 = b1 * m + (1.0 - b1) * ge
    v1 = b2 * v + (1.0 - b2) * ge * ge
    den = v1.sqrt() / h["bc2s"] + h["eps"]
    dec = p * (1.0 - h["lr"] * wd)
    p1 = dec - k * m1 / den
    Sm = (m.abs() + (1.0 - b1) * (ge.abs() + m.abs())) if lerp else ((b1 * m).abs() + ((1.0 - b1) * ge).abs())
    Sp = dec.abs() + k / den * Sm
    return {"p": (p1, Sp), "m": (m1, Sm), "v": (v1, v1)}


VARIANTS = ("a", "b", "c", "d", "e", "f", "g")


def adam_variant(which, p, m, v, g, cs, h, t_hyper):
    """The reference arithmetic with one seeded defect -> (p', m', v') in float64 (the sensitivity test rounds them to storage):
      a  the bf16-rounded m' and v' used in the parameter step      b  eps inside the square root
      c  bc2 where sqrt(bc2) belongs                                d  decay after the step
      e  the clip applied to m but not to v                         f  L2 form (g += wd p) instead of decoupled decay
      g  bc1 taken at step t - 1 (t_hyper: the tuple `h` was made from)"""
    b1, b2, lr, eps, wd, bc1, bc2s = h["b1"], h["b2"], h["lr"], h["eps"], h["wd"], h["bc1"], h["bc2s"]
    ge = g * cs
    gv = g if which == "e" else ge
    if which == "f":
        ge = ge + wd * p
        gv = ge
    if which == "g":
        bc1 = f32(1.0 - math.pow(t_hyper[1], float(t_hyper[5] - 1)))
    m1 = b1 * m + (1.0 - b1) * ge
    v1 = b2 * v + (1.0 - b2) * gv * gv
    mu, vu = (R.bf16_rne(m1).double(), R.bf16_rne(v1).double()) if which == "a" else (m1, v1)
    if which == "b":
        den = (vu + eps).sqrt() / bc2s
    elif which == "c":
        den = vu.sqrt() / (bc2s * bc2s) + eps
    else:
        den = vu.sqrt() / bc2s + eps
    k = lr / bc1 if bc1 != 0 else float("inf")
    if which == "d":
        p1 = (p - k * mu / den) * (1.0 - lr * wd)
    elif which == "f":
        p1 = p - k * mu / den
    else:
        p1 = p * (1.0 - lr * wd) - k * mu / den
    return p1, m1, v1


def _r32(x64):
    return x64.to(F32).double()


def _fma(a, b, c):
    """fp32 fused multiply-add of float64-held fp32 values: the product of two fp32 numbers is exact in float64"""
    return _r32(a * b + c)


def adam_restated(p, m, v, g, cs, h, lerp, fused, wd=None):
    """adam_elem of optimizer.hip in fp32 (every value below is the float64 image of an fp32 number): fused = False rounds every
    operation separately, fused = True contracts every multiply-add the expressions allow. -> fp32-valued (p', m', v')"""
    r = _r32
    wd = h["wd"] if wd is None else wd
    lr, b1, b2, eps, bc1, bc2s = h["lr"], h["b1"], h["b2"], h["eps"], h["bc1"], h["bc2s"]
    one_b1, one_b2, k = r(torch.tensor(1.0 - b1, dtype=F64)), r(torch.tensor(1.0 - b2, dtype=F64)), r(torch.tensor(lr / bc1, dtype=F64))
    wd_t = wd if torch.is_tensor(wd) else torch.tensor(wd, dtype=F64)
    ge = r(g * cs)
    if not fused:
        p = r(p * r(1.0 - r(lr * wd_t)))
        m = r(m + r(one_b1 * r(ge - m))) if lerp else r(r(b1 * m) + r(one_b1 * ge))
        v = r(r(b2 * v) + r(r(one_b2 * ge) * ge))
        den = r(r(r(v.sqrt()) / bc2s) + eps)
        p = r(p - r(k * r(m / den)))
    else:
        p = r(p * _fma(-lr * torch.ones_like(wd_t), wd_t, 1.0))
        m = _fma(one_b1, r(ge - m), m) if lerp else _fma(b1 * torch.ones_like(m), m, r(one_b1 * ge))
        v = _fma(b2 * torch.ones_like(v), v, r(r(one_b2 * ge) * ge))
        den = r(r(r(v.sqrt()) / bc2s) + eps)
        p = _fma(-k, r(m / den), p)
    return p, m, v


# ------------------------------------------------------------------------------------------------ acceptance
def bf16_step(b, up):
    """the next bf16 value above (up) or below b, by bits; -0 and +0 are one point"""
    i = R.bits(b).to(torch.int32)
    k = torch.where(i >= 0, i, -(i & 0x7FFF))
    k = k + (1 if up else -1)
    i = torch.where(k >= 0, k, (-k) | 0x8000)
    i = torch.where(i >= 0x8000, i - 0x10000, i).to(torch.int16)
    return i.view(BF16).reshape(b.shape)


def bf16_floor(x64):
    b = R.bf16_rne(x64)
    return torch.where(b.double() > x64, bf16_step(b, False), b)


def bf16_ceil(x64):
    b = R.bf16_rne(x64)
    return torch.where(b.double() < x64, bf16_step(b, True), b)


class Layout:
    """The tensors of a flat buffer: names, bounds, shapes - what a failure message needs to say where an element lives."""

    def __init__(self, tensors, n):
        """tensors: [(name, offset, rows, cols)] in layout order; a tensor owns the elements up to the next one's offset"""
        self.names = [t[0] for t in tensors]
        self.lo = [int(t[1]) for t in tensors]
        self.hi = self.lo[1:] + [int(n)]
        self.rows = [int(t[2]) for t in tensors]
        self.cols = [int(t[3]) for t in tensors]
        self.n = int(n)

    @property
    def ranges(self):
        return list(zip(self.lo, self.hi))

    def where(self, i, path):
        ti = max(k for k, lo in enumerate(self.lo) if lo <= i)
        c = self.cols[ti]
        r, col = divmod(i - self.lo[ti], max(c, 1))
        form = path if path in ("flat", "range") else ("tile" if c > 1 else "strided")
        return f"tensor {self.names[ti]} [{self.rows[ti]} x {c}] (row {r}, column {col}), kernel form {form}"


def _explain(name, i, got, lo, hi, ref, S, layout, path, cls, index=None):
    flat = i if index is None else int(index[i])
    w = layout.where(flat, path) if layout is not None else "-"
    c = CLASSES[int(cls[i])] if cls is not None else "-"
    return (f"{name}: flat index {flat} ({flat % 8} mod 8), {w}, class {c}: got {float(got[i])!r} not in [{float(lo[i])!r}, {float(hi[i])!r}], "
            f"ref {float(ref[i])!r}, S {float(S[i])!r}")


def accept(name, got, ref, S, cls, layout=None, path="flat", sr=False, stats=None, index=None):
    """The rule over one array of a case -> the number of violations (0 to pass); the first one is explained on stdout and in
    stats["msg"]. got: fp32 or bf16; ref, S: float64; cls: the class of every element. Elements with a non-finite reference are
    held to its pattern; the underflow class goes through row_exact_ref's accept_bf16 / accept_f32 under the underflow rule,
    every other element through them under the plain rule (with sr: the neighbour rule, here); nothing is left out.
    stats: a dict that receives the worst |err| / S in units of 2^-24 (fp32 arrays, the underflow class apart) and msg.
    index: the flat index of every element handed over, where they are a selection of the buffer (a ranged update)."""
    dev = ref.device
    got, cls = got.detach().to(dev).reshape(-1), cls.to(dev)
    ref, S = ref.reshape(-1), S.reshape(-1)
    g64 = got.double()
    nf = ~torch.isfinite(ref)
    bad = nf & ~((torch.isnan(ref) & torch.isnan(g64)) | (g64 == ref))
    fin = ~nf
    assert bool(torch.isfinite(S[fin]).all()), f"{name}: a finite reference with a non-finite S"
    under = fin & (cls == UNDER)
    main = fin & ~under
    z = torch.zeros_like(ref)
    refc, Sc = torch.where(fin, ref, z), torch.where(fin, S, z)
    lo64, hi64 = refc - DELTA_OPT * Sc, refc + DELTA_OPT * Sc
    flush = under & (refc.abs() < R.TINY) & (g64.abs() <= R.TINY)
    if got.dtype == BF16:
        lo, hi = (bf16_floor(lo64), bf16_ceil(hi64)) if sr else (R.bf16_rne(lo64), R.bf16_rne(hi64))
        lo, hi = lo.double(), hi.double()
        mine = fin & ~((lo <= g64) & (g64 <= hi)) & ~flush
        if sr:
            R.assert_normal(name, refc[main])
            nbad = int(mine.sum())
        else:
            nbad = R.accept_bf16(name, got[main], ref[main], S[main], delta=DELTA_OPT)
            if bool(under.any()):
                nbad += R.accept_bf16(name + " (underflow class)", got[under], ref[under], S[under], delta=DELTA_OPT, underflow=True)
            assert nbad == int(mine.sum()), (name, nbad, int(mine.sum()))
    else:
        assert got.dtype == F32 and not sr, (got.dtype, sr)
        lo, hi = lo64, hi64
        mine = fin & ~((g64 - refc).abs() <= DELTA_OPT * Sc) & ~flush
        R.assert_normal(name, refc[main])
        nbad = R.accept_f32(name, got[main], ref[main], S[main], delta=DELTA_OPT)
        if bool(under.any()):
            keep = (~flush)[under].double()                        # the underflow rule: any |got| <= 2^-120 where |ref| < 2^-120
            nbad += R.accept_f32(name + " (underflow class)", got[under] * keep.float(), ref[under] * keep, S[under] * keep, delta=DELTA_OPT)
        assert nbad == int(mine.sum()), (name, nbad, int(mine.sum()))
        if stats is not None:
            k = main & (Sc > 0)
            stats["worst"] = float(((g64 - refc).abs()[k] / Sc[k]).max()) * 2.0 ** 24 if bool(k.any()) else 0.0
    bad |= mine
    nbad = int(bad.sum())
    if nbad:
        i = int(bad.nonzero()[0])
        per = {CLASSES[c]: int((bad & (cls == c)).sum()) for c in range(len(CLASSES)) if bool((bad & (cls == c)).any())}
        host = [t.cpu() for t in (g64, lo, hi, ref, S, cls)]
        msg = (f"{nbad} violations, by class {per}; first: " + _explain(name, i, *host[:5], layout, path, host[5], index))
        for c in range(len(CLASSES)):       # and the first one of every other class that has any
            if CLASSES[c] in per and c != int(cls[i]):
                msg += "; " + _explain("first " + CLASSES[c], int((bad & (cls == c)).nonzero()[0]), *host[:5], layout, path, host[5], index)
        print("[optim-exact] " + msg)
        if stats is not None:
            stats["msg"] = msg
    return nbad


def check(name, got, ref, S, cls, layout, path, sr=False, stats=None, index=None):
    """assert the rule; the assertion message is the explained first violation"""
    stats = {} if stats is None else stats
    n = accept(name, got, ref, S, cls, layout, path, sr, stats, index)
    assert n == 0, stats.get("msg")


# ------------------------------------------------------------------------------------------------ gradient norm
def clip_coef(norm32, max_norm):
    """min(1, f32(max_norm) / (f32(norm) + f32(1e-6))) in fp32 from the norm the kernel returned; 1 when max_norm <= 0"""
    if not max_norm > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return c if np.isnan(c) else np.float32(min(c, np.float32(1.0)))


def ulp_apart(a, b):
    """distance of two finite fp32 numbers of one sign in units in the last place"""
    ia, ib = int(np.float32(a).view(np.int32)), int(np.float32(b).view(np.int32))
    return abs(ia - ib)
