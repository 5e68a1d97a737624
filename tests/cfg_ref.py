"""numpy restatement of slam_cfg_scores (include/slam_engine.h), CPU only.

`cfg_f32` follows the header's float32 arithmetic step by step: both rows are read as the sampler reads a score (`clean`), their
statistics (m, S) are slam_token_logprobs' (`row_lse_f32` of tests/logprob_ref.py: that file's chunk and butterfly order),
L = m + logf(S), then a = x - L_x, u = y - L_y, d = a - u and g d + u, each operation rounded to float32 on its own, with the
header's non-finite rules. `cfg_f64` is the same definition in float64 without any prescribed order: the reference of the GPU
test, whose tolerance is 10 x the largest |f32 - f64| over `op_cases()`. Two things of the float32 format belong to the
definition and are kept in float64 too: a subtraction, product or sum beyond float32's range is +-inf there (a row holding +inf,
read as FLT_MAX, puts its other scores near -FLT_MAX, and g times that overflows), and the result is stored as a float32.
"""
import numpy as np

from tests.logprob_ref import NEG_INF, VOCABS, clean, row_lse_f32

GUIDANCE = (1.5, 3.0, 0.5, 0.0, -1.0)


def _pair_f32(x, y, g) -> np.ndarray:
    x, y = clean(x), clean(y)
    g = np.float32(g)
    out = np.full(len(x), NEG_INF, np.float32)
    mx, Sx = row_lse_f32(x)
    if mx == NEG_INF:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        a = (x - np.float32(mx + np.log(Sx).astype(np.float32))).astype(np.float32)
        my, Sy = row_lse_f32(y)
        if my == NEG_INF:
            return a
        u = (y - np.float32(my + np.log(Sy).astype(np.float32))).astype(np.float32)
        d = (a - u).astype(np.float32)
        r = ((g * d).astype(np.float32) + u).astype(np.float32)
    r = np.where(u == NEG_INF, a, r)
    return np.where(a == NEG_INF, NEG_INF, r).astype(np.float32)


def cfg_f32(logits: np.ndarray, g: float) -> np.ndarray:
    """scores float32 [B, V] of logits float32 [2 B, V] in the kernel's arithmetic."""
    B = len(logits) // 2
    return np.stack([_pair_f32(logits[b], logits[B + b], g) for b in range(B)])


def _f32_range(v: np.ndarray) -> np.ndarray:
    """float64 values that float32 cannot hold become +-inf, as the rounding to float32 makes them."""
    with np.errstate(over="ignore"):
        return np.where(np.isinf(v.astype(np.float32)), np.sign(v) * np.inf, v)


def _lse_f64(x: np.ndarray):
    m = x.max()
    return m if m == -np.inf else m + np.log(np.exp(x - m).sum())


def _pair_f64(x, y, g) -> np.ndarray:
    x, y = clean(x).astype(np.float64), clean(y).astype(np.float64)
    Lx, Ly = _lse_f64(x), _lse_f64(y)
    if Lx == -np.inf:
        return np.full(len(x), -np.inf)
    with np.errstate(invalid="ignore"):
        a = _f32_range(x - Lx)
        if Ly == -np.inf:
            return a
        u = _f32_range(y - Ly)
        r = _f32_range(_f32_range(np.float64(g) * _f32_range(a - u)) + u)
    r = np.where(u == -np.inf, a, r)
    return np.where(a == -np.inf, -np.inf, r)


def cfg_f64(logits: np.ndarray, g: float) -> np.ndarray:
    """The same scores from float64 arithmetic, stored as float32 like the kernel's and returned as float64."""
    B = len(logits) // 2
    r = np.stack([_pair_f64(logits[b], logits[B + b], g) for b in range(B)])
    with np.errstate(over="ignore"):
        return r.astype(np.float32).astype(np.float64)


def op_cases():
    """The GPU op test's inputs: (name, logits float32 [6, V], g). B = 3: rows 0 .. 2 are conditional, rows 3 .. 5 their
    unconditional twins. V = 502, 2048, 2049 (one launch: an odd row stride, exactly one chunk; two launches: one score above a
    chunk) and 152167 (75 chunks); with V = 502 and the odd ones rows 1 and 2 of both logits and scores do not start on a
    16-byte boundary. Pair 0 is plain. Pair 1 holds -inf entries and a NaN on the conditional side, other -inf entries on the
    unconditional side, one index where both are -inf. Pair 2 holds a +inf on the conditional side ("v.." cases) or on the
    unconditional side ("u.." cases, V = 502 and 2049). Every one of these runs every g of GUIDANCE. "xdead" has an all -inf
    conditional row and an all-NaN one, "ydead" an all -inf unconditional row and an all-NaN one."""
    cases = []

    def base(V):
        r = np.random.default_rng(V)
        x = (r.standard_normal((6, V)) * 3.0).astype(np.float32)
        x[1, 5:40:7] = -np.inf
        x[1, V // 2] = np.nan
        x[4, 6:60:9] = -np.inf
        x[4, 12] = -np.inf  # 12 is in 5:40:7 too: -inf on both sides
        x[4, V // 2 + 1] = np.nan
        return x

    for V in VOCABS:
        for g in GUIDANCE:
            x = base(V)
            x[2, V // 3] = np.inf
            cases.append((f"v{V}_g{g}", x, g))
    for V in (502, 2049):
        for g in GUIDANCE:
            x = base(V)
            x[5, V // 3] = np.inf
            cases.append((f"u{V}_g{g}", x, g))
    for g in (1.5, 0.0):
        x = base(502)
        x[0, :] = -np.inf
        x[2, :] = np.nan
        cases.append((f"xdead_g{g}", x, g))
        x = base(2049)
        x[3, :] = -np.inf
        x[5, :] = np.nan
        cases.append((f"ydead_g{g}", x, g))
    return cases


def restatement_error(cases=None) -> float:
    """Largest |cfg_f32 - cfg_f64| over the finite entries of the cases; non-finite entries must agree exactly."""
    worst = 0.0
    for _, x, g in (cases or op_cases()):
        a, r = cfg_f32(x, g).astype(np.float64), cfg_f64(x, g)
        fin = np.isfinite(r)
        assert np.array_equal(a[~fin], r[~fin])
        if fin.any():
            worst = max(worst, float(np.abs(a[fin] - r[fin]).max()))
    return worst
