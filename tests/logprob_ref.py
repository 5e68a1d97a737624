"""numpy restatement of slam_token_logprobs (include/slam_engine.h), CPU only.

`logprob_f32` follows the header's float32 arithmetic and summation order step by step: chunks of 2048 scores; in a chunk
thread t of 256 adds expf(x_i - m_c) for i = t, t + 256, .. in that order, a wave's 64 lanes are combined by the xor butterfly
32, 16, .., 1, the four waves as ((w0 + w1) + w2) + w3; the chunks are combined in chunk order,
S = fmaf(s_c, expf(m_c - m), S). `logprob_f64` is the same definition (NaN -> -inf, +inf -> FLT_MAX, the raw row otherwise) in float64 without
any prescribed order: the reference of the GPU test, whose tolerance is 10 x the largest |f32 - f64| over `op_cases()`.
"""
import numpy as np

CHUNK = 2048
THREADS = 256
FLT_MAX = np.float32(3.4028234663852886e38)
NEG_INF = np.float32(-np.inf)


def clean(x) -> np.ndarray:
    """The kernel's reading of a score: NaN -> -inf, +inf -> FLT_MAX (float32)."""
    x = np.array(x, dtype=np.float32, copy=True)
    x[np.isnan(x)] = NEG_INF
    return np.minimum(x, FLT_MAX)


def _chunk_f32(v: np.ndarray):
    """(m_c, s_c) of one cleaned float32 chunk of at most CHUNK scores."""
    m = v.max()
    if m == NEG_INF:
        return m, np.float32(0.0)
    with np.errstate(invalid="ignore"):
        e = np.exp((v - m).astype(np.float32)).astype(np.float32)
    e = np.concatenate([e, np.zeros(CHUNK - len(e), np.float32)])  # adding +0 changes nothing: the missing scores
    e = e.reshape(CHUNK // THREADS, THREADS)                        # row j, column t = score t + 256 j
    acc = np.zeros(THREADS, np.float32)
    for j in range(e.shape[0]):
        acc = (acc + e[j]).astype(np.float32)
    w = acc.reshape(THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, lane ^ o]).astype(np.float32)
    w = w[:, 0]
    return m, np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])


def _fmaf(a, b, c) -> np.float32:
    """fmaf(a, b, c): the product of two float32 is exact in float64; its sum with c is rounded to float64 and then to float32
    (a double rounding that differs from the single one in rare half-way cases only: far below what the tests resolve)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def row_lse_f32(row: np.ndarray):
    """(m, S) of one raw float32 row in the kernel's order."""
    x = clean(row)
    parts = [_chunk_f32(x[c:c + CHUNK]) for c in range(0, len(x), CHUNK)]
    m = max(p[0] for p in parts)
    if len(parts) == 1:
        return m, parts[0][1]
    S = np.float32(0.0)
    if m != NEG_INF:
        for mc, sc in parts:
            if mc != NEG_INF:
                S = _fmaf(sc, np.exp(np.float32(mc - m)).astype(np.float32), S)
    return m, S


def logprob_f32(logits: np.ndarray, tokens) -> np.ndarray:
    out = np.zeros(len(logits), np.float32)
    for b, row in enumerate(logits):
        t = int(tokens[b])
        if not 0 <= t < len(row):
            continue
        m, S = row_lse_f32(row)
        if m == NEG_INF:
            out[b] = NEG_INF
            continue
        out[b] = np.float32(clean(row[t:t + 1])[0] - np.float32(m + np.log(S).astype(np.float32)))
    return out


def logprob_f64(logits: np.ndarray, tokens) -> np.ndarray:
    out = np.zeros(len(logits), np.float64)
    for b, row in enumerate(logits):
        t = int(tokens[b])
        if not 0 <= t < len(row):
            continue
        x = clean(row).astype(np.float64)
        m = x.max()
        if m == -np.inf:
            out[b] = -np.inf
            continue
        out[b] = x[t] - (m + np.log(np.exp(x - m).sum()))
    return out


VOCABS = (502, 2048, 2049, 152167)  # one launch (odd row stride), exactly one chunk, one score above it, 75 chunks


def op_cases():
    """The GPU op test's inputs: (name, logits float32 [3, V], tokens int64 [3]). Row 0 is plain with token 0 picked; row 1
    holds -inf entries and a NaN with token V - 1 picked; row 2 holds one +inf, which is the token picked (its log-prob is
    exactly 0: FLT_MAX absorbs the rest). With V = 502 and 2049 rows 1 and 2 do not start on a 16-byte boundary. The
    "special" case picks ids outside the vocabulary (-1 and V: 0.0) and the NaN entry (-inf); "empty" has a row of -inf only
    and a row of NaN only (-inf each) and picks a -inf entry of an ordinary row (-inf)."""
    cases = []
    for V in VOCABS:
        g = np.random.default_rng(V)
        x = (g.standard_normal((3, V)) * 3.0).astype(np.float32)
        x[1, 5:40:7] = -np.inf
        x[1, V // 2] = np.nan
        x[2, V // 3] = np.inf
        cases.append((f"v{V}", x, np.array([0, V - 1, V // 3], np.int64)))
    V = 502
    x = cases[0][1].copy()
    x[2, V // 3] = 1.0
    cases.append(("special", x, np.array([-1, V // 2, V], np.int64)))
    x = cases[0][1].copy()
    x[0, :] = -np.inf
    x[2, :] = np.nan
    cases.append(("empty", x, np.array([3, 5, 0], np.int64)))
    return cases


def restatement_error(cases=None) -> float:
    """Largest |logprob_f32 - logprob_f64| over the finite entries of the cases; non-finite entries must agree exactly."""
    worst = 0.0
    for _, x, tok in (cases or op_cases()):
        a, r = logprob_f32(x, tok), logprob_f64(x, tok)
        fin = np.isfinite(r)
        assert np.array_equal(a[~fin].astype(np.float64), r[~fin])
        if fin.any():
            worst = max(worst, float(np.abs(a[fin].astype(np.float64) - r[fin]).max()))
    return worst
