"""numpy / Python-integer restatement of slam_sample_tokens_full's rule (include/slam_engine.h), and the inputs of its tests.
sc and y_i are formed in float32 (IEEE: the device's bits), exp2 in float64, everything behind it in exact integers. The device's
exp2 is a couple of fp32 ulps off, so a mass carries a relative error of about 2^-22 and a sum of masses at most that of Q; a
decision whose integer quantity lies within TOL * Q (four times that) of flipping is reported as `near`. Shared by
tests/test_full_sampling_host.py (the cap on near decisions, from the reference alone) and tests/test_gpu_full_sampling.py."""
import math

import numpy as np

from tests.sampling_ref import DOMAIN, greedy, scores
from tests.sr_ref import MASK, philox4x32_10

TOL = 2.0 ** -20
QMAX = 1 << 40
SEED, PAD, STEPS = 0x5EED0123456789, 1, 64
ROW_IDS = [3, (1 << 33) + 5, 7, 1 << 40, 12]  # beyond 32 bits too
# name -> (do_sample, temperature, top_p, min_p, epsilon_cutoff)
SETTINGS = {"t0.7": (1, 0.7, 1.0, 0.0, 0.0), "t1.3": (1, 1.3, 1.0, 0.0, 0.0), "top_p": (1, 1.0, 0.9, 0.0, 0.0),
            "top_p_tiny": (1, 1.0, 1e-6, 0.0, 0.0), "min_p": (1, 1.0, 1.0, 0.05, 0.0), "epsilon": (1, 1.0, 1.0, 0.0, 3e-4),
            "all": (1, 0.9, 0.9, 0.05, 3e-4), "greedy": (0, 1.0, 1.0, 0.0, 0.0)}


def masses(x, banned, temperature):
    """q [V] (int64) of one logits row, or None when the row has no score above -inf."""
    x = scores(x, banned)
    if x.max() == -np.inf:
        return None
    sc = (np.float32(1.0) / np.float32(temperature)) * np.float32(1.44269504)
    with np.errstate(over="ignore", invalid="ignore"):
        y = ((x - x.max()) * sc).astype(np.float32)
    return np.floor(np.exp2(y.astype(np.float64)) * float(QMAX)).astype(np.int64)


def cut(q, top_p, min_p, eps):
    """(c, slack): the threshold of the kept set { q_i >= c }, and the smallest distance of a cut comparison from flipping."""
    Q, c, slack = int(q.sum()), 0, math.inf
    vals, inv = np.unique(q, return_inverse=True)
    if np.float32(top_p) < 1:
        S = np.cumsum(np.bincount(inv, weights=None, minlength=len(vals)) * vals)  # S(v) of every distinct value, exact in int64
        thr = int(float(np.float32(1.0) - np.float32(top_p)) * float(Q))
        kept = S > thr
        c = int(vals[kept][0]) if kept.any() else QMAX
        slack = min(slack, int(np.abs(S[vals > 0] - thr).min()))
    if min_p > 0:
        c = max(c, int(float(np.float32(min_p)) * float(QMAX)))
    if eps > 0:
        Q1 = int(q[q >= c].sum())
        c = max(c, math.ceil(float(np.float32(eps)) * float(Q1)))
    c = min(c, QMAX)
    if min_p > 0 or eps > 0:
        slack = min(slack, int(np.abs(vals[vals > 0] - c).min()) if c < QMAX else math.inf)
    return c, slack


def sample_rows(x, banned, setting, row_ids, steps, seed=SEED):
    """(tok [B, len(steps)] int64, -1 where the row has no score; near [B, len(steps)] bool) for logits x [B, V]: row b draws with
    row id row_ids[b] at every step of `steps`."""
    do_sample, temperature, top_p, min_p, eps = SETTINGS[setting] if isinstance(setting, str) else setting
    r = np.asarray(row_ids, dtype=np.int64).astype(np.uint64)[:, None]
    s = np.asarray(steps, dtype=np.uint64)[None, :]
    r, s = np.broadcast_arrays(r, s)
    w = philox4x32_10((r & MASK, s, r >> np.uint64(32), np.full_like(r, DOMAIN)), (seed & MASK, seed >> 32))
    tok = np.full(r.shape, -1, dtype=np.int64)
    near = np.zeros(r.shape, dtype=bool)
    for b in range(x.shape[0]):
        if not do_sample:
            tok[b] = greedy(x[b], banned)
            continue
        q = masses(x[b], banned, temperature)
        if q is None:
            continue
        c, slack = cut(q, top_p, min_p, eps)
        band = TOL * float(q.sum())
        cum = np.cumsum(np.where(q >= c, q, 0))
        for j in range(r.shape[1]):
            t = (((int(w[0][b, j]) << 32) | int(w[1][b, j])) * int(cum[-1])) >> 64
            i = int(np.searchsorted(cum, t, side="right"))  # the lowest id whose prefix sum exceeds t
            tok[b, j] = i
            near[b, j] = slack < band or min(t - (int(cum[i - 1]) if i else 0), int(cum[i]) - t) < band
    return tok, near


def logits(V, B=5):
    """Rows by kind. B = 5: N(0, 3^2) rounded to 1/16 (ties at every level, cut values apart); one dominant token in front of a
    tail of mass 0; all scores equal; 30 % -inf and a NaN; no score at all. B = 2 (the 152,167 case): a +inf (read as FLT_MAX) far
    into the row over a full N(0, 3^2) background, and N(0, 3^2) on every 16th id, -inf between them, a tail of mass 0 - a
    full-support row of that length has more than 2 % of its mass on tokens lighter than the band itself."""
    g = np.random.default_rng(V + (1000 if V == 4097 else 0))  # chosen on the CPU: no cut lands inside the band
    x = (np.round(g.normal(0.0, 3.0, (B, V)) * 16) / 16).astype(np.float32)
    if B == 2:
        x[0, (2 * V) // 3 + 1] = np.inf
        live = np.arange(V) % 16 == 5
        x[1, ~live] = -np.inf
        x[1, V - 10000:] -= 100.0
        return x
    x[1, V // 3] = x[1].max() + 6.0
    x[1, V - V // 4:] -= 100.0
    x[2] = 0.25
    x[3, g.random(V) < 0.3] = -np.inf
    x[3, 1] = np.nan
    x[4] = -np.inf
    x[4, V // 2] = np.nan
    return x


def banned(V):
    """The vocabulary-wide mask: ids 0, 7 and the last one."""
    m = np.zeros(V, dtype=np.uint8)
    m[[0, 7, V - 1]] = 1
    return m
