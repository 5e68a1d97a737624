"""numpy restatement of the device sampler's contract (slam_sample_tokens, include/slam_engine.h) on top of
tests/sr_ref.philox4x32_10: the scores, the ranked candidates, the weights, the top-p cut and the draw. Two versions of the
arithmetic: fp32 in the stated summation orders (what the kernels do), and fp64, which also says how close each draw came to a
boundary of the cumulative weights and how close each row's top-p cut came to its threshold - the cases in which fp32 and fp64
may legitimately pick different tokens. Shared by tests/test_sampling_host.py (known answers, uniformity) and
tests/test_gpu_sampling.py (the kernels against the fp64 version)."""
import numpy as np

from tests.sr_ref import MASK, philox4x32_10

DOMAIN = 0x53414D50  # "SAMP": the fourth counter word


def uniform(seed, row_ids, steps):
    """u = (w[0] >> 8) * 2^-24 of the draws (row id, step): float64 array [len(row_ids), len(steps)], exact in fp32 too."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = np.asarray(row_ids, dtype=np.int64).astype(np.uint64)[:, None]
    s = np.asarray(steps, dtype=np.uint64)[None, :]
    r, s = np.broadcast_arrays(r, s)
    w = philox4x32_10((r & MASK, s, r >> np.uint64(32), np.full_like(r, DOMAIN)), (seed & MASK, seed >> 32))
    return (w[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def scores(x, banned=None):
    """fp32 scores of one logits row: banned and NaN -> -inf, +inf -> the largest float, -0 -> +0."""
    x = np.array(x, dtype=np.float32)
    x[np.isnan(x)] = -np.inf
    if banned is not None:
        x[np.asarray(banned) != 0] = -np.inf
    x = np.minimum(x, np.finfo(np.float32).max)
    return x + np.float32(0.0)


def candidates(x, top_k):
    """ids of the k' = min(top_k, scores above -inf) candidates in rank order: (score descending, id ascending)."""
    order = np.argsort(-x, kind="stable")
    return order[:min(int(top_k), int((x > -np.inf).sum()))]


def greedy(x, banned=None):
    """The lowest id among the maxima, or -1 when no score is above -inf (the kernel then emits pad_id)."""
    c = candidates(scores(x, banned), 1)
    return int(c[0]) if len(c) else -1


def kept(x, banned, top_k, temperature, top_p, fp64=False, ranked=None):
    """(ids of the m kept ranks, cum [m], smallest |tail_j / P - (1 - top_p)| over j > 0) of one logits row, in fp32 in the
    contract's summation orders, or in fp64 (from the same fp32 scores, temperature and top_p). ids is empty when the row has no
    candidate. ranked: candidates(scores(x, banned), K) computed earlier for some K >= top_k (its first top_k entries are the
    candidates of top_k)."""
    f = np.float64 if fp64 else np.float32
    x = scores(x, banned)
    ids = candidates(x, top_k) if ranked is None else np.asarray(ranked)[:int(top_k)]
    if len(ids) == 0:
        return ids, np.zeros(0, f), np.inf
    xs = x[ids].astype(f)
    inv_t = f(1.0) / f(np.float32(temperature))
    w = np.exp((xs - xs[0]) * inv_t).astype(f)
    w[0] = f(1.0)
    m, margin = len(ids), np.inf
    tp = np.float32(top_p)
    if tp < 1.0 and len(ids) > 1:
        tail = np.cumsum(w[::-1], dtype=f)[::-1]            # tail_j = w_{k'-1} + ... + w_j, from the last rank upward
        thr = (f(1.0) - f(tp)) * tail[0]
        drop = tail <= thr
        drop[0] = False
        m = int(np.argmax(drop)) if drop.any() else len(ids)  # tail decreases with j: the dropped ranks are a suffix
        margin = float(np.min(np.abs(tail[1:].astype(np.float64) / float(tail[0]) - (1.0 - float(tp)))))
    cum = np.cumsum(w[:m], dtype=f)
    return ids[:m], cum, margin


def sample_row(x, banned, top_k, temperature, top_p, seed, row_ids, steps, fp64=False, ranked=None):
    """Tokens [len(row_ids), len(steps)] drawn from ONE logits row for every (row id, step); -1 where the row has no candidate.
    With fp64 also returns (dist [len(row_ids), len(steps)]: |u total - nearest cum_j| / total, margin: the row's top-p one)."""
    ids, cum, margin = kept(x, banned, top_k, temperature, top_p, fp64, ranked)
    u = uniform(seed, row_ids, steps)
    if len(ids) == 0:
        tok = np.full(u.shape, -1, dtype=np.int64)
        return (tok, np.full(u.shape, np.inf), margin) if fp64 else tok
    f = np.float64 if fp64 else np.float32
    target = u.astype(f) * cum[-1]
    j = (cum[None, None, :] > target[..., None]).argmax(-1)
    j = np.where(cum[-1] > target, j, len(ids) - 1)
    tok = ids[j].astype(np.int64)
    if not fp64:
        return tok
    dist = np.abs(target[..., None] - cum[None, None, :]).min(-1) / cum[-1]
    return tok, dist, margin
