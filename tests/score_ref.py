"""float64 restatement of slam_op_score_rows' row statistics and of slam_extend_score's output layout (include/slam_engine.h),
CPU only, numpy.

row_stats takes the scores of M rows ([M, V], any float dtype; the caller forms them in float64 from the bf16 operands) and
applies the contract: every score is read as the sampler reads it (NaN -> -inf, +inf -> FLT_MAX), masked columns count as -inf,
the vocabulary is cut into chunks of SCORE_CHUNK columns, each chunk yields (m_c, s_c, best value, best id), the chunks are
combined in chunk order by m = max m_c, S = s_c * exp(m_c - m) + S with chunks of m_c = -inf skipped, the best id moves to a
later chunk only on a strictly larger value (the lowest id among equals), lp = x_target - (m + log S). In float64 the order
of the sums is immaterial at the tolerances the tests use; the structure is kept so that the chunk rule itself is exercised.

extend_layout derives what slam_extend_score writes into lp_out / argmax_out from (ids, new_lens) and the per-position
log-softmax / argmax of the model, and extend_targets the targets its rows score.

op_inputs / OP_SHAPES are the inputs of the GPU op test (tests/test_gpu_score.py); the host test checks on them that near-ties
are rare enough for the argmax comparison to mean something."""
import numpy as np
import torch

SCORE_CHUNK = 512
FLT_MAX = float(np.finfo(np.float32).max)
NO_TARGET = -100

OP_KV = [(896, 502), (1536, 2049), (64, 152167)]
OP_M = [1, 15, 16, 17, 63, 64, 65, 130]
OP_ROWS = max(OP_M)
TIE_SHARE = 0.02  # rows whose top-1 / top-2 gap is below the margin: at most this share of a case


def clean(x):
    x = np.array(x, dtype=np.float64)
    x[np.isnan(x)] = -np.inf
    return np.minimum(x, FLT_MAX)


def row_stats(x, targets, mask=None, chunk=SCORE_CHUNK):
    """(lp float64 [M], argmax int64 [M]) of the scores x [M, V] at targets [M] under the contract."""
    x = clean(x)
    M, V = x.shape
    if mask is not None:
        x[:, np.asarray(mask[:V]) != 0] = -np.inf
    parts = []
    for c0 in range(0, V, chunk):
        xc = x[:, c0:c0 + chunk]
        m_c = xc.max(1)
        with np.errstate(invalid="ignore"):
            s_c = np.where(np.isneginf(m_c), 0.0, np.exp(xc - np.where(np.isneginf(m_c), 0.0, m_c)[:, None]).sum(1))
        bi = xc.argmax(1) + c0  # numpy's argmax is the first (lowest) index of the maximum
        parts.append((m_c, s_c, m_c.copy(), np.where(np.isneginf(m_c), -1, bi)))
    m = np.max(np.stack([p[0] for p in parts]), 0)
    S = np.zeros(M)
    bv = np.full(M, -np.inf)
    best = np.full(M, -1, dtype=np.int64)
    for m_c, s_c, v_c, i_c in parts:
        live = ~np.isneginf(m_c)
        with np.errstate(invalid="ignore"):
            S = np.where(live, s_c * np.exp(np.where(live, m_c - m, 0.0)) + S, S)
        take = v_c > bv
        bv = np.where(take, v_c, bv)
        best = np.where(take, i_c, best)
    targets = np.asarray(targets, dtype=np.int64)
    lp = np.zeros(M)
    has = (targets >= 0) & (targets < V)
    xt = x[np.arange(M), np.where(has, targets, 0)]
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.where(np.isneginf(m) | np.isneginf(xt), -np.inf, xt - (m + np.log(np.where(S > 0, S, 1.0))))
    lp[has] = val[has]
    return lp, best


def top2_gap(x, mask=None):
    """(gap between the two largest cleaned scores, max |finite score|) per row."""
    x = clean(x)
    if mask is not None:
        x[:, np.asarray(mask[:x.shape[1]]) != 0] = -np.inf
    part = np.partition(x, -2, axis=1)[:, -2:]
    fin = np.where(np.isfinite(x), np.abs(x), 0.0).max(1)
    with np.errstate(invalid="ignore"):
        return part[:, 1] - part[:, 0], fin


def tie_margin(absmax):
    return 1e-4 * np.maximum(1.0, absmax)


def op_inputs(K, V, seed=None):
    """X bf16 [OP_ROWS, K] = randn, W bf16 [V, K] = 0.03 randn, targets int64 [OP_ROWS] (every fifth row has none). The case
    of M rows is the first M rows: row m is the same row in every case."""
    g = torch.Generator().manual_seed(1000 + K + V if seed is None else seed)
    X = torch.randn(OP_ROWS, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(V, K, generator=g) * 0.03).to(torch.bfloat16)
    t = torch.randint(0, V, (OP_ROWS,), generator=g)
    t[3::5] = NO_TARGET
    return X, W, t


def scores_f64(X, W):
    return (X.double() @ W.double().t()).numpy()


def extend_targets(ids, new_lens):
    """targets [B, T] of the chunk's rows: row (b, t) scores ids[b][t + 1] when t + 1 < new_lens[b], nothing else."""
    ids = np.asarray(ids, dtype=np.int64)
    B, T = ids.shape
    tg = np.full((B, T), NO_TARGET, dtype=np.int64)
    for b in range(B):
        n = int(new_lens[b])
        for t in range(T):
            if t + 1 < n:
                tg[b, t] = ids[b, t + 1]
    return tg


def extend_layout(new_lens, T, row_lp, row_argmax, lp_before, argmax_before=None):
    """What slam_extend_score leaves in lp_out / argmax_out ([B, T] each) given, for every chunk row (b, t), row_lp[b][t] = the
    log-prob of that row's target and row_argmax[b][t] = its greedy token; lp_before / argmax_before: the buffers' contents
    before the call. Column 0 of lp_out keeps what it held."""
    lp = np.array(lp_before, dtype=np.float64, copy=True)
    B = len(new_lens)
    am = None if row_argmax is None else np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        n = min(max(int(new_lens[b]), 0), T)
        for t in range(1, T):
            lp[b, t] = row_lp[b][t - 1] if t < n else 0.0
        if am is not None:
            for t in range(n):
                am[b, t] = row_argmax[b][t]
    return lp, am
