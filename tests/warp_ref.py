"""numpy restatement of slam_sample_tokens_warped's contract (include/slam_engine.h) on top of tests/sampling_ref.py: the
ranked candidates and the top-p prefix come from there, the four warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff) and the
draw over the kept ranks are restated here. Two versions of the arithmetic, as in sampling_ref: fp32 in the contract's
summation orders, and fp64 (from the same fp32 scores and parameters), which also returns the smallest relative distance of
any decision from its threshold - the cases in which fp32 and fp64 may legitimately keep different sets:
  min_p       |w_j - min_p w_top| / (min_p w_top)
  typical_p   |c_i - mass| / mass for every i, and |s_cut - s_nb| / max(1, H, -log p_cut, -log p_nb) for the two neighbours of
              the cut element in the (s, rank) order: only those two comparisons can change the kept set. (s is a difference
              of two numbers of the size of H and -log p, so that size is the scale of its rounding error.)
  epsilon     |p_j - eps| / eps, eta |p_j - eta| / eta over the ranks that are not exempt
together with sampling_ref's top-p margin and, per draw, its distance |u total - nearest cum| / total.
A warp description is the tuple (min_p, typical_p, epsilon_cutoff, eta_cutoff); OFF switches all four off."""
import numpy as np

from tests import sampling_ref as R

OFF = (0.0, 1.0, 0.0, 0.0)


def _seq_sum(v, f):
    """v[0] + v[1] + ... in that order in precision f, starting from 0."""
    return np.cumsum(v, dtype=f)[-1] if len(v) else f(0.0)


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(np.asarray(a, np.float64) - float(b)) / abs(float(b))
    d = np.where(np.isnan(d), 0.0, d)
    return float(d.min()) if d.size else np.inf


def chain(x, banned, top_k, temperature, top_p, warp, fp64=False, ranked=None):
    """(ids [k'] of the ranked candidates, keep bool [k'] = the set S behind the chain, w [k'], margin) of one logits row.
    margin is the smallest of the relative distances listed above, top-p's included (inf where nothing was decided)."""
    f = np.float64 if fp64 else np.float32
    min_p, typical_p, eps_cut, eta_cut = (np.float32(v) for v in warp)
    xs_all = R.scores(x, banned)
    ids = R.candidates(xs_all, top_k) if ranked is None else np.asarray(ranked)[:int(top_k)]
    kk = len(ids)
    if kk == 0:
        return ids, np.zeros(0, bool), np.zeros(0, f), np.inf
    kept_ids, _, margin = R.kept(x, banned, top_k, temperature, top_p, fp64, ids)
    xs32 = xs_all[ids]
    xs = xs32.astype(f)
    inv_t = f(1.0) / f(np.float32(temperature))
    a = ((xs - xs[0]) * inv_t).astype(f)
    with np.errstate(under="ignore"):
        w = np.exp(a).astype(f)
    w[0] = f(1.0)
    rank = np.arange(kk)
    keep = rank < len(kept_ids)

    def normalise(keep):
        Z = _seq_sum(np.where(keep, w, f(0.0)), f)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (w / Z).astype(f), (a - np.log(Z)).astype(f)

    def entropy(keep, p, lp):
        with np.errstate(invalid="ignore"):
            term = np.where(keep & (w > 0), p * lp, f(0.0)).astype(f)
        return -_seq_sum(term, f)

    if min_p > 0:
        top = int(np.argmax(keep))
        thr = f(min_p) * w[top]
        others = keep & (rank != top)
        margin = min(margin, _rel(w[others], thr))
        keep = keep & ~(others & (w < thr))
    if typical_p < 1:
        p, lp = normalise(keep)
        H = entropy(keep, p, lp)
        with np.errstate(invalid="ignore"):
            s = np.abs(-lp - H).astype(f)
        S = rank[keep]
        order = S[np.lexsort((S, s[S]))]  # (s ascending, rank ascending)
        c = np.cumsum(p[order], dtype=f)
        mass = f(typical_p)
        last = min(int((c < mass).sum()), len(order) - 1)
        cut = order[last]
        margin = min(margin, _rel(c, mass))
        for nb in (last - 1, last + 1):
            if 0 <= nb < len(order):
                o = order[nb]
                scale = max(1.0, float(H), float(-lp[cut]), float(-lp[o]))
                with np.errstate(invalid="ignore"):
                    d = abs(float(s[cut]) - float(s[o])) / scale
                margin = min(margin, 0.0 if np.isnan(d) else d)
        keep = keep & ~(s > s[cut])
    for on, use_eta in ((eps_cut > 0, False), (eta_cut > 0, True)):
        if not on:
            continue
        p, lp = normalise(keep)
        if use_eta:
            H = entropy(keep, p, lp)
            thr = min(f(eta_cut), (np.sqrt(f(eta_cut)) * np.exp(-H)).astype(f))
        else:
            thr = f(eps_cut)
        top = int(np.argmax(keep))
        judged = keep & (xs32 != xs32[top])
        margin = min(margin, _rel(p[judged], thr))
        keep = keep & ~(judged & (p < thr))
    return ids, keep, w, margin


def kept_mask(x, banned, top_k, temperature, top_p, warp, fp64=False):
    """(bool [vocab]: the tokens the chain keeps, margin) - what HF's warpers leave finite."""
    ids, keep, _, margin = chain(x, banned, top_k, temperature, top_p, warp, fp64)
    mask = np.zeros(len(np.asarray(x)), bool)
    mask[ids[keep]] = True
    return mask, margin


def sample_row(x, banned, top_k, temperature, top_p, warp, seed, row_ids, steps, fp64=False, ranked=None):
    """Tokens [len(row_ids), len(steps)] drawn from ONE logits row for every (row id, step); -1 where the row has no candidate.
    With fp64 also returns (dist [len(row_ids), len(steps)]: |u total - nearest cum_j| / total, margin: the row's)."""
    ids, keep, w, margin = chain(x, banned, top_k, temperature, top_p, warp, fp64, ranked)
    u = R.uniform(seed, row_ids, steps)
    if len(ids) == 0:
        tok = np.full(u.shape, -1, dtype=np.int64)
        return (tok, np.full(u.shape, np.inf), margin) if fp64 else tok
    f = np.float64 if fp64 else np.float32
    ids = ids[keep]
    cum = np.cumsum(w[keep], dtype=f)
    target = u.astype(f) * cum[-1]
    j = (cum[None, None, :] > target[..., None]).argmax(-1)
    j = np.where(cum[-1] > target, j, len(ids) - 1)
    tok = ids[j].astype(np.int64)
    if not fp64:
        return tok
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.abs(target[..., None] - cum[None, None, :]).min(-1) / cum[-1]
    return tok, np.where(np.isnan(dist), 0.0, dist), margin
