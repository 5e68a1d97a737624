"""-m gpu: slam_op_score_rows, the LM head fused with the row statistics, against the float64 restatement (tests/score_ref.py).

Accuracy: the same rows go through the existing fp32 route - slam_op_gemm_skinny with fp32 output, then slam_token_logprobs -
and the new log-probs' largest error against float64 must be at most twice that route's on the same inputs, plus 1e-6. Both
routes round only in the fp32 accumulation and in expf / logf; the factor 2 covers the other summation order.
Argmax: exact wherever the float64 gap between the two largest scores exceeds 1e-4 max(1, max |x|); the excluded rows stay
at or under 2 % (test_score_host.py checks the same inputs on the CPU). Forced ties (duplicated W rows, made dominant: equal
accumulator bits) return the lower id, within a tile, across tiles, groups and chunks. The mask, one NaN and one +inf score,
run-to-run bits, and a row scored alone against the same row in the batch. Outputs and partials are pre-poisoned with NaN."""
import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import score_ref as R
from tests.gpu_util import lib, ptr, stream, sync
from tests.test_gpu_generate import _skinny

pytestmark = pytest.mark.gpu

_cache = {}


def _case(K, V):
    """The inputs of (K, V) on the device and their float64 reference over all OP_ROWS rows, computed once."""
    if (K, V) not in _cache:
        X, W, t = R.op_inputs(K, V)
        X, W, t = X.cuda(), W.cuda(), t.cuda()
        x64 = (X.double() @ W.double().t()).cpu().numpy()
        lp, am = R.row_stats(x64, t.cpu().numpy())
        gap, absmax = R.top2_gap(x64)
        _cache[(K, V)] = (X, W, t, lp, am, gap < R.tie_margin(absmax))
    return _cache[(K, V)]


def _score(X, W, t, mask=None):
    M, K = X.shape
    V = W.shape[0]
    nws = E.score_rows_workspace_bytes(M, V)
    assert nws == lib().slam_op_score_rows_workspace(M, V) and nws % 4 == 0
    ws = torch.full((nws // 4,), float("nan"), dtype=torch.float32, device="cuda")
    lp = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    am = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    rc = lib().slam_op_score_rows(ptr(X), ptr(W), ptr(t), ptr(mask), ptr(lp), ptr(am), M, V, K, ptr(ws), nws, stream())
    assert rc == 0, rc
    sync()
    return lp, am


def _route(X, W, t, mask=None):
    """The existing fp32 route: gemm_skinny (fp32 out), the mask as -inf, slam_token_logprobs."""
    M, V = X.shape[0], W.shape[0]
    Y = _skinny(X, W, None, None, True)
    if mask is not None:
        Y[:, mask[:V].bool()] = float("-inf")
    out = torch.full((M, 1), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(E.token_logprobs_workspace_bytes(M, V), dtype=torch.uint8, device="cuda")
    E.token_logprobs(Y, t.contiguous(), out, 0, ws)
    sync()
    return out[:, 0]


def _bits(a):
    return a.view(torch.int32)


def _check(tag, X, W, t, ref_lp, ref_am, near, mask=None):
    """One launch (and a second for the bits) against the reference and the route; returns (lp, argmax) on the CPU."""
    M = X.shape[0]
    lp, am = _score(X, W, t, mask)
    lp2, am2 = _score(X, W, t, mask)
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(am, am2), (tag, "two runs differ")
    got, rt = lp.double().cpu().numpy(), _route(X, W, t, mask).double().cpu().numpy()
    assert not np.isnan(got).any(), (tag, "poison left in lp")
    fin = np.isfinite(ref_lp)
    assert (got[~fin] == ref_lp[~fin]).all(), (tag, "-inf rows")
    e_new = float(np.abs(got[fin] - ref_lp[fin]).max()) if fin.any() else 0.0
    e_rt = float(np.abs(rt[fin] - ref_lp[fin]).max()) if fin.any() else 0.0
    print(f"[score] {tag}: lp max abs err {e_new:.3e} (fp32 route {e_rt:.3e}), near-tie rows {int(near.sum())}/{M}")
    assert e_new <= 2 * e_rt + 1e-6, (tag, e_new, e_rt)
    a = am.cpu().numpy()
    assert float(near.mean()) <= R.TIE_SHARE, (tag, "too many near-ties", float(near.mean()))
    assert (a[~near] == ref_am[~near]).all(), (tag, "argmax", np.nonzero(a != ref_am)[0][:8])
    assert ((a >= 0) & (a < W.shape[0])).all() or (ref_am == -1).any(), tag
    return lp, am


@pytest.mark.parametrize("M", R.OP_M)
@pytest.mark.parametrize("kv", R.OP_KV, ids=[f"K{k}-V{v}" for k, v in R.OP_KV])
def test_score_rows_vs_fp64(kv, M):
    K, V = kv
    X, W, t, ref_lp, ref_am, near = _case(K, V)
    lp, am = _check((K, V, M), X[:M], W, t[:M], ref_lp[:M], ref_am[:M], near[:M])
    none = (t[:M] == R.NO_TARGET).cpu()
    assert (lp.cpu()[none] == 0.0).all()
    # a row scored alone gives the bits it has in the batch: nothing depends on M, the row's index or the grid
    for m in sorted({0, M // 2, M - 1}):
        l1, a1 = _score(X[m:m + 1], W, t[m:m + 1])
        assert torch.equal(_bits(l1), _bits(lp[m:m + 1])) and torch.equal(a1, am[m:m + 1]), ((K, V, M), m, "alone vs batch")


def _dominant(K, V, M, pairs, seed):
    """X with a constant first column and W whose rows pairs[.] are copies of one another with a large first entry: those
    scores are equal bit for bit and about 30 above every other score of every row."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(V, K, generator=g) * 0.03).to(torch.bfloat16)
    X[:, 0] = 4.0
    for i, j in pairs:
        W[i, 0] = 8.0
        W[j] = W[i]
    return X.cuda(), W.cuda()


@pytest.mark.parametrize("pair", [(5, 9), (5, 21), (70, 300), (500, 515), (511, 512), (100, 2048)],
                         ids=["lanes", "tiles", "groups", "group-edge", "chunk-boundary", "chunks"])
def test_forced_tie_takes_the_lower_id(pair):
    K, V, M = 896, 2049, 17
    i, j = pair
    X, W = _dominant(K, V, M, [pair], seed=i * 7 + j)
    t = torch.full((M,), i, dtype=torch.int64, device="cuda")
    t[1::2] = j
    lp, am = _score(X, W, t)
    assert (am == i).all(), (pair, am.tolist())
    x64 = (X.double() @ W.double().t()).cpu().numpy()
    assert (x64[:, i] == x64[:, j]).all() and (np.sort(x64, 1)[:, -3] < x64[:, i] - 20).all()
    ref_lp, _ = R.row_stats(x64, t.cpu().numpy())
    e_new = float(np.abs(lp.double().cpu().numpy() - ref_lp).max())
    e_rt = float(np.abs(_route(X, W, t).double().cpu().numpy() - ref_lp).max())
    print(f"[score] tie {pair}: lp max abs err {e_new:.3e} (fp32 route {e_rt:.3e})")
    assert e_new <= 2 * e_rt + 1e-6, (pair, e_new, e_rt)
    # the two ids hold the same score: the same row scored at i and at j gives the same bits
    assert torch.equal(_bits(lp[0:1]), _bits(_score(X[:1], W, t[1:2])[0]))


def test_mask_moves_argmax_and_renormalises():
    K, V, M = 1536, 2049, 65
    X, W, t, ref_lp, ref_am, near = _case(K, V)
    X, t = X[:M], t[:M].clone()
    top = int(ref_am[0])
    t[1] = top  # a masked target
    mask = torch.zeros(V + 7, dtype=torch.uint8, device="cuda")
    mask[top] = 1
    mask[3] = 255
    x64 = (X.double() @ W.double().t()).cpu().numpy()
    mlp, mam = R.row_stats(x64, t.cpu().numpy(), mask.cpu().numpy())
    gap, absmax = R.top2_gap(x64, mask.cpu().numpy())
    lp, am = _check("mask", X, W, t, mlp, mam, gap < R.tie_margin(absmax), mask)
    assert int(am[0]) != top and int(am[0]) == int(mam[0]) and not bool(near[0])  # the runner-up
    assert float(lp[1]) == float("-inf") and mlp[1] == -np.inf
    assert (am != top).all() and (am != 3).all()
    plain, _ = _score(X, W, t)
    rows = [m for m in range(M) if int(t[m]) >= 0 and int(t[m]) not in (top, 3)]
    assert (lp[rows] >= plain[rows]).all() and float(lp[0]) > float(plain[0])  # mass left the softmax: every log-prob rises


def test_nan_and_inf_scores_read_as_the_sampler_reads_them():
    K, V, M = 896, 502, 16
    g = torch.Generator().manual_seed(11)
    X = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(V, K, generator=g) * 0.03).to(torch.bfloat16)
    X[:, 0] = 1.0
    X[:, 1] = 1.0
    a, b = 77, 300
    W[b, 0], W[b, 1] = float("inf"), float("-inf")  # inf - inf: a NaN score in every row
    t = torch.randint(0, V, (M,), generator=g)
    t[(t == a) | (t == b)] = 5
    t[0], t[1] = b, a
    X, W, t = X.cuda(), W.cuda(), t.cuda()
    x64 = (X.double() @ W.double().t()).cpu().numpy()
    assert np.isnan(x64[:, b]).all()
    ref_lp, ref_am = R.row_stats(x64, t.cpu().numpy())
    gap, absmax = R.top2_gap(x64)
    lp, am = _check("nan", X, W, t, ref_lp, ref_am, gap < R.tie_margin(absmax))
    assert float(lp[0]) == float("-inf") and (am != b).all()  # NaN counts as -inf: never the argmax, -inf as a target
    W[a, 0] = float("inf")  # and a +inf score: FLT_MAX
    x64 = (X.double() @ W.double().t()).cpu().numpy()
    assert np.isposinf(x64[:, a]).all()
    lp, am = _score(X, W, t)
    assert (am == a).all()
    assert float(lp[1]) == 0.0 and float(lp[0]) == float("-inf")
    assert (lp[2:] == -R.FLT_MAX).all()  # x - (FLT_MAX + logf(1)) in fp32: finite, as slam_token_logprobs gives
    assert torch.equal(_bits(lp), _bits(_route(X, W, t).contiguous()))
