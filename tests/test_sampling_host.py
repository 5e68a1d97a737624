"""CPU tier of the device sampler (slam_sample_tokens / slam_sample_workspace_bytes, include/slam_engine.h): the host-only
workspace arithmetic, every refusal before a launch, and the contract's numpy restatement on its own: fp32 against fp64 away
from the boundaries, the uniformity of the draws, and the structure cases the kernels are later held to."""
import ctypes as C

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import sampling_ref as R

E_INVAL = -1


def test_symbols_exported_and_bound():
    lib = E.load_library()
    for n in ("slam_sample_workspace_bytes", "slam_sample_tokens"):
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    assert C.sizeof(E.SlamSampleDesc) == 40  # 4 x 4 bytes, the 8-byte seed, 3 x 4 bytes, padded to the seed's alignment


def test_workspace_bytes_host_only_and_monotone():
    f = E.sample_workspace_bytes
    Bs, Vs, Ks = (1, 3, 8, 64, 96), (1, 17, 502, 2048, 2049, 4099, 152167, 152576), (1, 25, 40, 256)
    for B in Bs:
        for V in Vs:
            for k in Ks:
                assert f(B, V, k) > 0, (B, V, k)
    for V in Vs:
        for k in Ks:
            assert all(f(a, V, k) <= f(b, V, k) for a, b in zip(Bs, Bs[1:]))
    for B in Bs:
        for k in Ks:
            assert all(f(B, a, k) <= f(B, b, k) for a, b in zip(Vs, Vs[1:]))
        for V in Vs:
            assert all(f(B, V, a) <= f(B, V, b) for a, b in zip(Ks, Ks[1:]))
    assert f(0, 502, 25) == 0 and f(8, 0, 25) == 0  # nothing to size


def _desc(**kw):
    d = dict(do_sample=1, top_k=25, temperature=0.8, top_p=1.0, seed=11, step=0, pad_id=0, n_eos=0)
    d.update(kw)
    return E.SlamSampleDesc(**d)


def test_refusals_before_any_launch():
    lib = E.load_library()
    fake, nxt, ws, eos = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22), C.c_void_p(1 << 23)
    B, V = 8, 502
    nws = lib.slam_sample_workspace_bytes(B, V, 25)

    def call(logits=fake, B=B, V=V, desc=None, use_desc=True, eos_ids=None, nxt=nxt, ws=ws, nws=nws, **kw):
        d = C.byref(desc if desc is not None else _desc(**kw)) if use_desc else None
        return lib.slam_sample_tokens(logits, B, V, None, d, None, eos_ids, None, nxt, None, 0, ws, nws, None)

    assert call(logits=None) == E_INVAL
    assert call(use_desc=False) == E_INVAL
    assert call(nxt=None) == E_INVAL
    for b in (0, -1):
        assert call(B=b) == E_INVAL
    for v in (0, -5):
        assert call(V=v) == E_INVAL
    for k in (0, -1, 257, 300):
        assert call(top_k=k) == E_INVAL
    assert call(do_sample=2) == E_INVAL
    for t in (0.0, -0.8, float("nan")):
        assert call(temperature=t) == E_INVAL
        assert call(do_sample=0, temperature=t) == E_INVAL
    for p in (0.0, -0.1, 1.0001, float("nan")):
        assert call(top_p=p) == E_INVAL
    for n in (-1, 17):
        assert call(n_eos=n, eos_ids=eos) == E_INVAL
    assert call(n_eos=1, eos_ids=None) == E_INVAL
    assert call(nws=nws - 1) == E_INVAL
    assert call(ws=None) == E_INVAL
    assert call(top_k=26) == E_INVAL  # the workspace was sized for 25
    assert call(do_sample=0, nws=lib.slam_sample_workspace_bytes(B, V, 1) - 1) == E_INVAL  # greedy sizes for k = 1


def _row(V, scale=3.0):
    return (torch.randn(V, generator=torch.Generator().manual_seed(V)) * scale).numpy()


# ---- the restatement on its own ----------------------------------------------------------------------------------------------
def test_philox_draws_are_keyed_on_seed_row_and_step():
    u = R.uniform(11, [0, 1, (1 << 32) + 1], [0, 1, 2])
    assert u.shape == (3, 3) and (u >= 0).all() and (u < 1).all()
    assert len(np.unique(u)) == 9  # row ids that differ only above bit 32 differ too
    assert (u * 2.0 ** 24 == np.floor(u * 2.0 ** 24)).all()  # 24 bits: exact in fp32
    assert (R.uniform(11, [1], [2]) == u[1, 2]).all()  # one draw does not depend on what is drawn beside it
    assert (R.uniform(12, [0, 1, (1 << 32) + 1], [0, 1, 2]) != u).any()
    assert (R.uniform(11 + (1 << 32), [0], [0]) != u[0, 0]).all()


def test_scores_and_candidates():
    x = np.array([1.0, np.nan, np.inf, -np.inf, 5.0, -0.0, 0.0, 5.0], dtype=np.float32)
    s = R.scores(x, banned=[0, 0, 0, 0, 1, 0, 0, 0])
    assert s[1] == -np.inf and s[4] == -np.inf and s[2] == np.finfo(np.float32).max
    assert list(R.candidates(s, 25)) == [2, 7, 0, 5, 6]  # k' = the number of finite scores; -0 ties with +0 by id
    assert list(R.candidates(s, 2)) == [2, 7]
    assert R.greedy(x) == 2 and R.greedy(x, banned=[0, 0, 1, 0, 0, 0, 0, 0]) == 4
    assert R.greedy(np.full(9, -np.inf)) == -1 and R.greedy(np.full(9, np.nan)) == -1
    eq = np.full(100, 0.25, dtype=np.float32)
    assert list(R.candidates(R.scores(eq), 25)) == list(range(25))
    assert R.greedy(eq) == 0


def test_top_p_cut_is_hf_rule():
    """HF's TopPLogitsWarper on the top-k survivors: ascending sort, softmax, cumsum, drop cum <= 1 - top_p, keep the last."""
    x = _row(502)
    for top_p in (0.9, 0.7, 0.3):
        ids, _, _ = R.kept(x, None, 25, 0.8, top_p, fp64=True)
        s = torch.from_numpy(x).double() / float(np.float32(0.8))
        top = s.topk(25)
        srt, idx = torch.sort(top.values, descending=False)
        drop = srt.softmax(-1).cumsum(-1) <= (1 - float(np.float32(top_p)))
        drop[-1] = False
        want = sorted(top.indices[idx[~drop]].tolist())
        assert sorted(ids.tolist()) == want, top_p


@pytest.mark.parametrize("V,k,T,top_p", [(17, 40, 0.5, 1.0), (502, 25, 0.8, 1.0), (502, 25, 0.8, 0.9), (502, 256, 1.3, 0.7),
                                         (502, 1, 1.0, 1.0), (4099, 25, 0.8, 0.9), (152167, 25, 0.8, 1.0)])
def test_fp32_and_fp64_restatements_agree_away_from_boundaries(V, k, T, top_p):
    x = _row(V)
    rows, steps = np.arange(64), np.arange(64)
    t32 = R.sample_row(x, None, k, T, top_p, 11, rows, steps)
    t64, dist, margin = R.sample_row(x, None, k, T, top_p, 11, rows, steps, fp64=True)
    near = dist <= 1e-5
    print(f"V {V} k {k} T {T} p {top_p}: {near.mean():.4%} of draws near a boundary, top-p margin {margin:.3e}")
    assert near.mean() <= 0.03
    if margin > 1e-5:
        assert (t32[~near] == t64[~near]).all()
    kk = min(k, V)
    assert set(np.unique(t64)) <= set(R.candidates(R.scores(x), kk).tolist())


# 99.9 % quantiles of chi-square with m - 1 degrees of freedom
CHI2_999 = {24: 51.18, 7: 24.32}


@pytest.mark.parametrize("V,k,T,top_p,m", [(502, 25, 0.8, 1.0, 25), (502, 25, 0.8, 0.9, 8), (152167, 25, 0.8, 1.0, 25)])
def test_draws_follow_the_kept_set_probabilities(V, k, T, top_p, m):
    x = _row(V)
    ids, cum, _ = R.kept(x, None, k, T, top_p)
    assert len(ids) == m
    p = np.diff(np.concatenate([[0.0], cum.astype(np.float64)])) / float(cum[-1])
    tok = R.sample_row(x, None, k, T, top_p, 11, np.arange(64), np.arange(256))
    n = tok.size
    counts = np.array([(tok == i).sum() for i in ids], dtype=np.float64)
    assert counts.sum() == n == 16384
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    print(f"V {V} k {k} T {T} p {top_p}: chi-square {chi2:.1f} over {m} kept, bound {CHI2_999[m - 1]}")
    assert chi2 < CHI2_999[m - 1]
