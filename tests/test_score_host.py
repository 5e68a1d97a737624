"""CPU tier of slam_op_score_rows / slam_extend_score / UnitLM.score_continuations: the three new symbols are declared, exported
and bound; every argument refusal comes back before anything reaches the device (fake pointers and host-created engines, as in
test_extend_abi.py and test_opt_host.py); the Python argument errors; the float64 restatement (tests/score_ref.py) on values
that can be checked by hand; the lp_out / argmax_out layout on hand-written cases; and the share of near-tie rows in the
inputs of the GPU op test."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import score_ref as R

NEW = ["slam_extend_score", "slam_op_score_rows", "slam_op_score_rows_workspace"]
SLAM = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
OPT = (2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0)
E_INVAL, E_STATE, E_NOMEM = -1, -2, -3


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    assert hasattr(E.Engine, "extend_score") and hasattr(E, "score_rows") and hasattr(E, "score_rows_workspace_bytes")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))), "include", "slam_engine.h")).read()
    assert f"#define SLAM_SCORE_CHUNK {R.SCORE_CHUNK}" in hdr and E.SCORE_CHUNK == R.SCORE_CHUNK


def test_score_rows_refused_before_a_launch():
    lib = E.load_library()
    fake = C.c_void_p(1 << 20)
    M, V, K = 70, 5000, 896
    need = lib.slam_op_score_rows_workspace(M, V)
    assert need == E.score_rows_workspace_bytes(M, V) == M * -(-V // R.SCORE_CHUNK) * 16 + M * 4

    def call(X=fake, W=fake, tg=fake, mask=None, lp=fake, am=fake, M=M, V=V, K=K, ws=fake, nb=need):
        return lib.slam_op_score_rows(X, W, tg, mask, lp, am, M, V, K, ws, nb, None)

    odd = lambda k: C.c_void_p((1 << 20) + k)  # noqa: E731
    for kw in (dict(X=None), dict(W=None), dict(tg=None), dict(lp=None), dict(ws=None), dict(M=0), dict(M=-1), dict(M=1 << 26),
               dict(V=0), dict(V=-5), dict(V=65535 * 512 + 1), dict(K=0), dict(K=-8), dict(K=900), dict(K=4), dict(X=odd(8)), dict(W=odd(2)), dict(ws=odd(8)),
               dict(tg=odd(4)), dict(am=odd(4)), dict(lp=odd(2)), dict(nb=need - 1), dict(nb=0)):
        assert call(**kw) == E_INVAL, kw
    for M_, V_ in ((0, 502), (-1, 502), (3, 0), (3, -7), (1 << 26, 502), (3, 65535 * 512 + 1)):
        assert lib.slam_op_score_rows_workspace(M_, V_) == 0
    for M_, V_ in ((1, 1), (64, 512), (64, 513), (4096, 152167)):
        assert lib.slam_op_score_rows_workspace(M_, V_) == M_ * -(-V_ // R.SCORE_CHUNK) * 16 + M_ * 4


def test_extend_score_refused_before_a_launch():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    h = eng.h
    fake = C.c_void_p(1 << 20)

    def call(hh=h, ids=fake, new_lens=fake, lens=fake, B=2, T=16, logits=fake, lp=fake, am=fake):
        return lib.slam_extend_score(hh, ids, new_lens, lens, B, T, logits, lp, am, None)

    for kw in (dict(hh=None), dict(ids=None), dict(new_lens=None), dict(lens=None), dict(logits=None), dict(lp=None), dict(B=0),
               dict(B=-2), dict(T=0), dict(T=-1)):
        assert call(**kw) == E_INVAL, kw
    assert call() == E_STATE  # nothing bound
    assert b"params" in lib.slam_last_error(h) and b"workspace" in lib.slam_last_error(h)
    assert lib.slam_bind_params(h, fake, None) == 0
    assert call() == E_STATE  # parameters but no workspace
    assert lib.slam_bind_workspace(h, fake, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert call() == E_STATE  # no cache
    assert b"cache" in lib.slam_last_error(h)
    assert lib.slam_bind_kv_cache(h, fake, lib.slam_kv_cache_bytes(h, 200, 64), 200, 64) == 0
    assert call(B=2, T=129) == E_NOMEM
    assert call(B=129, T=1) == E_NOMEM
    assert call(B=2, T=65) == E_STATE
    assert b"capacity" in lib.slam_last_error(h)
    assert call() == E_STATE  # no prefill
    assert b"prefill" in lib.slam_last_error(h)
    assert call(am=None) == E_STATE  # argmax_out is optional: the refusal is still the missing prefill
    assert call(lp=None) == E_INVAL
    eng.close()


def test_extend_score_refuses_opt():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*OPT), 1, 128)
    h = eng.h
    fake = C.c_void_p(1 << 20)
    assert lib.slam_bind_params(h, fake, None) == 0
    assert lib.slam_bind_workspace(h, fake, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert lib.slam_extend_score(h, fake, fake, fake, 2, 16, fake, fake, fake, None) == E_INVAL
    assert b"Qwen2" in lib.slam_last_error(h)
    assert lib.slam_extend_score(h, fake, fake, fake, 2, 16, fake, None, fake, None) == E_INVAL
    eng.close()


def _bare():
    from slamkit_amd.model.unit_lm import UnitLM
    return UnitLM.__new__(UnitLM)  # host-only: the arguments are checked before the model is touched


@pytest.mark.parametrize("kw,what", [
    (dict(num_per_prompt=0), "num_per_prompt"), (dict(num_per_prompt=-2), "num_per_prompt"), (dict(num_per_prompt=1.0), "num_per_prompt"),
    (dict(num_per_prompt=True), "num_per_prompt"), (dict(score_chunk=0), "score_chunk"), (dict(score_chunk=2.0), "score_chunk"),
    (dict(score_chunk="4"), "score_chunk"), (dict(score_chunk=True), "score_chunk"), (dict(prefill_chunk=0), "prefill_chunk"),
    (dict(prefill_chunk=-1), "prefill_chunk"), (dict(num_per_prompt=3), "rows"), (dict(continuations=None), "continuations"),
    (dict(continuation_lengths=torch.zeros(3, dtype=torch.int32)), "continuation_lengths"),
])
def test_score_continuations_rejects_bad_arguments(kw, what):
    args = dict(input_ids=torch.zeros(2, 4, dtype=torch.long), continuations=torch.zeros(4, 5, dtype=torch.long), num_per_prompt=2)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _bare().score_continuations(**args)


def test_score_continuations_refuses_opt():
    m = _bare()
    m.config = types.SimpleNamespace(is_opt=True)
    with pytest.raises(ValueError, match="OPT"):
        m.score_continuations(torch.zeros(2, 4, dtype=torch.long), continuations=torch.zeros(2, 5, dtype=torch.long))


def test_restatement_on_hand_values():
    inf, nan = np.inf, np.nan
    x = np.array([[0.0, 0.0, nan, -inf], [inf, 1.0, 2.0, 3.0], [-inf, nan, -inf, -inf], [1.0, 3.0, 3.0, 2.0]])
    lp, am = R.row_stats(x, [1, 0, 2, -100])
    assert abs(lp[0] + np.log(2.0)) < 1e-12 and lp[1] == 0.0 and lp[2] == -inf and lp[3] == 0.0
    assert am.tolist() == [0, 0, -1, 1]  # the lowest id among equals; +inf reads as FLT_MAX; no score above -inf
    lp, am = R.row_stats(x, [2, 7, 0, 1])
    assert lp[0] == -inf and lp[1] == 0.0 and lp[2] == -inf  # a NaN target, an id outside the row, an empty row
    assert abs(lp[3] - (3.0 - np.log(np.exp(1.0) + 2 * np.exp(3.0) + np.exp(2.0)))) < 1e-12
    # the mask: the top-1 column leaves, argmax moves to the runner-up and lp renormalises; a masked target gives -inf
    mask = np.array([0, 1, 0, 0], np.uint8)
    lp, am = R.row_stats(x[3:], [2], mask)
    assert am.tolist() == [2] and abs(lp[0] - (3.0 - np.log(np.exp(1.0) + np.exp(3.0) + np.exp(2.0)))) < 1e-12
    assert R.row_stats(x[3:], [1], mask)[0][0] == -inf
    # more than one chunk: the chunk-order combination agrees with the plain definition; a tie across the boundary goes left
    g = np.random.default_rng(1)
    y = g.standard_normal((3, 1500)) * 4
    y[1, 700] = y[1, 100] = 50.0
    y[2, 1499] = y[2, 511] = y[2, 512] = 60.0
    t = [1499, 700, 5]
    lp, am = R.row_stats(y, t)
    ref = y[np.arange(3), t] - np.log(np.exp(y - y.max(1, keepdims=True)).sum(1)) - y.max(1)
    assert np.abs(lp - ref).max() < 1e-10
    assert am.tolist() == [int(y[0].argmax()), 100, 511]
    gap, absmax = R.top2_gap(y)
    assert gap[1] == 0.0 and gap[2] == 0.0 and gap[0] > 0 and absmax[2] == 60.0


def test_extend_layout_on_hand_cases():
    T = 4
    ids = np.array([[5, 6, 7, 8], [9, 1, 1, 1], [3, 4, 2, 2], [1, 1, 1, 1]])
    new_lens = [T, 1, 2, 0]
    tg = R.extend_targets(ids, new_lens)
    assert tg.tolist() == [[6, 7, 8, -100], [-100] * 4, [4, -100, -100, -100], [-100] * 4]
    row_lp = -np.arange(1.0, 17.0).reshape(4, 4)      # row (b, t)'s log-prob of its target: distinct values
    row_am = np.arange(100, 116).reshape(4, 4)
    poison = np.full((4, T), 777.0)
    lp, am = R.extend_layout(new_lens, T, row_lp, row_am, poison)
    assert lp[:, 0].tolist() == [777.0] * 4            # column 0 belongs to the caller
    assert lp[0, 1:].tolist() == [-1.0, -2.0, -3.0]    # new_lens = T: columns 1 .. T-1 from rows 0 .. T-2
    assert lp[1, 1:].tolist() == [0.0, 0.0, 0.0]       # new_lens = 1: nothing beyond column 0
    assert lp[2, 1:].tolist() == [-9.0, 0.0, 0.0]
    assert lp[3, 1:].tolist() == [0.0, 0.0, 0.0]       # new_lens = 0: zeros from column max(1, 0) on
    assert am.tolist() == [[100, 101, 102, 103], [104, -1, -1, -1], [108, 109, -1, -1], [-1] * 4]
    lp1, am1 = R.extend_layout([1, 0], 1, [[-5.0], [-6.0]], [[7], [8]], np.full((2, 1), 3.0))
    assert lp1.tolist() == [[3.0], [3.0]] and am1.tolist() == [[7], [-1]]  # T = 1: lp_out is not written at all


@pytest.mark.parametrize("kv", R.OP_KV, ids=[f"K{k}-V{v}" for k, v in R.OP_KV])
def test_gpu_op_inputs_have_few_near_ties(kv):
    K, V = kv
    X, W, t = R.op_inputs(K, V)
    x = R.scores_f64(X, W)
    gap, absmax = R.top2_gap(x)
    near = gap < R.tie_margin(absmax)
    for M in R.OP_M:
        share = float(near[:M].mean())
        print(f"[score] K={K} V={V} M={M}: near-tie rows {share:.1%} (smallest gap {gap[:M].min():.3e})")
        assert share <= R.TIE_SHARE, (K, V, M, share)
    assert ((t == R.NO_TARGET).sum() > 0) and ((t >= 0) & (t < V)).sum() > 100
