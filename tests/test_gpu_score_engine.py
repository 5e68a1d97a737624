"""-m gpu: slam_extend_score on the tiny and wide golden models of test_gpu_extend.py, prompts of 37, 20 and 5 tokens.

Ragged chunks of T in {1, 5, 16, 17, 70} columns with new_lens holding 0, 1 and T: the cache, lens and logits_out carry the
bits slam_extend leaves on a second, identically prefilled cache; lp_out / argmax_out have the layout of tests/score_ref.py
(column 0 keeps its poison, zeros and -1 behind a row's tokens, inert rows untouched). Accuracy per row, the project's own bar:
the RMS over positions of lp - log_softmax(oracle logits)[target] is at most 2 LOGITS_TOL rms(oracle logits), against the fp32
oracle and against one full forward. argmax_out at a row's last real position equals argmax(logits_out[b]) unless the fp32
gap is below the near-tie margin. A chunk's last position chained into the next chunk through slam_token_logprobs matches the
single-chunk run within the op bound: both calls have the single run's width, so the hidden rows are the same and the two
numbers are the two fp32 routes of tests/test_gpu_score.py on one row. With e = the existing route's largest error against
float64 (gemm_skinny fp32 + slam_token_logprobs, measured here on that test's inputs - the reference route, not the code under
test), the link's one side is within e of the float64 value and the other within the op bound 2 e + 1e-6, so they differ by at
most 3 e + 1e-6. The logit mask is honoured."""
import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import score_ref as R
from tests.gpu_util import sync
from tests.test_gpu_extend import POISON, _poisoned_cache
from tests.test_gpu_generate import LOGITS_TOL, _mk, _tiny, _wide

pytestmark = pytest.mark.gpu

LENS = [37, 20, 5]
TMAX = 70
CAP = 256
SENT = 777.0
_models = {}
_route_err = []


def _chain_tol():
    """3 e + 1e-6, e = the largest |fp32 route - float64| over the op test's inputs (all rows of every (K, V) case)."""
    if not _route_err:
        from tests.test_gpu_score import _case, _route
        e = 0.0
        for K, V in R.OP_KV:
            X, W, t, ref_lp, _, _ = _case(K, V)
            fin = np.isfinite(ref_lp)
            e = max(e, float(np.abs(_route(X, W, t).double().cpu().numpy()[fin] - ref_lp[fin]).max()))
        _route_err.append(e)
    return 3 * _route_err[0] + 1e-6


def _setup(which):
    """Model, the rows' full sequences (prompt + TMAX continuation tokens), oracle and forward logits: computed once."""
    if which not in _models:
        cfg, sd = _tiny() if which == "tiny" else _wide()
        m = _mk(cfg, sd, max_tokens=1024, seed=7)
        sd_bf = {k: v.float() for k, v in m.state_dict(torch.bfloat16).items()}
        g = torch.Generator().manual_seed(17)
        B = len(LENS)
        full = torch.zeros(B, max(LENS) + TMAX, dtype=torch.long)
        for b, ln in enumerate(LENS):
            full[b, 0] = 1
            full[b, 1:ln + TMAX] = torch.randint(2, cfg.vocab, (ln + TMAX - 1,), generator=g)
        ref = O.model_forward(cfg, sd_bf, full).double()
        fwd = m(input_ids=full).logits.float().cpu().double()
        _models[which] = (cfg, m, full, ref, fwd)
    return _models[which]


def _prefilled(m, cfg, full):
    """A poisoned cache bound and prefilled with the prompts: (cache view, lens, logits)."""
    B, T = len(LENS), max(LENS)
    dev = m.device
    kv = _poisoned_cache(m, cfg, B, CAP)
    lens_d = torch.tensor(LENS, dtype=torch.int32, device=dev)
    logits = torch.full((B, cfg.vocab), float("nan"), dtype=torch.float32, device=dev)
    ids = torch.zeros(B, T, dtype=torch.long)
    for b, ln in enumerate(LENS):
        ids[b, :ln] = full[b, :ln]
    m.engine.prefill(ids.to(dev).contiguous(), lens_d, B, T, logits)
    sync()
    return kv, lens_d, logits


def _chunk(full, base, new, T, dev):
    ids = torch.zeros(len(base), T, dtype=torch.long)
    for b, (p, n) in enumerate(zip(base, new)):
        ids[b, :n] = full[b, p:p + n]
    return ids.to(dev).contiguous()


def _col0(logits, ids, lp, V):
    """Column 0 the way the contract asks the caller to fill it."""
    ws = torch.empty(E.token_logprobs_workspace_bytes(ids.shape[0], V), dtype=torch.uint8, device=ids.device)
    E.token_logprobs(logits, ids[:, 0].contiguous(), lp, 0, ws)


def _ref_lp(logits64, full, base, new, mask=None):
    """Per row: float64 log-softmax of the reference logits at the chunk's tokens, positions base .. base + new - 1."""
    out = []
    for b, (p, n) in enumerate(zip(base, new)):
        x = logits64[b, p - 1:p - 1 + n].clone()
        if mask is not None:
            x[:, mask] = float("-inf")
        out.append(torch.log_softmax(x, -1).gather(1, full[b, p:p + n, None])[:, 0].numpy())
    return out


def _new_lens(T):
    base = [T, 1, 0]
    r = T % 3
    return base[r:] + base[:r]


@pytest.mark.parametrize("T", [1, 5, 16, 17, 70])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_ragged_chunk(which, T):
    cfg, m, full, ref, fwd = _setup(which)
    dev, B, V = m.device, len(LENS), cfg.vocab
    new = _new_lens(T)
    assert {0, 1, T} <= set(new)
    ids = _chunk(full, LENS, new, T, dev)
    new_d = torch.tensor(new, dtype=torch.int32, device=dev)
    # slam_extend on one prefilled cache
    kv_a, lens_a, logits_a = _prefilled(m, cfg, full)
    inert = [b for b in range(B) if new[b] == 0]
    for b in inert:
        logits_a[b].fill_(SENT)
    m.engine.extend(ids, new_d, lens_a, B, T, logits_a)
    sync()
    kv_a = kv_a.clone()
    # slam_extend_score on a second one
    kv_b, lens_b, logits_b = _prefilled(m, cfg, full)
    kv0 = kv_b.clone()
    lp = torch.full((B, T), SENT, dtype=torch.float32, device=dev)
    am = torch.full((B, T), -7, dtype=torch.int64, device=dev)
    _col0(logits_b, ids, lp, V)
    for b in inert:
        logits_b[b].fill_(SENT)
        lp[b, 0] = SENT
    m.engine.extend_score(ids, new_d, lens_b, B, T, logits_b, lp, am)
    sync()
    assert torch.equal(kv_b, kv_a), (which, T, "cache bits differ from slam_extend's")
    assert torch.equal(lens_b, lens_a) and lens_b.tolist() == [p + n for p, n in zip(LENS, new)]
    assert torch.equal(logits_b.view(torch.int32), logits_a.view(torch.int32)), (which, T, "logits_out bits differ")
    for b in inert:
        assert (logits_b[b] == SENT).all() and torch.equal(kv_b[:, :, b], kv0[:, :, b]), (which, T, b, "inert row was written")
        assert float(lp[b, 0]) == SENT, (which, T, b, "column 0 was written")
    # without argmax_out: the same lp bits
    _, lens_c, logits_c = _prefilled(m, cfg, full)
    lp_c = torch.full((B, T), SENT, dtype=torch.float32, device=dev)
    m.engine.extend_score(ids, new_d, lens_c, B, T, logits_c, lp_c, None)
    sync()
    assert torch.equal(lp_c[:, 1:].view(torch.int32), lp[:, 1:].view(torch.int32)) and (lp_c[:, 0] == SENT).all()
    # layout: what the rows' own values give through the restatement's layout rule
    got, gam = lp.cpu().double().numpy(), am.cpu().numpy()
    row_lp = [[got[b, t + 1] if t + 1 < T else 0.0 for t in range(T)] for b in range(B)]
    want_lp, want_am = R.extend_layout(new, T, row_lp, gam, got)
    assert np.array_equal(want_lp, got) and np.array_equal(want_am, gam), (which, T, "layout")
    for b in range(B):
        n = new[b]
        assert (got[b, max(1, n):] == 0.0).all() and (gam[b, n:] == -1).all()
        assert ((gam[b, :n] >= 0) & (gam[b, :n] < V)).all() and np.isfinite(got[b, :n]).all()
    # accuracy per row (column 0 is slam_token_logprobs on the prefill logits: the chain's first link)
    for name, logits64 in (("oracle", ref), ("forward", fwd)):
        want = _ref_lp(logits64, full, LENS, new)
        for b in range(B):
            n = new[b]
            if n == 0:
                continue
            rows = ref[b, LENS[b] - 1:LENS[b] - 1 + n]
            bar = 2 * LOGITS_TOL * float(rows.pow(2).mean().sqrt())
            rms = float(np.sqrt(np.mean((got[b, :n] - want[b]) ** 2)))
            print(f"[extend_score] {which} T={T} row {b} ({n} positions) vs {name}: lp rms diff {rms:.3e} (bar {bar:.3e})")
            assert rms <= bar, (which, T, b, name, rms, bar)
    # the greedy token behind a row's last real position against the last-token logits the call returned
    for b in range(B):
        n = new[b]
        if n == 0:
            continue
        x = logits_b[b].double().cpu().numpy()[None]
        gap, absmax = R.top2_gap(x)
        if gap[0] >= R.tie_margin(absmax)[0]:
            assert gam[b, n - 1] == int(x[0].argmax()), (which, T, b, "argmax_out vs argmax(logits_out)")


@pytest.mark.parametrize("T", [5, 16, 17, 70])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_chunks_chain_through_token_logprobs(which, T):
    cfg, m, full, ref, fwd = _setup(which)
    dev, B, V = m.device, len(LENS), cfg.vocab
    s = T // 2
    whole = [T, T - 1, 2]
    whole_d = torch.tensor(whole, dtype=torch.int32, device=dev)
    ids = _chunk(full, LENS, whole, T, dev)
    _, lens_a, logits_a = _prefilled(m, cfg, full)
    one = torch.full((B, T), SENT, dtype=torch.float32, device=dev)
    _col0(logits_a, ids, one, V)
    m.engine.extend_score(ids, whole_d, lens_a, B, T, logits_a, one, None)
    # the same tokens in two calls of the same width: s (at most) first, the rest behind
    first = [min(n, s) for n in whole]
    rest = [n - f for n, f in zip(whole, first)]
    _, lens_b, logits_b = _prefilled(m, cfg, full)
    ids1 = _chunk(full, LENS, first, T, dev)
    lp1 = torch.full((B, T), SENT, dtype=torch.float32, device=dev)
    _col0(logits_b, ids1, lp1, V)
    m.engine.extend_score(ids1, torch.tensor(first, dtype=torch.int32, device=dev), lens_b, B, T, logits_b, lp1, None)
    base2 = [p + f for p, f in zip(LENS, first)]
    ids2 = _chunk(full, base2, rest, T, dev)
    lp2 = torch.full((B, T), SENT, dtype=torch.float32, device=dev)
    _col0(logits_b, ids2, lp2, V)
    m.engine.extend_score(ids2, torch.tensor(rest, dtype=torch.int32, device=dev), lens_b, B, T, logits_b, lp2, None)
    sync()
    assert lens_b.tolist() == lens_a.tolist() == [p + n for p, n in zip(LENS, whole)]
    one, lp1, lp2 = one.cpu().double(), lp1.cpu().double(), lp2.cpu().double()
    for b in range(B):
        f, r = first[b], rest[b]
        if r == 0:
            continue
        d = abs(float(lp2[b, 0]) - float(one[b, f]))  # the link: slam_token_logprobs on call 1's logits_out vs the fused head
        print(f"[extend_score] {which} T={T} row {b}: chained link |diff| {d:.3e} (bound {_chain_tol():.3e})")
        assert d <= _chain_tol(), (which, T, b, "chained link", d)
        chained = torch.cat([lp1[b, :f], lp2[b, :r]])
        rows = ref[b, LENS[b] - 1:LENS[b] - 1 + whole[b]]
        bar = 2 * LOGITS_TOL * float(rows.pow(2).mean().sqrt())
        rms = float((chained - one[b, :whole[b]]).pow(2).mean().sqrt())
        assert rms <= bar, (which, T, b, "chained vs single chunk", rms, bar)


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_logit_mask_is_honoured(which):
    cfg, m, full, ref, fwd = _setup(which)
    dev, B, V, T = m.device, len(LENS), cfg.vocab, 17
    new = [T, 9, 0]
    ids = _chunk(full, LENS, new, T, dev)
    # masked: the oracle's top-1 at row 0's second chunk position, one of row 1's targets, and two more columns
    top = int(ref[0, LENS[0]].argmax())
    tgt = int(full[1, LENS[1] + 4])
    cols = sorted({top, tgt, 2, V - 1})
    mask = torch.zeros(m.engine.padded_vocab(), dtype=torch.uint8, device=dev)
    mask[torch.tensor(cols, device=dev)] = 1
    _, lens_d, logits = _prefilled(m, cfg, full)
    lp = torch.full((B, T), SENT, dtype=torch.float32, device=dev)
    am = torch.full((B, T), -7, dtype=torch.int64, device=dev)
    m.engine.set_logit_mask(mask)
    try:
        m.engine.extend_score(ids, torch.tensor(new, dtype=torch.int32, device=dev), lens_d, B, T, logits, lp, am)
        sync()
    finally:
        m.engine.set_logit_mask(None)
    got, gam = lp.cpu().double().numpy(), am.cpu().numpy()
    want = _ref_lp(ref, full, LENS, new, mask=torch.tensor(cols))
    for b in range(B):
        n = new[b]
        assert not np.isin(gam[b, :n], cols).any(), (which, b, "a masked column is the argmax")
        if n < 2:
            continue
        w, g = want[b][1:], got[b, 1:n]
        dead = np.isneginf(w)
        assert (g[dead] == -np.inf).all(), (which, b, "masked target")
        rows = ref[b, LENS[b]:LENS[b] - 1 + n]
        bar = 2 * LOGITS_TOL * float(rows.pow(2).mean().sqrt())
        rms = float(np.sqrt(np.mean((g[~dead] - w[~dead]) ** 2)))
        print(f"[extend_score] {which} mask row {b}: lp rms diff {rms:.3e} (bar {bar:.3e}), {int(dead.sum())} masked targets")
        assert rms <= bar, (which, b, rms, bar)
    assert np.isneginf(got[1, 4]) and float(lp[2, 0]) == SENT
    assert int(gam[0, 0]) != top
