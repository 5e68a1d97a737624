"""-m gpu: UnitLM.score_continuations on the tiny golden model, prompts of 37, 20 and 5 tokens.

It scores what generate(do_sample=True, sampler="engine", num_return_sequences=2, return_logprobs=True) sampled, an EOS firing
mid-way, in one block and in blocks of 16 columns: per row the RMS difference to generate's own log-probs stays within the
project's bar, 2 LOGITS_TOL rms(logits of the row's continuation positions), and behind the EOS both are zero. Row sums
against sequence_logps of the concatenated batch within bar x sqrt(length). return_argmax against a greedy generate up to the
first near-tie. num_per_prompt = 3 from two prompts against the repeated batch with num_per_prompt = 1. ignore_tokens."""
import math

import pytest
import torch

from tests.test_gpu_generate import LOGITS_TOL, _mk, _tiny

pytestmark = pytest.mark.gpu

LENS = [37, 20, 5]


@pytest.fixture(scope="module")
def tiny():
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=512, seed=7)
    g = torch.Generator().manual_seed(23)
    T = max(LENS)
    ids = torch.zeros(len(LENS), T, dtype=torch.long)
    am = torch.zeros_like(ids)
    for b, ln in enumerate(LENS):
        ids[b, :ln] = torch.randint(2, cfg.vocab, (ln,), generator=g)
        am[b, :ln] = 1
    return cfg, m, ids, am


def _concat(ids, am, n, cont, clen):
    """The [B n, T + T_c] batch the parent route scores: prompt tokens, then the row's continuation, right-padded; labels hold
    the continuation tokens only. Also the prompt lengths per row."""
    plen = am.sum(1).repeat_interleave(n).tolist()
    R_ = cont.shape[0]
    L = max(p + int(c) for p, c in zip(plen, clen))
    full = torch.zeros(R_, L, dtype=torch.long)
    lab = torch.full((R_, L), -100, dtype=torch.long)
    for r in range(R_):
        p, c = plen[r], int(clen[r])
        src = ids[r // n][am[r // n] != 0]
        full[r, :p] = src
        full[r, p:p + c] = cont[r, :c]
        lab[r, p:p + c] = cont[r, :c]
    return full, lab, plen


def _bars(m, full, plen, clen):
    """Per row: 2 LOGITS_TOL rms(forward logits at the positions that predict the row's continuation); and those logits."""
    lg = m(input_ids=full).logits.float().cpu()
    bars = []
    for r, (p, c) in enumerate(zip(plen, clen)):
        c = int(c)
        bars.append(2 * LOGITS_TOL * float(lg[r, p - 1:p - 1 + max(c, 1)].pow(2).mean().sqrt()))
    return bars, lg


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt()) if a.numel() else 0.0


@pytest.fixture(scope="module")
def sampled(tiny):
    cfg, m, ids, am = tiny
    kw = dict(attention_mask=am, do_sample=True, sampler="engine", num_return_sequences=2, temperature=0.8, top_k=25,
              max_new_tokens=24, pad_token_id=0, seed=11)
    free = m.generate(ids, eos_token_id=[], **kw).cpu()
    T_in = ids.shape[1]
    eos = sorted({int(free[1, T_in + 3]), int(free[4, T_in + 9])})  # the same draws repeat up to each row's EOS
    out = m.generate(ids, eos_token_id=eos, return_logprobs=True, **kw)
    seq, lp = out.sequences.cpu(), out.logprobs.cpu()
    cont = seq[:, T_in:]
    hit = torch.isin(cont, torch.tensor(eos))
    clen = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full((cont.shape[0],), cont.shape[1]))
    assert int(clen.min()) < cont.shape[1] and int(clen.max()) > int(clen.min()), "the EOS must fire mid-way"
    full, lab, plen = _concat(ids, am, 2, cont, clen)
    bars, _ = _bars(m, full, plen, clen)
    return cont, clen, lp, full, lab, bars


@pytest.mark.parametrize("score_chunk", [None, 16])
def test_scores_what_generate_sampled(tiny, sampled, score_chunk):
    cfg, m, ids, am = tiny
    cont, clen, lp, full, lab, bars = sampled
    got = m.score_continuations(ids, am, continuations=cont, continuation_lengths=clen, num_per_prompt=2,
                                score_chunk=score_chunk, prefill_chunk=None if score_chunk is None else 16)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == cont.shape
    got = got.cpu()
    for r in range(cont.shape[0]):
        c = int(clen[r])
        assert (got[r, c:] == 0).all() and (lp[r, c:] == 0).all(), (r, "behind the EOS both are zero")
        assert torch.isfinite(got[r, :c]).all() and (got[r, :c] <= 0).all()
        d = _rms(got[r, :c], lp[r, :c])
        print(f"[score_continuations] chunk {score_chunk} row {r} ({c} tokens): rms diff to generate's log-probs {d:.3e} (bar {bars[r]:.3e})")
        assert d <= bars[r], (score_chunk, r, d, bars[r])
    # row sums against the parent route: sequence_logps over the concatenated batch
    ll, cnt = m.sequence_logps(full, lab, padding_free=False)
    ll, cnt = ll.cpu(), cnt.cpu()
    assert cnt.tolist() == [float(c) for c in clen.tolist()]
    for r in range(cont.shape[0]):
        d = abs(float(got[r].double().sum()) - float(ll[r]))
        assert d <= bars[r] * math.sqrt(int(clen[r])), (score_chunk, r, d, bars[r])


def test_argmax_reproduces_greedy_generate(tiny):
    cfg, m, ids, am = tiny
    T_in, NEW = ids.shape[1], 16
    seq = m.generate(ids, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], pad_token_id=0).cpu()
    cont = seq[:, T_in:]
    assert cont.shape == (len(LENS), NEW)
    lp, amx = m.score_continuations(ids, am, continuations=cont, score_chunk=5, return_argmax=True)
    lp, amx = lp.cpu(), amx.cpu()
    assert amx.dtype == torch.int64 and amx.shape == cont.shape and torch.isfinite(lp).all()
    clen = torch.full((len(LENS),), NEW)
    full, lab, plen = _concat(ids, am, 1, cont, clen)
    bars, lg = _bars(m, full, plen, clen)
    for r, p in enumerate(plen):
        top = lg[r, p - 1:p - 1 + NEW].topk(2, -1).values
        low = ((top[:, 0] - top[:, 1]) < bars[r]).nonzero()
        trust = int(low[0]) if len(low) else NEW  # positions before the first near-tie must agree exactly
        diff = (amx[r] != cont[r]).nonzero()
        first = int(diff[0]) if len(diff) else NEW
        print(f"[score_continuations] greedy row {r}: agrees for {first} positions, first near-tie at {trust}")
        assert first >= trust, (r, "argmax left the greedy continuation at", first, "before the first near-tie", trust)
    # pads: -1 and 0.0
    short = torch.tensor([NEW, 3, 0])
    lp2, am2 = m.score_continuations(ids, am, continuations=cont, continuation_lengths=short, score_chunk=5, return_argmax=True)
    lp2, am2 = lp2.cpu(), am2.cpu()
    for r, c in enumerate(short.tolist()):
        assert (am2[r, c:] == -1).all() and (lp2[r, c:] == 0).all() and (am2[r, :c] >= 0).all()
        assert _rms(lp2[r, :c], lp[r, :c]) <= bars[r]


def test_n_per_prompt_equals_the_repeated_batch(tiny):
    cfg, m, ids, am = tiny
    ids2, am2, n, Tc = ids[:2], am[:2], 3, 12
    g = torch.Generator().manual_seed(31)
    cont = torch.randint(2, cfg.vocab, (2 * n, Tc), generator=g)
    clen = torch.tensor([Tc, 0, 7, 1, Tc, 5])
    a = m.score_continuations(ids2, am2, continuations=cont, continuation_lengths=clen, num_per_prompt=n, score_chunk=5).cpu()
    b = m.score_continuations(ids2.repeat_interleave(n, 0), am2.repeat_interleave(n, 0), continuations=cont,
                              continuation_lengths=clen, num_per_prompt=1).cpu()
    full, lab, plen = _concat(ids2, am2, n, cont, clen)
    bars, lg = _bars(m, full, plen, clen)
    want = torch.log_softmax(lg.double(), -1)
    for r in range(2 * n):
        c = int(clen[r])
        assert (a[r, c:] == 0).all() and (b[r, c:] == 0).all()  # a row of length 0 is legal and gives zeros
        assert _rms(a[r, :c], b[r, :c]) <= bars[r], (r, "n per prompt vs the repeated batch")
        ref = want[r, plen[r] - 1:plen[r] - 1 + c].gather(1, cont[r, :c, None])[:, 0]
        assert _rms(a[r, :c], ref) <= bars[r], (r, "vs the forward's log-softmax")
    with pytest.raises(ValueError):
        m.score_continuations(ids2, am2, continuations=cont[:5], num_per_prompt=n)


def test_ignore_tokens_masks_and_is_cleared(tiny):
    cfg, m, ids, am = tiny
    g = torch.Generator().manual_seed(37)
    cont = torch.randint(2, cfg.vocab, (len(LENS), 9), generator=g)
    ign = [int(cont[0, 0]), int(cont[1, 5]), 1]
    plain = m.score_continuations(ids, am, continuations=cont, score_chunk=4).cpu()
    lp, amx = m.score_continuations(ids, am, continuations=cont, score_chunk=4, ignore_tokens=ign, return_argmax=True)
    lp, amx = lp.cpu(), amx.cpu()
    dead = torch.isin(cont, torch.tensor(ign))
    assert dead[0, 0] and dead[1, 5]  # one in a block's first column (slam_token_logprobs), one inside a block (the fused head)
    assert (lp[dead] == float("-inf")).all() and torch.isfinite(lp[~dead]).all()
    assert (lp[~dead] >= plain[~dead] - 1e-5).all()  # mass left the softmax: no log-prob falls
    assert not torch.isin(amx, torch.tensor(ign)).any()
    again = m.score_continuations(ids, am, continuations=cont, score_chunk=4).cpu()
    assert torch.equal(again.view(torch.int32), plain.view(torch.int32))  # the mask was cleared, and the call is reproducible
