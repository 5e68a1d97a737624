"""-m gpu: n samples per prompt from one prefill (slam_kv_repeat, generate(num_return_sequences=)) and the log-probability of
every sampled token (slam_token_logprobs, generate(return_logprobs=True)).

The cache fan-out is checked bit for bit against a snapshot taken before it, on a cache poisoned with a bf16 NaN pattern
(the poison is data: nothing is read out of bounds), for the overlapping (B = 3, n = 2; B = 5, n = 2) and the disjoint
(B = 3, n = 5) cases; a decode step behind it against a prefill + decode of the explicitly repeated batch; generate against
generate of the repeated prompts.

The comparisons with the repeated batch use prompt rows of 128 tokens (shorter prompts padded to that stride). The prefill's
attention cuts the flattened [B T] token axis into 128-query / 64-key tiles from token 0, so the bits of a row's K / V depend
on where the row starts modulo the tile: with a stride of 128 row b of the B-row prefill and its copies b n + i of the
B n-row prefill sit at the same offset in their tiles and the results are equal bit for bit. At another stride the two ways
differ by the rounding of a different tile cut - a property of slam_prefill as it stands, not of the fan-out, which is an exact
copy (first test).

Log-prob tolerance: logprob_tol() = 10 x the float32 restatement's own largest error against the float64 reference on the same
inputs (tests/logprob_ref.py: 1.165e-06 measured on the CPU, so 1.165e-05), computed from the restatement when first used and never
from the kernel under test. Non-finite expectations (-inf) must be met exactly."""
import functools

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import logprob_ref as R
from tests.gpu_util import lib, ptr, rel_err, stream, sync
from tests.test_gpu_generate import GOLDEN, LOGITS_TOL, _mk, _tiny, _wide

pytestmark = pytest.mark.gpu

CASES = R.op_cases()


@functools.lru_cache(None)
def logprob_tol() -> float:
    return 10.0 * R.restatement_error(CASES)


POISON = 0x7FC1  # a bf16 NaN
STRIDE = 128     # prompt row stride of the comparisons with the repeated batch (module docstring)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _model(which, max_tokens=1024):
    cfg, sd = _tiny() if which == "tiny" else _wide()
    return cfg, _mk(cfg, sd, max_tokens=max_tokens)


def _prompts(cfg, lens, seed=3, width=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), width or max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(2, cfg.vocab, (n,), generator=g)
    return ids


def _prefilled(m, cfg, ids, lens, rows, cap):
    """A poisoned cache of `rows` rows bound to the engine and prefilled with the len(lens) prompts. Returns the cache as
    int16 [L, 2, rows, nKV, cap, hd], lens int32 [rows] and logits fp32 [rows, V] with their first B entries filled."""
    dev = m.device
    B, T = ids.shape
    nb = m.engine.kv_cache_bytes(rows, cap)
    cache = torch.full((nb // 2,), POISON, dtype=torch.int16, device=dev)
    m.engine.bind_kv_cache(cache, rows, cap)
    lens_d = torch.zeros(rows, dtype=torch.int32, device=dev)
    lens_d[:B] = torch.tensor(lens, dtype=torch.int32)
    logits = torch.full((rows, cfg.vocab), float("nan"), dtype=torch.float32, device=dev)
    m.engine.prefill(ids.to(dev).contiguous(), lens_d, B, T, logits)
    return cache.view(cfg.n_layers, 2, rows, cfg.n_kv_heads, cap, cfg.head_dim), lens_d, logits


@pytest.mark.parametrize("which", ["tiny", "wide"])
@pytest.mark.parametrize("lens,ns", [((1, 37, 70), (1, 2, 5)), ((1, 37, 70, 12, 64), (2,))], ids=["B3", "B5"])
def test_kv_repeat_copies_exactly(which, lens, ns):
    cfg, m = _model(which)
    ids = _prompts(cfg, lens)
    B = len(lens)
    for n in ns:
        rows = B * n + 1  # one row more than needed: it must keep its poison
        kv, lens_d, logits = _prefilled(m, cfg, ids, lens, rows, 128)
        kv0, lens0, logits0 = kv.clone(), lens_d.clone(), logits.clone()
        assert (kv0[:, :, B:] == POISON).all()
        m.engine.kv_repeat(n, lens_d, logits)
        sync()
        if n == 1:
            assert torch.equal(kv, kv0) and torch.equal(lens_d, lens0) and torch.equal(_bits(logits), _bits(logits0))
            continue
        for b, ln in enumerate(lens):
            for i in range(n):
                r = b * n + i
                assert torch.equal(kv[:, :, r, :, :ln], kv0[:, :, b, :, :ln]), (which, n, b, i)
                assert int(lens_d[r]) == ln, (which, n, b, i)
                assert torch.equal(_bits(logits[r]), _bits(logits0[b])), (which, n, b, i)
        assert (kv[:, :, B * n] == POISON).all() and int(lens_d[B * n]) == 0
        assert torch.isnan(logits[B * n]).all()
        assert not torch.isnan(logits[:B * n]).any()


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_decode_behind_kv_repeat(which):
    cfg, m = _model(which)
    lens, n = (1, 37, 70), 2
    B, BN = len(lens), len(lens) * n
    ids = _prompts(cfg, lens, seed=4, width=STRIDE)
    dev = m.device
    tok = torch.arange(5, 5 + BN, dtype=torch.int64, device=dev)  # a different token in every row
    _, lens_d, logits = _prefilled(m, cfg, ids, lens, BN, STRIDE + 64)
    h = m.engine.h
    assert lib().slam_kv_repeat(h, 4, ptr(lens_d), ptr(logits), stream()) == -1  # B n above max_batch: EINVAL
    m.engine.kv_repeat(n, lens_d, logits)
    m.engine.decode_step(tok, lens_d, BN, logits)
    sync()
    got = logits.clone()
    assert lens_d.tolist() == [ln + 1 for ln in lens for _ in range(n)]
    assert lib().slam_kv_repeat(h, 1, ptr(lens_d), ptr(logits), stream()) == -2  # after a decode step: ESTATE
    with pytest.raises(E.EngineError):
        m.engine.kv_repeat(n, lens_d, logits)
    # the explicitly repeated batch through prefill + decode
    rep_lens = [ln for ln in lens for _ in range(n)]
    _, lens_r, logits_r = _prefilled(m, cfg, ids.repeat_interleave(n, 0), rep_lens, BN, STRIDE + 64)
    m.engine.decode_step(tok, lens_r, BN, logits_r)
    sync()
    assert not torch.isnan(got).any()  # the unspecified (poisoned) keys behind lens[b] are never read
    assert torch.equal(_bits(got), _bits(logits_r)), which


def test_decode_behind_kv_repeat_at_another_stride():
    """Prompt rows of 70 tokens: the rows of the B-row and of the B n-row prefill start at different offsets in the prefill's
    attention tiles, so the two ways are not held to equal bits; their decode logits agree within the model tolerance of
    test_gpu_generate.py (rel-RMS 2e-2, the bound the decode path is held to against the full forward)."""
    cfg, m = _model("tiny")
    lens, n = (1, 37, 70), 2
    BN = len(lens) * n
    ids = _prompts(cfg, lens, seed=4)
    tok = torch.arange(5, 5 + BN, dtype=torch.int64, device=m.device)
    _, lens_d, logits = _prefilled(m, cfg, ids, lens, BN, 128)
    m.engine.kv_repeat(n, lens_d, logits)
    m.engine.decode_step(tok, lens_d, BN, logits)
    sync()
    got = logits.clone()
    _, lens_r, logits_r = _prefilled(m, cfg, ids.repeat_interleave(n, 0), [ln for ln in lens for _ in range(n)], BN, 128)
    m.engine.decode_step(tok, lens_r, BN, logits_r)
    sync()
    assert not torch.isnan(got).any()
    for r in range(BN):
        e = rel_err(got[r], logits_r[r])
        assert e <= LOGITS_TOL, (r, e)


def test_kv_repeat_twice():
    """A second fan-out before any decode step: B -> B n -> B n m rows, row b of the prefill in rows b n m .. b n m + n m - 1."""
    cfg, m = _model("tiny")
    lens, n, mm = (5, 40), 2, 3
    B, rows = len(lens), len(lens) * n * mm
    kv, lens_d, logits = _prefilled(m, cfg, _prompts(cfg, lens, seed=6), lens, rows, 64)
    kv0, logits0 = kv.clone(), logits.clone()
    m.engine.kv_repeat(n, lens_d, logits)
    m.engine.kv_repeat(mm, lens_d, logits)
    sync()
    for r in range(rows):
        b = r // (n * mm)
        assert torch.equal(kv[:, :, r, :, :lens[b]], kv0[:, :, b, :, :lens[b]]), r
        assert int(lens_d[r]) == lens[b] and torch.equal(_bits(logits[r]), _bits(logits0[b])), r
    m.engine.decode_step(torch.arange(2, 2 + rows, dtype=torch.int64, device=m.device), lens_d, rows, logits)
    sync()
    assert not torch.isnan(logits).any()


def _left_padded(cfg, seed=9):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, cfg.vocab, (4, STRIDE), generator=g)  # the longest prompt fills the stride
    am = torch.ones_like(ids)
    am[1, :5] = 0
    am[2, :58] = 0
    am[3, :STRIDE - 5] = 0
    return ids, am


@pytest.fixture(scope="module")
def tiny():
    cfg, m = _model("tiny", max_tokens=512)
    ids, am = _left_padded(cfg)
    first = m(input_ids=ids[:1]).logits[0, -1].float()
    bad = [[int(t)] for t in first.topk(3).indices]
    kw = dict(attention_mask=am, bad_words_ids=bad, do_sample=True, temperature=0.8, top_k=25, top_p=0.95, max_new_tokens=24,
              pad_token_id=0, seed=11)
    return cfg, m, ids, am, kw


def _with_eos(m, ids, kw, sampler, n):
    """kw + this sampler + EOS ids that some rows emit early and others late or never: the tokens that two rows of the same
    seeded call without an EOS produce at steps 2 and 5 (the call with the EOS repeats those draws up to each row's EOS)."""
    kw = dict(kw, sampler=sampler)
    free = m.generate(ids, eos_token_id=[], num_return_sequences=n, **kw).cpu()
    return dict(kw, eos_token_id=sorted({int(free[1, STRIDE + 2]), int(free[-1, STRIDE + 5])}))


@pytest.mark.parametrize("sampler", ["engine", "torch"])
def test_generate_n_equals_repeated_prompts(tiny, sampler):
    cfg, m, ids, am, kw = tiny
    n = 3
    kw = _with_eos(m, ids, kw, sampler, n)
    rep = dict(kw, attention_mask=am.repeat_interleave(n, 0))
    a = m.generate(ids, num_return_sequences=n, **kw)
    b = m.generate(ids.repeat_interleave(n, 0), **rep)
    assert isinstance(a, torch.Tensor) and a.dtype == torch.int64
    a, b = a.cpu(), b.cpu()
    assert a.shape[0] == 4 * n and torch.equal(a, b)
    assert torch.equal(a[:, :STRIDE], ids.repeat_interleave(n, 0))  # the prompt part as passed, HF's row order
    new = a[:, STRIDE:]
    eos = torch.tensor(kw["eos_token_id"])
    hit = torch.isin(new, eos)
    assert hit.any(1).any() and hit[:, :8].any(), "no row met an EOS early: the case checks nothing"
    for r in range(4 * n):
        if hit[r].any():
            k = int(hit[r].nonzero()[0])
            assert (new[r, k + 1:] == 0).all()
    assert not torch.isin(new, torch.tensor([w[0] for w in kw["bad_words_ids"]])).any()
    for p in range(4):
        rows = new[p * n:(p + 1) * n]
        assert not all(torch.equal(rows[0], rows[i]) for i in range(1, n)), p
    if sampler == "engine":
        sid = torch.tensor([40, 7, 19, 3, 1000003, 5, 77, 2, 9, 11, 1 << 40, 6])
        a2 = m.generate(ids, num_return_sequences=n, sample_ids=sid, **kw).cpu()
        b2 = m.generate(ids.repeat_interleave(n, 0), sample_ids=sid, **rep).cpu()
        assert torch.equal(a2, b2) and not torch.equal(a2, a)


def test_generate_n_refusals(tiny):
    cfg, m, ids, am, kw = tiny
    with pytest.raises(ValueError):
        m.generate(ids, attention_mask=am, max_new_tokens=4, num_return_sequences=2)  # greedy
    with pytest.raises(ValueError):
        m.generate(ids, num_return_sequences=2, sampler="engine", sample_ids=torch.arange(4), **kw)
    with pytest.raises(ValueError):
        m.generate(ids, num_return_sequences=0, **kw)


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_existing_generation_unchanged(tag):
    gold = dict(np.load(GOLDEN))
    cfg, m = _model(tag, max_tokens=512)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    want = torch.from_numpy(gold[f"{tag}_seq"])
    margin = torch.from_numpy(gold[f"{tag}_margin"])
    kw = dict(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(),
              max_new_tokens=int(gold["max_new_tokens"]), eos_token_id=int(gold[f"{tag}_eos"]), pad_token_id=0)
    out = m.generate(num_return_sequences=1, **kw)
    assert isinstance(out, torch.Tensor) and not isinstance(out, tuple)
    out = out.cpu()
    assert torch.equal(out, m.generate(**kw).cpu())
    assert out.dtype == torch.int64 and out.shape == want.shape
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids)
    tol = 2 * LOGITS_TOL * float(gold[f"{tag}_score_rms"])
    for b in range(want.shape[0]):  # the existing criterion: exact up to the row's first near-tie step
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else want.shape[1] - T
        diff = (out[b, T:] != want[b, T:]).nonzero()
        first = int(diff[0]) if len(diff) else want.shape[1] - T
        assert first >= trust, (tag, b, first, trust)


# ---- log-probabilities: the op ----------------------------------------------------------------------------------------------
def _logprobs(x, tok, done=None, finished=None, column=0, width=1):
    B, V = x.shape
    out = torch.full((B, width), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(E.token_logprobs_workspace_bytes(B, V), dtype=torch.uint8, device="cuda")
    E.token_logprobs(x, tok, out, column, ws, done, finished)
    sync()
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_token_logprobs_vs_fp64(case):
    name, x_np, tok_np = case
    ref = R.logprob_f64(x_np, tok_np)
    x = torch.from_numpy(x_np).cuda()
    tok = torch.from_numpy(tok_np).cuda()
    out = _logprobs(x, tok, column=1, width=3)
    assert (out[:, 0] == 7.0).all() and (out[:, 2] == 7.0).all()  # only the column asked for
    got = out[:, 1].cpu().double().numpy()
    fin = np.isfinite(ref)
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    print(f"[logprob] {name}: max |kernel - fp64| = {err:.3e} (tolerance {logprob_tol():.3e})")
    assert np.array_equal(got[~fin], ref[~fin]), (name, got, ref)
    assert err <= logprob_tol(), (name, err, logprob_tol())
    again = _logprobs(x, tok, column=1, width=3)
    assert torch.equal(_bits(out), _bits(again)), "not the same bits on a second run"
    for b in range(x.shape[0]):  # the row alone, at the start of its own (aligned) buffer
        alone = _logprobs(x[b:b + 1].clone(), tok[b:b + 1].clone())
        assert torch.equal(_bits(alone[0, 0]), _bits(out[b, 1])), (name, b)


def test_token_logprobs_finished_protocol():
    x_np = CASES[0][1].copy()
    x_np[2, x_np.shape[1] // 3] = 1.0  # no +inf here: every row's value is an ordinary number
    x = torch.from_numpy(x_np).cuda()
    tok = torch.tensor([4, 9, 17], dtype=torch.int64, device="cuda")
    want = torch.from_numpy(R.logprob_f64(x_np, tok.cpu().numpy()))
    fin = torch.zeros(3, dtype=torch.uint8, device="cuda")
    out = torch.full((3, 3), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(E.token_logprobs_workspace_bytes(3, x.shape[1]), dtype=torch.uint8, device="cuda")
    dones = ([0, 1, 0], [0, 1, 1], [0, 1, 1])
    for k, d in enumerate(dones):
        E.token_logprobs(x, tok, out, k, ws, torch.tensor(d, dtype=torch.uint8, device="cuda"), fin)
        sync()
        assert fin.tolist() == d
    out = out.cpu().double()
    # [row, call]: row 0 never finishes; row 1 is done at call 0 and row 2 at call 1, and that EOS step itself has its value
    live = torch.tensor([[1, 1, 1], [1, 0, 0], [1, 1, 0]], dtype=torch.bool)
    assert (out[~live] == 0.0).all()
    assert ((out - want[:, None]).abs()[live] <= logprob_tol()).all()
    # without `done` the flags are cleared; without `finished` nothing is skipped
    last = torch.zeros(3, 1, device="cuda")
    E.token_logprobs(x, tok, last, 0, ws, None, fin)
    sync()
    assert fin.tolist() == [0, 0, 0] and float(last[0, 0]) != 0.0 and float(last[1, 0]) == 0.0


def test_token_logprobs_behind_the_sampler_with_pad_equal_eos():
    V, eos = 502, 3
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(3, V, generator=g) * 3).cuda()
    x[1, eos] = 50.0  # greedy picks the EOS id in row 1; pad_id is that id too
    desc = E.SlamSampleDesc(do_sample=0, top_k=1, temperature=1.0, top_p=1.0, seed=0, step=0, pad_id=eos, n_eos=1)
    eos_i = torch.tensor([eos], dtype=torch.int32, device="cuda")
    done = torch.zeros(3, dtype=torch.uint8, device="cuda")
    fin = torch.zeros(3, dtype=torch.uint8, device="cuda")
    nxt = torch.empty(3, dtype=torch.int64, device="cuda")
    new = torch.empty(3, 3, dtype=torch.int64, device="cuda")
    lp = torch.full((3, 3), 7.0, dtype=torch.float32, device="cuda")
    sws = torch.empty(E.sample_workspace_bytes(3, V, 1), dtype=torch.uint8, device="cuda")
    ws = torch.empty(E.token_logprobs_workspace_bytes(3, V), dtype=torch.uint8, device="cuda")
    for k in range(3):  # sampler and log-prob back to back on one stream, nothing in between
        desc.step = k
        E.sample_tokens(x, desc, nxt, sws, None, None, eos_i, done, new)
        E.token_logprobs(x, nxt, lp, k, ws, done, fin)
    sync()
    assert new[1].tolist() == [eos, eos, eos] and done.tolist() == [0, 1, 0] and fin.tolist() == [0, 1, 0]
    want = torch.log_softmax(x.double(), -1).gather(1, new[:, :1]).cpu()[:, 0]
    lp = lp.cpu().double()
    assert abs(float(lp[1, 0]) - float(want[1])) <= logprob_tol() and lp[1, 1:].tolist() == [0.0, 0.0]
    for b in (0, 2):  # rows that never finish keep getting values
        assert ((lp[b] - want[b]).abs() <= logprob_tol()).all() and (lp[b] != 0).all()


# ---- log-probabilities: end to end ----------------------------------------------------------------------------------------------
def _replay_logprobs(m, cfg, ids, am, seq, n):
    """Teacher-forced: the prompts prefilled and fanned out as generate does it, then the returned tokens fed back one
    step at a time; torch's fp32 log_softmax of every step's logits at the returned token. [B n, new]."""
    dev = m.device
    B, T_in = ids.shape
    BN, new = B * n, seq.shape[1] - T_in
    lens = am.sum(1).tolist()
    T = max(lens)
    comp = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        comp[b, :lens[b]] = ids[b][am[b].bool()]
    _, lens_d, logits = _prefilled(m, cfg, comp, lens, BN, -(-(T + new) // 64) * 64)
    m.engine.kv_repeat(n, lens_d, logits)
    toks = seq[:, T_in:].to(dev)
    cols = []
    for k in range(new):
        cols.append(torch.log_softmax(logits, -1).gather(1, toks[:, k:k + 1]))
        if k + 1 < new:
            m.engine.decode_step(toks[:, k].contiguous(), lens_d, BN, logits)
    sync()
    return torch.cat(cols, 1).cpu()


@pytest.mark.parametrize("sampler", ["engine", "torch"])
def test_generate_logprobs_end_to_end(tiny, sampler):
    cfg, m, ids, am, kw = tiny
    n = 2
    kw = _with_eos(m, ids, kw, sampler, n)
    out = m.generate(ids, num_return_sequences=n, return_logprobs=True, **kw)
    assert isinstance(out, tuple) and out._fields == ("sequences", "logprobs")
    seq, lp = out.sequences.cpu(), out.logprobs.cpu()
    assert torch.equal(seq, m.generate(ids, num_return_sequences=n, **kw).cpu())  # asking for them changes no token
    new = seq[:, STRIDE:]
    assert lp.dtype == torch.float32 and lp.shape == new.shape and new.shape[0] == 4 * n  # trimmed together
    want = _replay_logprobs(m, cfg, ids, am, seq, n)
    hit = torch.isin(new, torch.tensor(kw["eos_token_id"]))
    after = (hit.cumsum(1) - hit.long()) > 0  # strictly behind the row's first EOS
    assert after.any(), "no row finished early: the zeros are not checked"
    assert (lp[after] == 0.0).all()
    err = float((lp.double() - want.double()).abs()[~after].max())
    print(f"[logprob] generate({sampler}): max |returned - replayed log_softmax| = {err:.3e} (tolerance {logprob_tol():.3e})")
    assert (lp[~after] < 0).all() and err <= logprob_tol(), err
