"""-m gpu: classifier-free guidance. slam_cfg_scores against the float64 restatement (tests/cfg_ref.py: tolerance 10 x the
float32 restatement's own error, non-finite entries exact, guard words intact), its invariance (a pair alone in a differently
aligned buffer, a second run: the same bits), the degenerate scales, slam_cfg_mirror_tokens; UnitLM.generate(guidance_scale=)
against HuggingFace's own guided greedy `generate` (tests/golden/cfg_hf.npz, make_golden_cfg.py) up to each row's first
near-tie, a guided row alone against the same row in a batch under both samplers, num_return_sequences, prefill_chunk,
return_logprobs against score_continuations, and guidance off."""
import json
import os

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import cfg_ref as R
from tests.gpu_util import lib, ptr, stream, sync
from tests.test_gpu_generate import LOGITS_TOL, _mk, _tiny, _wide
from tests.test_gpu_score_model import _bars, _concat, _rms

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg_hf.npz")
CASES = R.op_cases()
GUARD = 7.0
_tol = []


def cfg_tol() -> float:
    """10 x the float32 restatement's own distance from float64 over the cases: measured on the CPU, never on the kernel."""
    if not _tol:
        _tol.append(10.0 * R.restatement_error(CASES))
    return _tol[0]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cfg(x, g, front=64):
    """slam_cfg_scores through the raw entry point on x [2 B, V]; the scores sit `front` floats into a buffer of guard
    values, with 64 more behind them. Returns (scores [B, V], the whole buffer)."""
    B, V = x.shape[0] // 2, x.shape[1]
    buf = torch.full((front + B * V + 64,), GUARD, dtype=torch.float32, device="cuda")
    scores = buf[front:front + B * V].view(B, V)
    nb = E.cfg_workspace_bytes(B, V)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = lib().slam_cfg_scores(ptr(x), B, V, float(g), ptr(scores), ptr(ws), nb, stream())
    assert rc == 0
    sync()
    return scores, buf


# ---- the op --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cfg_scores_vs_fp64(case):
    name, x_np, g = case
    ref = R.cfg_f64(x_np, g)
    B, V = ref.shape
    x = torch.from_numpy(x_np).cuda()
    raw = _bits(x).clone()
    out, buf = _cfg(x, g)
    assert (buf[:64] == GUARD).all() and (buf[64 + B * V:] == GUARD).all(), "a store outside scores"
    assert torch.equal(_bits(x), raw), "the raw logits were touched"
    got = out.cpu().double().numpy()
    fin = np.isfinite(ref)
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    print(f"[cfg] {name}: max |kernel - fp64| = {err:.3e} (tolerance {cfg_tol():.3e})")
    assert not np.isnan(got).any()
    assert np.array_equal(got[~fin], ref[~fin]), name
    assert err <= cfg_tol(), (name, err, cfg_tol())
    again, _ = _cfg(x, g)
    assert torch.equal(_bits(out), _bits(again)), "not the same bits on a second run"
    for b in range(B):  # the pair alone as B = 1: aligned logits, scores 5 floats into their buffer (4-byte aligned only)
        pair = torch.stack([x[b], x[B + b]]).clone()
        alone, abuf = _cfg(pair, g, front=5)
        assert (abuf[:5] == GUARD).all() and (abuf[5 + V:] == GUARD).all()
        assert torch.equal(_bits(alone[0]), _bits(out[b])), (name, b)


def test_cfg_wrapper_and_degenerate_scales():
    gold = np.load(GOLDEN)
    x = torch.from_numpy(np.concatenate([gold["op_x_2049"], gold["op_y_2049"]])).cuda()
    B, V = 3, 2049
    a = torch.log_softmax(x[:B].double(), -1)
    u = torch.log_softmax(x[B:].double(), -1)
    scores = torch.empty(B, V, dtype=torch.float32, device="cuda")
    ws = torch.empty(E.cfg_workspace_bytes(B, V), dtype=torch.uint8, device="cuda")
    for g, want in ((1.0, a), (0.0, u), (1.5, 1.5 * (a - u) + u)):
        E.cfg_scores(x, g, scores, ws)  # the ctypes wrapper generate uses; g = 1 through it is still the kernel's a_i
        sync()
        err = float((scores.double() - want).abs().max())
        assert err <= cfg_tol(), (g, err, cfg_tol())
        hf = torch.from_numpy(gold[f"op_out_2049_{g}"]).cuda() if g != 1.0 else None
        if hf is not None:  # transformers' own processor on the same rows
            assert float((scores.double() - hf.double()).abs().max()) <= cfg_tol(), g
    with pytest.raises(E.EngineError):
        E.cfg_scores(x, 1.5, x[:B], ws)  # overlapping
    with pytest.raises(ValueError):
        E.cfg_scores(x, 1.5, scores[:2], ws)


@pytest.mark.parametrize("B", [1, 5, 300])
def test_cfg_mirror_tokens(B):
    g = torch.Generator().manual_seed(B)
    buf = torch.randint(-(1 << 40), 1 << 40, (2 * B + 8,), generator=g).cuda()
    before = buf.clone()
    rc = lib().slam_cfg_mirror_tokens(ptr(buf), B, stream())
    assert rc == 0
    sync()
    assert torch.equal(buf[:B], before[:B]) and torch.equal(buf[B:2 * B], before[:B])
    assert torch.equal(buf[2 * B:], before[2 * B:]), "written beyond 2 B"
    nxt = before[:2 * B].clone()
    E.cfg_mirror_tokens(nxt)
    sync()
    assert torch.equal(nxt, buf[:2 * B])


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(tag):
        if tag not in made:
            cfg, sd = _tiny() if tag == "tiny" else _wide()
            made[tag] = (cfg, _mk(cfg, sd, max_tokens=512))
        return made[tag]
    return get


def _golden_kw(gold, k):
    kw = dict(input_ids=torch.from_numpy(gold[f"{k}_ids"]), attention_mask=torch.from_numpy(gold[f"{k}_mask"]),
              guidance_scale=float(gold[f"{k}_g"]), max_new_tokens=int(gold["max_new_tokens"]), eos_token_id=[], pad_token_id=0)
    if f"{k}_neg" in gold:
        kw["negative_prompt_ids"] = torch.from_numpy(gold[f"{k}_neg"])
    if k.endswith("bans"):
        kw.update(bad_words_ids=json.loads(str(gold["bad_words"])), no_repeat_ngram_size=int(gold["no_repeat_ngram_size"]))
    return kw


def _check_trusted(gold, k, out, floor):
    """Steps before a row's first near-tie (HF's own margin below (|g| + |1 - g|) 2 LOGITS_TOL rms) agree exactly; at least
    `floor` of all steps agree from the start."""
    want, margin = torch.from_numpy(gold[f"{k}_seq"]), torch.from_numpy(gold[f"{k}_margin"])
    g = float(gold[f"{k}_g"])
    tol = (abs(g) + abs(1 - g)) * 2 * LOGITS_TOL * float(gold[f"{k}_rms"])
    T = gold[f"{k}_ids"].shape[1]
    assert out.dtype == torch.int64 and out.shape == want.shape, (out.shape, want.shape)
    assert torch.equal(out[:, :T], want[:, :T])  # the prompt exactly as passed, left padding included
    new, wnew = out[:, T:], want[:, T:]
    matched = total = 0
    for b in range(want.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else wnew.shape[1]
        diff = (new[b] != wnew[b]).nonzero()
        first = int(diff[0]) if len(diff) else wnew.shape[1]
        print(f"[cfg generate] {k} row {b}: agrees for {first} steps, trusted {trust} of {wnew.shape[1]}")
        assert first >= trust, (k, b, "diverged at", first, "before the first near-tie", trust)
        matched += first
        total += wnew.shape[1]
    assert matched >= floor * total, (k, matched, total)


@pytest.mark.parametrize("case", ["g15", "g30neg", "g05neg", "g05bans"])
@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_generate_matches_hf_golden(tag, case, gold, models):
    _, m = models(tag)
    k = f"{tag}_{case}"
    out = m.generate(**_golden_kw(gold, k)).cpu()
    _check_trusted(gold, k, out, 0.5)
    if case == "g30neg":  # the engine sampler's greedy pick is the same argmax
        assert torch.equal(m.generate(sampler="engine", **_golden_kw(gold, k)).cpu(), out)


def test_generate_prefill_chunk(gold, models):
    _, m = models("tiny")
    k = "tiny_g30neg"  # prompts up to 70 tokens, negative prompts of 6: chunks of 16 end rows at different blocks
    out = m.generate(prefill_chunk=16, **_golden_kw(gold, k)).cpu()
    _check_trusted(gold, k, out, 0.0)


def _left_padded(cfg, lens, seed):
    g = torch.Generator().manual_seed(seed)
    T = max(lens)
    ids = torch.zeros(len(lens), T, dtype=torch.long)
    am = torch.zeros_like(ids)
    for b, n in enumerate(lens):
        ids[b, T - n:] = torch.randint(2, cfg.vocab, (n,), generator=g)
        am[b, T - n:] = 1
    neg = torch.randint(2, cfg.vocab, (len(lens), 6), generator=g)
    return ids, am, neg


def test_guided_batch_independence_greedy(models):
    cfg, m = models("wide")
    lens = [9, 30, 17]
    ids, am, neg = _left_padded(cfg, lens, 13)
    T = max(lens)
    for extra in (dict(), dict(negative_prompt_ids=neg)):
        kw = dict(guidance_scale=2.0, max_new_tokens=20, eos_token_id=[])
        batch = m.generate(input_ids=ids, attention_mask=am, **kw, **extra).cpu()
        for b, n in enumerate(lens):
            one = {k: v[b:b + 1] for k, v in extra.items()}
            alone = m.generate(input_ids=ids[b:b + 1, T - n:], **kw, **one).cpu()
            assert torch.equal(alone[0, n:], batch[b, T:]), (b, sorted(extra))
    plain = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=20, eos_token_id=[]).cpu()
    assert not torch.equal(plain, batch), "guidance changed nothing: the case checks nothing"


def test_guided_batch_independence_engine_sampler(models):
    cfg, m = models("tiny")
    lens = [16, 11, 5]
    ids, am, neg = _left_padded(cfg, lens, 9)
    sid = torch.tensor([40, 1 << 33, 7])
    kw = dict(guidance_scale=1.5, negative_prompt_ids=neg, do_sample=True, temperature=0.8, top_k=25, max_new_tokens=24,
              eos_token_id=[], seed=11, sampler="engine")
    a = m.generate(input_ids=ids, attention_mask=am, sample_ids=sid, **kw).cpu()
    assert torch.equal(a, m.generate(input_ids=ids, attention_mask=am, sample_ids=sid, **kw).cpu())
    for b, n in enumerate(lens):
        alone = m.generate(input_ids=ids[b:b + 1, 16 - n:], sample_ids=sid[b:b + 1], **dict(kw, negative_prompt_ids=neg[b:b + 1])).cpu()
        assert torch.equal(alone[0, n:], a[b, 16:]), b
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, attention_mask=am, sample_ids=torch.arange(6), **kw)  # only conditional rows are sampled


def test_guided_num_return_sequences(models):
    cfg, m = models("tiny")
    lens = [16, 7]
    ids, am, neg = _left_padded(cfg, lens, 21)
    n = 3
    sid = torch.tensor([5, 77, 2, 1 << 40, 9, 11])
    kw = dict(guidance_scale=1.5, negative_prompt_ids=neg, do_sample=True, temperature=0.8, top_k=25, max_new_tokens=16,
              eos_token_id=[], seed=3, sampler="engine")
    a = m.generate(input_ids=ids, attention_mask=am, num_return_sequences=n, sample_ids=sid, **kw).cpu()
    assert a.shape == (2 * n, 16 + 16) and torch.equal(a[:, :16], ids.repeat_interleave(n, 0))
    for r in range(2 * n):
        b = r // n
        one = m.generate(input_ids=ids[b:b + 1, 16 - lens[b]:], sample_ids=sid[r:r + 1],
                         **dict(kw, negative_prompt_ids=neg[b:b + 1])).cpu()
        assert torch.equal(one[0, lens[b]:], a[r, 16:]), r
    assert not torch.equal(a[0, 16:], a[1, 16:])
    t = m.generate(input_ids=ids, attention_mask=am, num_return_sequences=n, **dict(kw, sampler="torch")).cpu()  # runs
    assert t.shape == a.shape


@pytest.mark.parametrize("sampler", ["engine", "torch"])
def test_guided_logprobs_are_the_models_own(models, sampler):
    cfg, m = models("tiny")
    lens = [37, 20, 5]
    g = torch.Generator().manual_seed(23)
    T = max(lens)
    ids = torch.zeros(len(lens), T, dtype=torch.long)
    am = torch.zeros_like(ids)
    for b, ln in enumerate(lens):  # right-padded, as test_gpu_score_model.py's
        ids[b, :ln] = torch.randint(2, cfg.vocab, (ln,), generator=g)
        am[b, :ln] = 1
    kw = dict(attention_mask=am, guidance_scale=3.0, max_new_tokens=16, pad_token_id=0, eos_token_id=[], return_logprobs=True,
              no_repeat_ngram_size=2)
    if sampler == "engine":
        kw.update(do_sample=True, sampler="engine", temperature=0.8, top_k=25, seed=11)
    out = m.generate(ids, **kw)
    seq, lp = out.sequences.cpu(), out.logprobs.cpu()
    cont = seq[:, T:]
    assert lp.shape == cont.shape and torch.isfinite(lp).all() and (lp <= 0).all()
    got = m.score_continuations(ids, am, continuations=cont).cpu()
    clen = torch.full((len(lens),), cont.shape[1])
    full, _, plen = _concat(ids, am, 1, cont, clen)
    bars, _ = _bars(m, full, plen, clen)
    for r in range(len(lens)):
        d = _rms(got[r], lp[r])
        print(f"[cfg logprobs] {sampler} row {r}: rms diff to score_continuations {d:.3e} (bar {bars[r]:.3e})")
        assert d <= bars[r], (sampler, r, d, bars[r])


@pytest.mark.parametrize("sampler", [None, "engine"])
def test_guidance_off_is_the_plain_call(models, sampler):
    cfg, m = models("tiny")
    ids, am, _ = _left_padded(cfg, [16, 11, 5], 9)
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=16, eos_token_id=[], sampler=sampler, bad_words_ids=[[5], [7, 9]])
    if sampler == "engine":
        kw.update(do_sample=True, temperature=0.8, top_k=25, seed=11)
    plain = m.generate(**kw).cpu()
    assert torch.equal(m.generate(guidance_scale=None, **kw).cpu(), plain)
    assert torch.equal(m.generate(guidance_scale=1.0, **kw).cpu(), plain)
    assert not torch.equal(m.generate(guidance_scale=1.5, **kw).cpu(), plain)
