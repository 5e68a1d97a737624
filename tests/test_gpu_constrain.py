"""-m gpu: slam_constrain_scores (per-row bans from the row's own history) against tests/constrain_ref.py, which
tests/test_constrain_host.py holds to transformers' own processors, and generate's no_repeat_ngram_size, multi-token
bad_words_ids, min_new_tokens / min_length, begin_suppress_tokens and suppress_tokens under both samplers.

Kernel comparisons are exact: the whole scores array is compared as int32 bit patterns, which checks the -inf set and every
copied element (NaN and +-inf included) at once."""
import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import constrain_ref as R
from tests.gpu_util import sync
from tests.test_gpu_generate import _mk, _tiny
from tests.test_gpu_score_model import _bars, _concat, _rms

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel floats on both sides of the scores buffer: nothing may be written outside [B][V]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda") if len(v) else None


def _launch(logits, prompt, plen, new, step, n=0, npp=1, done=None, seqs=(), ban_eos=False, eos=(), begin=(), mode="out"):
    """One slam_constrain_scores call on fresh device copies. mode: "in" (scores is logits), "out" (a buffer of its own),
    "skew" (a buffer 4 bytes off the logits' 16-byte phase: the 4-byte copy path). Returns the scores as a CPU tensor."""
    B, V = logits.shape
    lg = torch.from_numpy(logits).cuda()
    if mode == "in":
        buf = None
        sc = lg
    else:
        skew = 1 if mode == "skew" else 0
        buf = torch.full((GUARD + skew + B * V + GUARD,), 7.25, dtype=torch.float32, device="cuda")
        sc = buf[GUARD + skew:GUARD + skew + B * V].view(B, V)
        if mode == "skew":
            assert (sc.data_ptr() - lg.data_ptr()) % 16 != 0
    off = [0]
    for w in seqs:
        off.append(off[-1] + len(w))
    desc = E.SlamConstrainDesc(step=step, no_repeat_ngram=n, n_per_prompt=npp, prompt_stride=0, ban_eos=int(ban_eos),
                               n_eos=len(eos), n_begin=len(begin), n_seqs=len(seqs), n_seq_tokens=off[-1])
    E.constrain_scores(lg, sc, desc, torch.from_numpy(prompt).cuda(), torch.from_numpy(plen).cuda(),
                       torch.from_numpy(new).cuda() if new is not None else None,
                       torch.from_numpy(done).cuda() if done is not None else None, _i32(list(eos)), _i32(list(begin)),
                       _i32([t for w in seqs for t in w]), _i32(off) if len(seqs) else None)
    sync()
    if buf is not None:
        assert bool((buf[:GUARD + (mode == "skew")] == 7.25).all()) and bool((buf[-GUARD:] == 7.25).all()), "wrote outside scores"
        assert np.array_equal(lg.cpu().numpy().view(np.int32), logits.view(np.int32)), "out of place must leave the logits alone"
    return sc.cpu().clone()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def _logits(rng, B, V, special):
    x = (3 * rng.standard_normal((B, V))).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(flat.size // 50, 6))
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), idx.size)
    for b in range(B):  # and at ids the histories hold, so that a ban lands on them and a copy has to keep them
        for t in special:
            if rng.random() < 0.3:
                x[b, t] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32))
    return x


def _alphabet(V):
    """Chunk edges (0, 2047, 2048, V - 1), two ordinary ids, one id >= V and one negative id (they ban nothing)."""
    ids = [0, 2047, 2048, V - 1, 1, min(5, V - 1), V + 3, -7]
    return np.array(ids, np.int64), [t for t in ids if 0 <= t < V]


def _histories(rng, alpha, lengths):
    p = np.array([0.28, 0.2, 0.2, 0.12, 0.06, 0.06, 0.04, 0.04])
    return [alpha[rng.choice(len(alpha), L, p=p)].tolist() for L in lengths]


def _pack(hists, step, npp, stride_new):
    """prompt [Bp][Tp] (right-padded with an id that would ban something if it were read), prompt_len, new [B][stride]. Rows
    of one prompt share its tokens: the prompt part is taken from the group's first row."""
    B = len(hists)
    Bp = B // npp
    plen = np.array([len(hists[g * npp]) - step for g in range(Bp)], np.int32)
    Tp = max(int(plen.max()), 1) + 3
    prompt = np.full((Bp, Tp), 1, np.int64)
    new = np.full((B, stride_new), 1, np.int64)
    for b in range(B):
        g = b // npp
        hists[b][:plen[g]] = hists[g * npp][:plen[g]]
        prompt[g, :plen[g]] = hists[b][:plen[g]]
        new[b, :step] = hists[b][plen[g]:]
    return prompt, plen, new


@pytest.mark.parametrize("V,B,npp", [(502, 5, 1), (2048, 1, 1), (2049, 3, 1), (2049, 3, 3), (152167, 2, 1), (502, 6, 3)])
def test_kernel_equals_ref(V, B, npp):
    rng = np.random.default_rng(V * 31 + B * 7 + npp)
    alpha, special = _alphabet(V)
    launches = 0
    for n in (0, 1, 2, 3, 5):
        targets = [0, max(n - 2, 0), max(n - 1, 0), n, 7, 300, 2100]
        for step in (0, 1, 6):
            for r0 in range(0, len(targets), max(B // npp, 1)):
                # history lengths mixed within the batch; a row cannot be shorter than the new tokens it already has
                lens = [max(targets[(r0 + b // npp) % len(targets)], step) for b in range(B)]
                hists = _histories(rng, alpha, lens)
                prompt, plen, new = _pack(hists, step, npp, 9)
                x = _logits(rng, B, V, special)
                done = (rng.random(B) < 0.3).astype(np.uint8) if B > 1 else np.array([launches % 4 == 3], np.uint8)
                sets, want = R.constrain(x, hists, step, n=n, done=done)
                for mode in ("in", "out", "skew"):
                    got = _launch(x, prompt, plen, new, step, n=n, npp=npp, done=done, mode=mode).numpy()
                    assert _same_bits(got, want), (V, B, npp, n, step, lens, mode, done.tolist(),
                                                   [sorted(s) for s in sets], np.argwhere(got.view(np.int32) != want.view(np.int32))[:8])
                    again = _launch(x, prompt, plen, new, step, n=n, npp=npp, done=done, mode=mode).numpy()
                    assert _same_bits(got, again), "two runs differ"
                    launches += 2
                for b in range(B):  # the comparison is not of empty sets: a long live row over eight symbols bans something
                    if not done[b] and lens[b] >= 300 and 0 < n <= 2:
                        assert sets[b], (n, step, b, lens[b])
    print(f"[constrain] V {V} B {B} n_per_prompt {npp}: {launches} launches equal to the restatement")


def test_row_alone_equals_row_in_batch():
    V, n, step = 2049, 3, 4
    rng = np.random.default_rng(5)
    alpha, special = _alphabet(V)
    hists = _histories(rng, alpha, [40, 300, 9, 2100, 5])
    x = _logits(rng, 5, V, special)
    prompt, plen, new = _pack(hists, step, 1, 8)
    batch = _launch(x, prompt, plen, new, step, n=n, mode="out").numpy()
    sets, want = R.constrain(x, hists, step, n=n)
    assert _same_bits(batch, want) and sum(len(s) > 0 for s in sets) >= 2
    for b in range(5):
        p1, l1, n1 = _pack([list(hists[b])], step, 1, 8)
        alone = _launch(x[b:b + 1].copy(), p1, l1, n1, step, n=n, mode="out").numpy()
        assert _same_bits(alone[0], batch[b]), b


@pytest.mark.parametrize("V", [502, 2049])
def test_sequences_eos_and_begin(V):
    rng = np.random.default_rng(V)
    last = V - 1
    # row 0: prompt (3 tokens) ends in the prefix of [4, 9 -> 11] only together with new tokens (spanning prompt and new)
    # row 1: a prefix that matches at the very end of the PROMPT is stale once new tokens exist; matches [2, 3 -> last]
    # row 2: history shorter than the longest entries, exactly as long as [3 -> 0]; row 3: done
    hists = [[7, 8, 4, 9], [5, 6, 2, 3], [1, 3], [0, 4, 4, 9]]
    step = 1
    seqs = [[4, 9, 11], [9, 12], [2, 3, last], [6, 2, 13], [3, 0], [3, V + 4], [8, 4, 9, 14], [7, 8, 4, 9, 15], [3, -2],
            [20, 21]]
    assert len(seqs[7]) == len(hists[0]) + 1  # Lh + 1 tokens: ignored although its prefix is the whole history
    prompt, plen, new = _pack(hists, step, 1, 4)
    x = _logits(rng, 4, V, [0, 11, 12, last])
    done = np.array([0, 0, 0, 1], np.uint8)
    for n_eos in (1, 3, 16):
        eos = [last, 0, V + 1, -1][:n_eos] + list(range(30, 30 + max(n_eos - 4, 0)))
        for ban_eos in (False, True):
            for st, begin in ((1, [17, last]), (0, [17, last, V, -3])):
                h = [r[:len(r) - step + st] for r in hists]  # step 0: the prompts alone
                sets, want = R.constrain(x, h, st, n=2, seqs=seqs, ban_eos=ban_eos, eos_ids=eos, begin_ids=begin, done=done)
                for mode in ("in", "out"):
                    got = _launch(x, prompt, plen, new, st, n=2, done=done, seqs=seqs, ban_eos=ban_eos, eos=eos, begin=begin,
                                  mode=mode).numpy()
                    assert _same_bits(got, want), (V, n_eos, ban_eos, st, mode, [sorted(s) for s in sets])
                if st == 1:
                    assert {11, 12, 14} <= sets[0] and 15 not in sets[0] and last in sets[1] and 13 not in sets[1]
                    assert 0 in sets[2] and sets[3] == set()
                    assert (17 in sets[0]) is False and ((last in sets[0]) == ban_eos)
                else:
                    assert {17, last} <= sets[0] and 11 not in sets[0]


# ---- generate ----------------------------------------------------------------------------------------------------------------
T_IN, NEW = 12, 60
PROMPT_SEED = 5


@pytest.fixture(scope="module")
def tiny():
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=512)
    g = torch.Generator().manual_seed(PROMPT_SEED)
    ids = torch.randint(2, cfg.vocab, (3, T_IN), generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0  # left padding: not part of the history
    free = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=NEW, eos_token_id=[]).cpu()
    return cfg, m, ids, am, free


def _real(ids, am, new_row, b):
    return ids[b][am[b].bool()].tolist() + [int(t) for t in new_row]


def _check_no_repeat(ids, am, free_new, got_new, n, npp=1, greedy=True):
    """Every row: no n-gram of its real tokens twice, and equal to the unconstrained row up to the first step at which the
    restatement bans the unconstrained choice (greedy: a ban elsewhere cannot move the argmax). Sampling draws the same
    uniform at every (row, step) in both runs, but any ban changes the candidates' weights, so there the rows are equal up to
    the first step at which the restatement bans anything at all."""
    for r in range(got_new.shape[0]):
        b = r // npp
        assert not R.has_repeated_ngram(_real(ids, am, got_new[r], b), n), (r, "an n-gram occurs twice")
        first = NEW
        for s in range(NEW):
            bans = R.ngram_bans(_real(ids, am, free_new[r, :s], b), n)
            if (int(free_new[r, s]) in bans) if greedy else bool(bans):
                first = s
                break
        assert torch.equal(got_new[r, :first], free_new[r, :first]), (r, first)
        if greedy and first < NEW:
            assert int(got_new[r, first]) != int(free_new[r, first]), (r, first)
    return first


def test_generate_no_repeat_ngram(tiny):
    cfg, m, ids, am, free = tiny
    free_new = free[:, T_IN:]
    # (a) the precondition: unconstrained greedy decoding loops
    assert any(R.has_repeated_ngram(_real(ids, am, free_new[b], b), 3) for b in range(3)), \
        "the unconstrained output holds no repeated 3-gram any more: pick another PROMPT_SEED"
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=NEW, eos_token_id=[])
    # (b) + (c)
    out_t = m.generate(no_repeat_ngram_size=3, **kw).cpu()
    out_e = m.generate(no_repeat_ngram_size=3, sampler="engine", **kw).cpu()
    assert torch.equal(out_t[:, :T_IN], ids) and out_t.shape == (3, T_IN + NEW)
    _check_no_repeat(ids, am, free_new, out_t[:, T_IN:], 3)
    assert torch.equal(out_t, out_e), "the two samplers disagree"
    assert not torch.equal(out_t, free)
    # (d) the log-probs are the raw logits': equal to a teacher-forced scoring of the same tokens
    for sampler in (None, "engine"):
        o = m.generate(no_repeat_ngram_size=3, sampler=sampler, return_logprobs=True, **kw)
        assert torch.equal(o.sequences.cpu(), out_t), sampler
        lp = o.logprobs.cpu()
        cont = out_t[:, T_IN:]
        clen = torch.full((3,), NEW)
        assert torch.isfinite(lp).all() and (lp <= 0).all(), "a banned score leaked into the log-probs"
        got = m.score_continuations(ids, am, continuations=cont).cpu()
        full, lab, plen = _concat(ids, am, 1, cont, clen)
        bars, _ = _bars(m, full, plen, clen)
        for r in range(3):
            d = _rms(got[r], lp[r])
            print(f"[constrain] sampler {sampler} row {r}: rms diff of generate's log-probs to score_continuations {d:.3e} (bar {bars[r]:.3e})")
            assert d <= bars[r], (sampler, r, d, bars[r])
    # (e) every option at its off value: the bits of a call without them
    for sampler in (None, "engine"):
        off = m.generate(no_repeat_ngram_size=0, min_new_tokens=0, min_length=0, begin_suppress_tokens=[], suppress_tokens=[],
                         bad_words_ids=[], sampler=sampler, return_logprobs=True, **kw)
        plain = m.generate(sampler=sampler, return_logprobs=True, **kw)
        assert torch.equal(off.sequences, plain.sequences) and torch.equal(plain.sequences.cpu(), free)
        assert torch.equal(off.logprobs.view(torch.int32), plain.logprobs.view(torch.int32))


@pytest.mark.parametrize("sampler", [None, "engine"])
def test_generate_min_new_tokens_and_min_length(tiny, sampler):
    cfg, m, ids, am, free = tiny
    eos = sorted({int(free[b, T_IN + 1]) for b in range(3)} | {int(free[b, T_IN]) for b in range(3)})
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=30, eos_token_id=eos, pad_token_id=0, sampler=sampler)
    et = torch.tensor(eos)
    plain = m.generate(**kw).cpu()[:, T_IN:]
    assert plain.shape[1] <= 2 and torch.isin(plain, et).any(1).all(), "without the option every row ends by step 1"
    for opt in (dict(min_new_tokens=5), dict(min_length=T_IN + 5)):
        new = m.generate(**opt, **kw).cpu()[:, T_IN:]
        assert new.shape[1] >= 5 and not torch.isin(new[:, :4], et).any(), (opt, new)
        if new.shape[1] < 30:  # generation still ends: every row holds an EOS, pads behind it
            assert torch.isin(new, et).any(1).all()
        for b in range(3):
            hit = torch.isin(new[b], et).nonzero()
            if len(hit):
                assert (new[b, int(hit[0]) + 1:] == 0).all()
    # generation still ends, at a step this test fixes: only token 1 (in no prompt) and 16 EOS ids are left unsuppressed, so
    # five 1s are forced; the six-token bad word then bans the sixth 1 and every row must take an EOS id at the sixth token
    every = list(range(2, 18))
    out = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=30, eos_token_id=every, pad_token_id=0, sampler=sampler,
                     min_new_tokens=5, suppress_tokens=[0] + list(range(18, cfg.vocab)), bad_words_ids=[[1] * 6]).cpu()[:, T_IN:]
    assert out.shape[1] == 6 and (out[:, :5] == 1).all() and torch.isin(out[:, 5], torch.tensor(every)).all(), out


@pytest.mark.parametrize("sampler", [None, "engine"])
def test_generate_multi_token_bad_word(tiny, sampler):
    """Ban the bigram at new positions (3, 4) of a baseline: the output agrees through position 3, differs at 4 and never holds
    the bigram. The tiny model's free greedy output repeats one token, so its (3, 4) bigram already stands at (0, 1); the
    baseline in which (3, 4) is the bigram's FIRST occurrence is the one under no_repeat_ngram_size=2 (all bigrams distinct),
    and the bad word is the only thing added to it. The free baseline is checked too, at the bigram's first occurrence."""
    cfg, m, ids, am, free = tiny
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], sampler=sampler)
    for extra in (dict(no_repeat_ngram_size=2), dict()):
        base = m.generate(**extra, **kw).cpu()[:, T_IN:] if extra else free[:, T_IN:]
        bigram = [int(base[0, 3]), int(base[0, 4])]
        real0 = _real(ids, am, base[0], 0)
        p0 = int(am[0].sum())
        at = next(j for j in range(p0, len(real0)) if real0[j - 1:j + 1] == bigram) - p0  # new position of its second token
        if extra:
            assert at == 4, "under no_repeat_ngram_size=2 the bigram at (3, 4) cannot have occurred before"
        out = m.generate(bad_words_ids=[bigram], **extra, **kw).cpu()[:, T_IN:]
        assert torch.equal(out[0, :at], base[0, :at]) and int(out[0, at]) != bigram[1], (extra, at)
        for b in range(3):
            row = _real(ids, am, out[b], b)
            assert all(row[j:j + 2] != bigram for j in range(int(am[b].sum()) - 1, len(row) - 1)), (b, "the bigram was emitted")
    free_new = free[:, T_IN:]
    # begin_suppress_tokens: the unconstrained first token is banned at step 0 only
    first = [int(free_new[b, 0]) for b in range(3)]
    sup = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=8, eos_token_id=[], begin_suppress_tokens=first,
                     sampler=sampler).cpu()[:, T_IN:]
    assert all(int(sup[b, 0]) not in first for b in range(3))
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, max_new_tokens=4, bad_words_ids=[list(range(2, 2 + E.CONSTRAIN_MAX_SEQ_LEN + 1))])
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, max_new_tokens=4, no_repeat_ngram_size=-1)


def test_generate_n_per_prompt_no_repeat(tiny):
    cfg, m, ids, am, free = tiny
    n = 3
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], do_sample=True, temperature=0.7, top_k=8,
              seed=17, sampler="engine", num_return_sequences=n)
    loose = m.generate(**kw).cpu()[:, T_IN:]
    assert any(R.has_repeated_ngram(_real(ids, am, loose[r], r // n), 2) for r in range(3 * n)), "nothing to prevent"
    out = m.generate(no_repeat_ngram_size=2, **kw).cpu()
    assert out.shape == (3 * n, T_IN + NEW) and torch.equal(out[:, :T_IN], ids.repeat_interleave(n, 0))
    _check_no_repeat(ids, am, loose, out[:, T_IN:], 2, npp=n, greedy=False)
    assert len({tuple(r.tolist()) for r in out[:, T_IN:]}) > 3, "the samples of a prompt must differ"
