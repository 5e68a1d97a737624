"""-m gpu: prompt-lookup decoding (n-gram proposals from the row's own history).

slam_ngram_propose against tests/lookup_ref.py, every output array exactly, with padding that would match, poisoned outputs and
forced rows; generate(prompt_lookup_num_tokens=) greedy against HuggingFace's own greedy (tests/golden/generate.npz, the
near-tie rule of test_assisted_greedy_matches_hf_golden), sampled against a replay of its trace through the restatements, and
on a model whose greedy continuation is periodic, where proposals MUST be accepted; the plain generate against its own loop
restated with the engine's primitives, and the refusals on a device model."""
import functools

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import lookup_ref as L
from tests import spec_ref as S
from tests.gpu_util import rel_err, sync
from tests.test_gpu_generate import GOLDEN, LOGITS_TOL, _mk, _tiny, _wide

pytestmark = pytest.mark.gpu

CANARY = -5
POISON = -7777
SEED = 11
FILL = 1
LHS = [1, 2, 3, 255, 256, 257, 1025]  # history lengths: around the block's 256-thread stride, and several strides


# ---- slam_ngram_propose ---------------------------------------------------------------------------------------------------------
def _rows(B, shift, rng):
    """B rows: lengths and prompt / new splits cycle with co-prime periods (7 lengths x { all prompt, all new, the boundary
    inside the last two tokens }), ids from 3 .. 6 symbols, every fifth row ends in a copy of an earlier stretch of 1, 4, 16 or
    17 tokens. The columns behind prompt_len and behind n_new repeat the row's last tokens: they WOULD match if they were read."""
    hist, plen = [], []
    for b in range(B):
        Lh = LHS[(b + shift) % 7]
        h = (rng.integers(0, 3 + b % 4, Lh) + 10).tolist()
        if b % 5 == 0 and Lh >= 40:
            m = [1, 4, 16, 17][(b // 5 + shift) % 4]
            s = int(rng.integers(0, Lh - 2 * m))
            h[Lh - m:] = h[s:s + m]
        kind = (b + shift) % 3
        hist.append(h)
        plen.append(Lh if kind == 0 else 0 if kind == 1 else max(Lh - 1 - b % 2, 0))
    plen = np.array(plen, np.int32)
    n_new = np.array([len(h) for h in hist], np.int32) - plen
    prompt = np.zeros((B, int(plen.max()) + 5), np.int64)
    new = np.zeros((B, int(n_new.max()) + 5), np.int64)
    for b, h in enumerate(hist):
        prompt[b, :plen[b]] = h[:plen[b]]
        prompt[b, plen[b]:] = np.resize(h[-4:], prompt.shape[1] - plen[b])
        new[b, :n_new[b]] = h[plen[b]:]
        new[b, n_new[b]:] = np.resize(h[-4:], new.shape[1] - n_new[b])
    done = np.array([(b + shift) % 6 == 5 for b in range(B)], np.uint8)
    return prompt, plen, new, n_new, done


def _launch(chunk0, prompt, plen, new, n_new, done, mx, eos, with_stats=True):
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(chunk=chunk0, prompt=prompt, plen=plen, new=new, n_new=n_new,
                                                           done=done).items()}
    B = chunk0.shape[0]
    n_prop = torch.full((B,), CANARY, dtype=torch.int32, device="cuda")
    stats = torch.full((2,), CANARY, dtype=torch.int32, device="cuda") if with_stats else None
    eos_t = torch.tensor(eos, dtype=torch.int32, device="cuda") if eos else None
    E.ngram_propose(d["chunk"], n_prop, mx, FILL, d["prompt"], d["plen"], d["new"], d["n_new"], d["done"], eos_t, stats)
    sync()
    return d["chunk"].cpu().numpy(), n_prop.cpu().numpy(), None if stats is None else stats.cpu().numpy()


@pytest.mark.parametrize("mx", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 4, 15])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_ngram_propose_matches_restatement(B, K, mx):
    rng = np.random.default_rng(B * 1000 + K * 20 + mx)
    sizes, counts, combos = set(), set(), set()
    for shift in range(21 if B < 21 else 3):  # every (length, split) pair occurs, whatever B
        prompt, plen, new, n_new, done = _rows(B, shift, rng)
        eos = [10, 500] if shift % 2 == 0 else []  # a symbol every row uses, and an id that never occurs
        chunk0 = np.full((B, K + 1), POISON, np.int64)
        chunk0[:, 0] = 70 + np.arange(B)
        want = L.propose_rows(chunk0, prompt, plen, new, n_new, done, K, mx, FILL, eos)
        chunk, n_prop, stats = _launch(chunk0, prompt, plen, new, n_new, done, mx, eos)
        assert np.array_equal(chunk[:, 0], chunk0[:, 0]), (B, K, mx, shift, "column 0 was written")
        assert np.array_equal(n_prop, want["n_prop"]), (B, K, mx, shift, n_prop, want["n_prop"])
        assert np.array_equal(chunk, want["chunk"]), (B, K, mx, shift)
        assert np.array_equal(stats, want["stats"]) and stats[1] == n_prop.sum() and stats[0] == (n_prop > 0).sum()
        assert (n_prop[done != 0] == 0).all()
        for b in range(B):
            sizes.add(L.propose(L.history(prompt, plen, new, n_new, b), K, mx, eos)[1])
            combos.add((int(plen[b] + n_new[b]), (b + shift) % 3))
        counts |= set(n_prop.tolist())
        if shift == 0:  # without stats: one launch, the same arrays; and a second run gives the same bits
            again = _launch(chunk0, prompt, plen, new, n_new, done, mx, eos, with_stats=False)
            assert np.array_equal(again[0], chunk) and np.array_equal(again[1], n_prop) and again[2] is None
    assert combos == {(n, k) for n in LHS for k in range(3)}
    assert {0, K} <= counts, (B, K, mx, counts)        # rows that propose nothing and rows that propose all K
    assert {0, 1, mx} <= sizes and max(sizes) == mx, (B, K, mx, sizes)  # no match, the shortest n-gram, and max_ngram itself


def test_ngram_propose_forced_rows():
    """Hand-worked rows in one launch (K = 3, max_ngram = 3, EOS id 9), with the expected arrays written out."""
    rows = [([7, 7], 2),                       # the continuation is cut by the end of the history
            ([5, 5, 5, 5], 1),                 # a match overlapping the tail: n = 3 at idx 0
            ([1, 2, 9, 4, 2, 3, 1, 2], 5),     # EOS is the first candidate: nothing, although n = 1 would have matched
            ([1, 2, 3, 9, 4, 1, 2], 7),        # EOS in the middle
            ([1, 2, 3, 4, 1, 2, 3], 3),        # done
            ([6], 1),                          # Lh == 1
            ([1, 2, 5, 7, 1, 2, 4, 7, 1, 2], 4),   # the longest n beats an earlier match of a shorter one
            ([1, 2, 3, 8, 5, 1, 2, 4, 6, 1, 2], 11)]  # n = 2 twice: the EARLIEST wins; all in the prompt
    B, K = len(rows), 3
    plen = np.array([p for _, p in rows], np.int32)
    n_new = np.array([len(h) - p for h, p in rows], np.int32)
    prompt = np.full((B, 12), 2, np.int64)  # the padding is a token of every history
    new = np.full((B, 12), 2, np.int64)
    for b, (h, p) in enumerate(rows):
        prompt[b, :p] = h[:p]
        new[b, :len(h) - p] = h[p:]
    done = np.array([0, 0, 0, 0, 1, 0, 0, 0], np.uint8)
    chunk0 = np.full((B, K + 1), POISON, np.int64)
    chunk, n_prop, stats = _launch(chunk0, prompt, plen, new, n_new, done, 3, [9])
    assert n_prop.tolist() == [1, 1, 0, 1, 0, 0, 3, 3]
    assert chunk[:, 1:].tolist() == [[7, FILL, FILL], [5, FILL, FILL], [FILL] * 3, [3, FILL, FILL], [FILL] * 3, [FILL] * 3,
                                    [4, 7, 1], [3, 8, 5]]
    assert (chunk[:, 0] == POISON).all() and stats.tolist() == [5, 9]
    want = L.propose_rows(chunk0, prompt, plen, new, n_new, done, K, 3, FILL, [9])
    assert np.array_equal(chunk, want["chunk"]) and np.array_equal(n_prop, want["n_prop"])


# ---- generate(prompt_lookup_num_tokens=) ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _model(tag):
    cfg, sd = _tiny() if tag == "tiny" else _wide()
    return cfg, _mk(cfg, sd, max_tokens=512)


@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_lookup_greedy_matches_hf_golden(tag, K, gold):
    _, m = _model(tag)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    want = torch.from_numpy(gold[f"{tag}_seq"])
    margin = torch.from_numpy(gold[f"{tag}_margin"])
    eos = int(gold[f"{tag}_eos"])
    nnew = int(gold["max_new_tokens"])
    out = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(), max_new_tokens=nnew,
                     eos_token_id=eos, pad_token_id=0, prompt_lookup_num_tokens=K,
                     max_matching_ngram_size={1: None, 4: 3, 7: 1}[K],  # the default (2), a longer and the shortest n-gram
                     prefill_chunk=32 if K == 4 else None).cpu()  # K = 4 also prefills in chunks
    assert out.dtype == torch.int64 and out.shape == want.shape, (out.shape, want.shape)
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids)
    tol = 2 * LOGITS_TOL * float(gold[f"{tag}_score_rms"])
    new, wnew = out[:, T:], want[:, T:]
    unchecked = []
    for b in range(want.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else wnew.shape[1]  # steps before the first near-tie must agree exactly
        diff = (new[b] != wnew[b]).nonzero()
        first = int(diff[0]) if len(diff) else wnew.shape[1]
        assert first >= trust, (tag, K, b, "diverged at", first, "before the first near-tie", trust)
        if trust == 0:
            unchecked.append(b)
    assert unchecked == ([1] if tag == "tiny" else []), (tag, unchecked)
    st = m.last_assist_stats
    print(f"[lookup] {tag} K={K}: {st}")
    assert st["tokens"] >= st["rounds"] >= 1 and st["accepted"] >= 0 and 0 <= st["proposed"] <= st["rounds"] * ids.shape[0] * K


def _sampling_case(cfg):
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, cfg.vocab, (4, 16), generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0
    am[3, :11] = 0
    return ids, am, torch.tensor([40, 3, 1 << 33, 7])


def _compact(ids, am):
    """The prompts as the kernel sees them: real tokens to the left, [B, max len], and their lengths."""
    plen = am.sum(1).numpy().astype(np.int32)
    prompt = np.zeros((ids.shape[0], int(plen.max())), np.int64)
    for b in range(ids.shape[0]):
        prompt[b, :plen[b]] = ids[b][am[b].bool()].numpy()
    return prompt, plen


def test_lookup_sampling_replays_through_the_restatement():
    cfg, m = _model("tiny")
    ids, am, sample_ids = _sampling_case(cfg)
    K, ngram, nnew, T = 4, 2, 20, ids.shape[1]
    bad = [[5], [11]]
    kw = dict(bad_words_ids=bad, do_sample=True, temperature=0.8, top_k=25, max_new_tokens=nnew, seed=SEED, sampler="engine",
              pad_token_id=0)
    plain = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=[], **kw).cpu()
    eos = [int(plain[1, T + 6]), int(plain[2, T + 13])]  # ids that occur: rows end at different steps
    m._lookup_trace = trace = []
    try:
        out = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=eos, prompt_lookup_num_tokens=K,
                         max_matching_ngram_size=ngram, **kw).cpu()
    finally:
        m._lookup_trace = None
    new = out[:, T:].numpy()
    B, n = new.shape
    assert torch.equal(out[:, :T], ids) and len(trace) == m.last_assist_stats["rounds"] >= 1
    assert np.isin(new, eos).any(), "the case needs an EOS id that occurs"
    banned = np.zeros(cfg.vocab, np.uint8)
    banned[[w[0] for w in bad]] = 1
    prompt, plen = _compact(ids, am)
    # replay: token 0 as returned, then every round through the restatements
    rep = np.zeros((B, nnew), np.int64)
    rep[:, 0] = new[:, 0]
    n_new = np.ones(B, np.int32)
    done = np.isin(new[:, 0], eos).astype(np.uint8)
    chunk0 = new[:, 0].copy()
    draws = excluded = proposed = 0
    emitted = []  # (row, position among the new tokens, round, column): where every emitted token's logits are
    for r, (chunk, logits_all, n_before, tgt, n_after, n_prop) in enumerate(trace):
        chunk, logits_all, tgt = chunk.numpy(), logits_all.numpy(), tgt.numpy()
        assert np.array_equal(n_before.numpy(), n_new) and np.array_equal(chunk[:, 0], chunk0), r
        prop = L.propose_rows(chunk, prompt, plen, rep, n_new, done, K, ngram, 0, eos)  # on the REPLAYED history
        assert np.array_equal(chunk, prop["chunk"]) and np.array_equal(n_prop.numpy(), prop["n_prop"]), (r, chunk, prop)
        proposed += int(prop["n_prop"].sum())
        live = [b for b in range(B) if not done[b]]
        ref, excl = S.target_tokens(logits_all, n_new, live, banned, True, 25, 0.8, 1.0, SEED, sample_ids.numpy())
        use = tgt.copy()
        for i, b in enumerate(live):
            ok = ~excl[i]
            assert np.array_equal(tgt[b][ok], ref[i][ok]), (r, b, tgt[b], ref[i])
            use[b][ok] = ref[i][ok]
        draws += excl.size
        excluded += int(excl.sum())
        res = S.accept(chunk, use, n_new, done, plen, rep, K, nnew, 0, eos)
        for b in live:
            emitted += [(b, int(n_new[b]) + j, r, j) for j in range(int(res["n_new"][b] - n_new[b]))]
        rep, n_new, done, chunk0 = res["out"], res["n_new"], res["done"], res["chunk"][:, 0]
        assert np.array_equal(n_after.numpy(), n_new), r
    print(f"[lookup] sampled: {m.last_assist_stats}, tokens per row {n_new.tolist()}, {draws} draws, {excluded} excluded, "
          f"equal to the plain call: {[bool((new[b, :k] == plain[b, T:T + k].numpy()).all()) for b, k in enumerate(n_new)]}")
    assert done.all() and int(n_new.max()) == n and m.last_assist_stats["proposed"] == proposed
    assert excluded <= 0.03 * draws, (excluded, draws)
    for b in range(B):
        assert np.array_equal(rep[b, :n_new[b]], new[b, :n_new[b]]) and (new[b, n_new[b]:] == 0).all(), b
    # the traced logits of every emitted position against one full forward of the finished rows: a wrong rollback shows here
    for b in range(B):
        row = torch.cat([ids[b][am[b].bool()], torch.from_numpy(new[b, :n_new[b]])])[None]
        fwd = m(input_ids=row).logits[0].float().cpu()
        for (bb, pos, r, j) in emitted:
            if bb == b:
                e = rel_err(trace[r][1][b, j], fwd[plen[b] + pos - 1])
                assert e <= LOGITS_TOL, (b, pos, r, j, e)
    # global indices as sample_ids: a row alone draws what it draws in the batch
    for b in range(B):
        alone = m.generate(input_ids=ids[b:b + 1][:, am[b].bool()], sample_ids=sample_ids[b:b + 1], eos_token_id=eos,
                           prompt_lookup_num_tokens=K, max_matching_ngram_size=ngram, **kw).cpu()
        assert np.array_equal(alone[0, plen[b]:].numpy(), new[b, :alone.shape[1] - plen[b]]), b
        assert alone.shape[1] - plen[b] == n_new[b]


# ---- a model whose greedy continuation is periodic: proposals must be accepted ---------------------------------------------------
ALLOWED = [7, 19, 101, 230, 377, 480]


def _periodic():
    """The tiny state dict with every o_proj and down_proj zeroed: both residual branches vanish, the stream is the current
    token's embedding and the logits depend on the last token alone. With all but six ids suppressed, greedy decoding is a
    walk on six states. Returns (cfg, sd, the bf16-rounded oracle's logits [vocab, vocab]: row t = the logits behind t)."""
    cfg, sd = _tiny()
    sd = {k: (torch.zeros_like(v) if k.endswith(("o_proj.weight", "down_proj.weight")) else v) for k, v in sd.items()}
    sd_bf = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    return cfg, sd, O.model_forward(cfg, sd_bf, torch.arange(cfg.vocab)[:, None])[:, 0]


def test_lookup_accepts_on_a_periodic_model():
    cfg, sd, lg = _periodic()
    m = _mk(cfg, sd, max_tokens=512)
    K, ngram, nnew = 4, 2, 40
    others = [t for t in range(2, cfg.vocab) if t not in ALLOWED]
    g = torch.Generator().manual_seed(22)  # a prompt seed whose four last tokens pass the margin check below, as the six ids do
    ids = torch.tensor(others)[torch.randint(0, len(others), (4, 9), generator=g)]
    am = torch.ones_like(ids)
    am[2, :4] = 0
    # every state the walk can be in - the six ids and the prompts' last tokens - has a clear winner among the six: the top-2
    # margin of the CPU oracle's logits exceeds twice the model tolerance on the row's RMS, so rounding cannot change a token
    states = ALLOWED + ids[:, -1].tolist()
    sub = lg[states][:, ALLOWED]
    top = sub.topk(2, -1).values
    need = 2 * LOGITS_TOL * lg[states].pow(2).mean(-1).sqrt()
    assert bool((top[:, 0] - top[:, 1] > need).all()), (top[:, 0] - top[:, 1], need)
    step = {s: ALLOWED[int(i)] for s, i in zip(states, sub.argmax(-1))}
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=nnew, eos_token_id=[], pad_token_id=0,
              suppress_tokens=[t for t in range(cfg.vocab) if t not in ALLOWED])
    plain = m.generate(**kw).cpu()
    m._lookup_trace = trace = []
    try:
        out = m.generate(prompt_lookup_num_tokens=K, max_matching_ngram_size=ngram, **kw).cpu()
    finally:
        m._lookup_trace = None
    T = ids.shape[1]
    assert torch.equal(out, plain) and out.shape == (4, T + nnew)
    for b in range(4):  # and both are the oracle's walk
        walk, s = [], int(ids[b, -1])
        for _ in range(nnew):
            s = step[s]
            walk.append(s)
        assert out[b, T:].tolist() == walk, b
    st = m.last_assist_stats
    print(f"[lookup] periodic model (functional figure, not a speed claim): {st}, "
          f"{st['accepted'] / max(st['proposed'], 1):.2f} of the proposals accepted, {st['tokens'] / (4 * st['rounds']):.2f} "
          f"tokens per row and round")
    assert 0 < st["accepted"] <= st["proposed"] and st["rounds"] < nnew and st["tokens"] == 4 * nnew
    # the stats are the replay's: every round through the restatement, greedy on the traced logits
    banned = np.ones(cfg.vocab, np.uint8)
    banned[ALLOWED] = 0
    prompt, plen = _compact(ids, am)
    new = out[:, T:].numpy()
    rep = np.zeros((4, nnew), np.int64)
    rep[:, 0] = new[:, 0]
    n_new, done = np.ones(4, np.int32), np.zeros(4, np.uint8)
    chunk = np.zeros((4, K + 1), np.int64)
    chunk[:, 0] = new[:, 0]
    rounds = proposed = accepted = 0
    tokens = 4
    while not done.all():
        res, prop, _ = L.lookup_round(chunk, trace[rounds][1].numpy(), prompt, plen, rep, n_new, done, K, ngram, nnew, 0, [], banned)
        assert np.array_equal(trace[rounds][0].numpy(), prop["chunk"]), rounds
        rounds += 1
        proposed += int(prop["stats"][1])
        tokens += int(res["stats"][3])
        accepted += int(res["stats"][4])
        rep, n_new, done, chunk = res["out"], res["n_new"], res["done"], res["chunk"]
    assert np.array_equal(rep, new)
    assert st == {"rounds": rounds, "proposed": proposed, "accepted": accepted, "tokens": tokens}


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def test_plain_generate_is_its_own_loop_restated():
    """Without the new arguments generate is what it was: the engine-sampler path, greedy, against prefill /
    slam_sample_tokens / slam_decode_step driven from here, token for token; and the lookup call emits the same tokens."""
    cfg, m = _model("tiny")
    ids, am, _ = _sampling_case(cfg)
    nnew, T = 12, ids.shape[1]
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=nnew, sampler="engine", eos_token_id=[], pad_token_id=0)
    out = m.generate(**kw).cpu()
    dev, B, V = m.device, ids.shape[0], cfg.vocab
    prompt, plen = _compact(ids, am)
    lens = torch.from_numpy(plen).to(dev)
    P = prompt.shape[1]
    m._ensure_workspace(max(B * P, 2 * B))
    cap = -(-(P + nnew) // 64) * 64
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap) + 256, dtype=torch.uint8, device=dev)
    off = (-cache.data_ptr()) % 256
    m.engine.bind_kv_cache(cache[off:], B, cap)
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    m.engine.prefill(torch.from_numpy(prompt).to(dev), lens, B, P, logits)
    ws = torch.empty(E.sample_workspace_bytes(B, V, 1), dtype=torch.uint8, device=dev)
    nxt = torch.empty(B, dtype=torch.int64, device=dev)
    new = torch.empty(B, nnew, dtype=torch.int64, device=dev)
    for s in range(nnew):
        desc = E.SlamSampleDesc(do_sample=0, top_k=1, temperature=1.0, top_p=1.0, seed=0, step=s, pad_id=0, n_eos=0)
        E.sample_tokens(logits, desc, nxt, ws, None, None, None, None, new)
        if s + 1 < nnew:
            m.engine.decode_step(nxt, lens, B, logits)
    sync()
    assert torch.equal(out[:, T:], new.cpu())


def test_lookup_refusals_on_the_device_model():
    cfg, m = _model("tiny")
    ids = torch.randint(2, cfg.vocab, (2, 6), generator=torch.Generator().manual_seed(1))
    kw = dict(input_ids=ids, max_new_tokens=4)
    with pytest.raises(ValueError, match="exclude each other"):
        m.generate(prompt_lookup_num_tokens=4, assistant_model=_mk(cfg, None, max_tokens=512, seed=5), **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size needs"):
        m.generate(max_matching_ngram_size=2, **kw)
    for k, n in ((0, None), (16, None), (4, 0), (4, 17)):
        with pytest.raises(ValueError, match="must be an int"):
            m.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n, **kw)
    with pytest.raises(ValueError, match="sampler='engine'"):
        m.generate(prompt_lookup_num_tokens=4, do_sample=True, top_k=5, **kw)
    with pytest.raises(ValueError, match="return_logprobs"):
        m.generate(prompt_lookup_num_tokens=4, return_logprobs=True, **kw)
    with pytest.raises(ValueError, match="history-dependent"):
        m.generate(prompt_lookup_num_tokens=4, no_repeat_ngram_size=2, **kw)
    with pytest.raises(ValueError, match="1024 rows"):
        m.generate(input_ids=ids[:1].expand(1025, -1), max_new_tokens=4, prompt_lookup_num_tokens=4)
    with pytest.raises(TypeError, match="unsupported arguments"):
        m.generate(prompt_lookup_tokens=4, **kw)  # a misspelt name is still refused
    out = m.generate(prompt_lookup_num_tokens=15, max_matching_ngram_size=16, **kw).cpu()  # the limits themselves are served
    assert out.shape == (2, 10) and torch.equal(out[:, :7], m.generate(**kw).cpu()[:, :7])  # token 0: the prefill's logits
