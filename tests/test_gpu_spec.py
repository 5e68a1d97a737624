"""-m gpu: assisted generation (draft-model speculative decoding).

slam_spec_accept against tests/spec_ref.py, every output array exactly; slam_sample_tokens_at row by row against
slam_sample_tokens on that row alone (and slam_sample_tokens against its own reference, unchanged); slam_extend_logits against
slam_extend (cache and lens bit for bit) and one full forward (rel-RMS <= LOGITS_TOL of test_gpu_generate.py, per written row),
with the rollback of slam_kv_rewind; generate(assistant_model=) greedy against HuggingFace's own greedy
(tests/golden/generate.npz, the near-tie rule of test_generate_chunked_matches_hf_golden) and sampled against a replay of its
trace through the restatements; the plain generate against its own loop restated with the engine's primitives."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import sampling_ref as R
from tests import spec_ref as S
from tests.gpu_util import lib, ptr, rel_err, stream, sync
from tests.test_gpu_generate import GOLDEN, LOGITS_TOL, _mk, _tiny, _wide

pytestmark = pytest.mark.gpu

POISON = 0x7FC1  # a bf16 NaN
CANARY = -5
SEED = 11


# ---- slam_spec_accept -----------------------------------------------------------------------------------------------------------
def _accept_case(B, K, shift, rng):
    """Rows with a forced agreement prefix of (b + shift) % (K + 1) proposals; EOS ids inside and right behind the accepted run,
    n_new close to max_new and finished rows spread over the rows by small co-prime periods."""
    max_new, eos = 3 * K + 9, [60, 61]
    tgt = rng.integers(2, 50, (B, K + 1))
    chunk = rng.integers(2, 50, (B, K + 1))
    n_new = rng.integers(1, max_new - K - 1, B)
    done = np.zeros(B, np.uint8)
    for b in range(B):
        a = (b + shift) % (K + 1)
        kind = (b // (K + 1) + b + shift) % 4
        if kind == 1 and a > 0:
            tgt[b, a // 2] = eos[0]      # inside the accepted run
        if kind == 2:
            tgt[b, a] = eos[1]           # right behind it: the correction token
        chunk[b, 1:a + 1] = tgt[b, :a]
        if a < K:
            chunk[b, a + 1] = tgt[b, a] + 1 if tgt[b, a] < 50 else 2  # never equal, never an EOS id
        if (b + shift) % 5 == 0:
            n_new[b] = max_new - 1 - (b + shift) % 3
        if (b + 2 * shift) % 3 == 2:
            done[b] = 1
    prompt_len = rng.integers(1, 40, B)
    return chunk, tgt, n_new.astype(np.int32), done, prompt_len.astype(np.int32), max_new, eos


@pytest.mark.parametrize("K", [1, 2, 7, 15])
@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_spec_accept_matches_restatement(B, K):
    rng = np.random.default_rng(B * 100 + K)
    seen = set()
    for shift in range(max(K + 1, 6)):
        chunk, tgt, n_new, done, plen, max_new, eos = _accept_case(B, K, shift, rng)
        stride = max_new + 3
        out0 = np.full((B, stride), CANARY, np.int64)
        want = S.accept(chunk, tgt, n_new, done, plen, out0, K, max_new, 0, eos)
        d = {k: torch.from_numpy(v).cuda() for k, v in dict(chunk=chunk, tgt=tgt, n_new=n_new, done=done, prompt_len=plen,
                                                               out=out0).items()}

        def i32(n):
            return torch.full((n,), CANARY, dtype=torch.int32, device="cuda")

        d.update(lens_t=i32(B), lens_d=i32(B), draft_new_lens=i32(B), tgt_new_lens=i32(B), stats=i32(5),
                 draft_ids=torch.full((B, 2), CANARY, dtype=torch.int64, device="cuda"))
        E.spec_accept(d["chunk"], d["tgt"], K, max_new, 0, torch.tensor(eos, dtype=torch.int32, device="cuda"), d["prompt_len"],
                      d["n_new"], d["done"], d["out"], d["lens_t"], d["lens_d"], d["draft_ids"], d["draft_new_lens"],
                      d["tgt_new_lens"], d["stats"])
        sync()
        for k, w in want.items():
            assert np.array_equal(d[k].cpu().numpy(), w), (B, K, shift, k)
        # the canary: out is untouched outside [n_new, n_new + m)
        m = want["n_new"] - np.minimum(n_new, max_new)
        col = np.arange(stride)[None]
        inside = (col >= n_new[:, None]) & (col < (n_new + m)[:, None])
        got = d["out"].cpu().numpy()
        assert (got[~inside] == CANARY).all() and (got[inside] != CANARY).all(), (B, K, shift)
        live = done == 0
        seen |= set(m[live].tolist())
        assert (m[live] >= 1).all() and (m[~live] == 0).all()
    if B >= 64:
        assert seen == set(range(1, K + 2)), (B, K, seen)  # every number of emitted tokens occurred


# ---- slam_sample_tokens_at ------------------------------------------------------------------------------------------------------
def _desc(do_sample, step, n_eos=0):
    return E.SlamSampleDesc(do_sample=do_sample, top_k=25 if do_sample else 1, temperature=0.8 if do_sample else 1.0, top_p=1.0,
                            seed=SEED, step=step, pad_id=0, n_eos=n_eos)


@functools.lru_cache(maxsize=None)
def _logits(V, B):
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(V * 7 + B)) * 3.0
    return x, x.cuda()


@pytest.mark.parametrize("do_sample", [1, 0])
@pytest.mark.parametrize("group", [1, 5])
@pytest.mark.parametrize("V", [502, 4100])
def test_sample_tokens_at_equals_one_row_calls(V, group, do_sample):
    B, base = 10, 3
    x, xd = _logits(V, B)
    nq = B // group
    rng = np.random.default_rng(V + group)
    steps = torch.from_numpy(rng.integers(0, 200, nq).astype(np.int32)).cuda()
    row_ids = torch.from_numpy(rng.integers(0, 1 << 40, nq)).cuda()
    banned = torch.zeros(V, dtype=torch.uint8, device="cuda")
    banned[x.argmax(-1).cuda()] = 1  # every row's best token
    banned[7] = 1
    ws = torch.empty(E.sample_workspace_bytes(B, V, 25), dtype=torch.uint8, device="cuda")
    nxt = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((B, 4), CANARY, dtype=torch.int64, device="cuda")
    E.sample_tokens_at(xd, _desc(do_sample, base), nxt, ws, steps, group, 2, banned, row_ids, out=out)
    sync()
    assert torch.equal(out[:, 2], nxt) and (out[:, [0, 1, 3]] == CANARY).all()
    one = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for b in range(B):
        q, j = divmod(b, group)
        E.sample_tokens(xd[b:b + 1], _desc(do_sample, base + int(steps[q]) + j), one, ws, banned, row_ids[q:q + 1])
        sync()
        assert int(one) == int(nxt[b]), (V, group, do_sample, b)
        assert banned[int(nxt[b])] == 0
    # no row ids, no steps: sequence q draws with row id q at step base + j
    E.sample_tokens_at(xd, _desc(do_sample, base), nxt, ws, None, group, 0, banned)
    sync()
    for b in range(B):
        q, j = divmod(b, group)
        E.sample_tokens(xd[b:b + 1], _desc(do_sample, base + j), one, ws, banned, torch.tensor([q], device="cuda"))
        sync()
        assert int(one) == int(nxt[b]), (V, group, do_sample, b, "defaults")


@pytest.mark.parametrize("V", [502, 4100])
def test_sample_tokens_itself_is_unchanged(V):
    """slam_sample_tokens against the fp64 restatement, by the rule (and under the cap) of test_gpu_sampling.py."""
    B = 10
    x, xd = _logits(V, B)
    steps = [0, 1, 2, 77] + list(range(100, 116))
    ws = torch.empty(E.sample_workspace_bytes(B, V, 25), dtype=torch.uint8, device="cuda")
    nxt = torch.empty(B, dtype=torch.int64, device="cuda")
    out = torch.full((B, 120), CANARY, dtype=torch.int64, device="cuda")
    for s in steps:
        E.sample_tokens(xd, _desc(1, s), nxt, ws, out=out)
    sync()
    got = out[:, steps].cpu().numpy()
    assert (out.cpu().numpy() != CANARY).sum() == B * len(steps)  # column desc.step, nothing else
    want, excl = np.empty_like(got), np.zeros(got.shape, bool)
    for b in range(B):
        tok, dist, margin = R.sample_row(x[b].numpy(), None, 25, 0.8, 1.0, SEED, [b], steps, fp64=True)
        want[b], excl[b] = tok[0], (dist[0] <= 1e-5) | (margin <= 1e-5)
    assert excl.mean() <= 0.03
    assert (got[~excl] == want[~excl]).all()
    E.sample_tokens(xd, _desc(0, 0), nxt, ws)
    sync()
    assert nxt.tolist() == [R.greedy(x[b].numpy()) for b in range(B)]


# ---- slam_extend_logits and slam_kv_rewind --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(tag):
    cfg, sd = _tiny() if tag == "tiny" else _wide()
    return cfg, _mk(cfg, sd, max_tokens=512)


def _poisoned_cache(m, cfg, rows, cap):
    nb = m.engine.kv_cache_bytes(rows, cap)
    cache = torch.full((nb // 2,), POISON, dtype=torch.int16, device=m.device)
    m.engine.bind_kv_cache(cache, rows, cap)
    return cache.view(cfg.n_layers, 2, rows, cfg.n_kv_heads, cap, cfg.head_dim)


@pytest.mark.parametrize("B,T", [(3, 2), (3, 5), (5, 16)])
def test_extend_logits_matches_extend_and_forward(B, T):
    cfg, m = _model("tiny")
    dev, V, cap = m.device, cfg.vocab, 128
    m._ensure_workspace(256)
    g = torch.Generator().manual_seed(B * 31 + T)
    base = [37, 20, 5, 1, 33][:B]
    new = [T, 0, max(1, T // 2), T, 1][:B]   # ragged: 0 and T included
    keep = [max(0, n - 1 - b % 2) for b, n in enumerate(new)]  # what a rollback keeps: fewer tokens on every row with some
    P = max(base)
    full = torch.randint(2, V, (B, P + 2 * T), generator=g)  # row b: base[b] prompt tokens, the chunk, then the second chunk
    alt = torch.randint(2, V, (B, T), generator=g)
    ids = torch.zeros(B, P, dtype=torch.long)
    chunk = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        ids[b, :base[b]] = full[b, :base[b]]
        chunk[b, :new[b]] = full[b, base[b]:base[b] + new[b]]
    ids_d, chunk_d, alt_d = ids.to(dev), chunk.to(dev), alt.to(dev)
    new_d = torch.tensor(new, dtype=torch.int32, device=dev)
    base_d = torch.tensor(base, dtype=torch.int32, device=dev)
    last = torch.empty(B, V, dtype=torch.float32, device=dev)

    def prefill():
        kv = _poisoned_cache(m, cfg, B, cap)
        lens = base_d.clone()
        m.engine.prefill(ids_d, lens, B, P, last)
        return kv, lens

    kv_a, lens_a = prefill()
    la = torch.full((B, V), float("nan"), dtype=torch.float32, device=dev)
    m.engine.extend(chunk_d, new_d, lens_a, B, T, la)
    sync()
    kv_b, lens_b = prefill()
    allg = torch.full((B, T, V), float("nan"), dtype=torch.float32, device=dev)
    m.engine.extend_logits(chunk_d, new_d, lens_b, B, T, allg)
    sync()
    assert torch.equal(kv_a, kv_b), "the cache differs from slam_extend's"
    assert lens_a.tolist() == lens_b.tolist() == [base[b] + new[b] for b in range(B)]
    seq = torch.zeros(B, P + T, dtype=torch.long)
    for b in range(B):
        seq[b, :base[b] + new[b]] = full[b, :base[b] + new[b]]
    fwd = m(input_ids=seq).logits.float().cpu()
    got = allg.cpu()
    for b in range(B):
        assert torch.isnan(got[b, new[b]:]).all(), (b, "an unwritten row was written")
        for t in range(new[b]):
            e = rel_err(got[b, t], fwd[b, base[b] + t])
            assert torch.isfinite(got[b, t]).all() and e <= LOGITS_TOL, (B, T, b, t, e)
        if new[b]:  # the last real row is what slam_extend's head gives, up to the head launch's shape
            assert rel_err(got[b, new[b] - 1], la[b].cpu()) <= LOGITS_TOL
    # rollback: keep[b] of the new tokens stay, the bound comes down, another chunk follows. The reference is a cache that
    # never held the rolled-back keys, brought to the same host bound.
    hi = max(base[b] + keep[b] for b in range(B))
    alt_new = torch.tensor([min(T, 1 + b) for b in range(B)], dtype=torch.int32, device=dev)
    lens_b.copy_(torch.tensor([base[b] + keep[b] for b in range(B)], dtype=torch.int32))
    assert lib().slam_kv_rewind(m.engine.h, 0) == -1 and lib().slam_kv_rewind(m.engine.h, P + T + 1) == -1
    m.engine.kv_rewind(hi)
    assert lib().slam_kv_rewind(m.engine.h, hi + 1) == -1  # the bound is hi now
    assert lib().slam_kv_repeat(m.engine.h, 1, ptr(lens_b), None, stream()) == -2  # refused behind a rewind
    one = torch.full((B, T, V), float("nan"), dtype=torch.float32, device=dev)
    m.engine.extend_logits(alt_d, alt_new, lens_b, B, T, one)
    sync()
    kv_c, lens_c = prefill()
    m.engine.extend_logits(chunk_d, torch.tensor(keep, dtype=torch.int32, device=dev), lens_c, B, T, allg)
    m.engine.kv_rewind(hi)
    two = torch.full((B, T, V), float("nan"), dtype=torch.float32, device=dev)
    m.engine.extend_logits(alt_d, alt_new, lens_c, B, T, two)
    sync()
    assert lens_b.tolist() == lens_c.tolist()
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)), "rolled-back keys changed the logits"
    seq = torch.zeros(B, P + 2 * T, dtype=torch.long)
    for b in range(B):
        n0, n1 = base[b] + keep[b], int(alt_new[b])
        seq[b, :n0] = full[b, :n0]
        seq[b, n0:n0 + n1] = alt[b, :n1]
    fwd = m(input_ids=seq).logits.float().cpu()
    for b in range(B):
        for t in range(int(alt_new[b])):
            e = rel_err(one[b, t].cpu(), fwd[b, base[b] + keep[b] + t])
            assert e <= LOGITS_TOL, (B, T, b, t, "behind the rollback", e)


# ---- generate(assistant_model=) -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _draft(tag, kind):
    """(a) "same": a second model from the target's own state dict; (b) "random": a seeded random model with one layer."""
    cfg, sd = _tiny() if tag == "tiny" else _wide()
    if kind == "same":
        return _mk(cfg, sd, max_tokens=512)
    return _mk(dataclasses.replace(cfg, n_layers=1), None, max_tokens=512, seed=5)


@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("kind", ["same", "random"])
@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_assisted_greedy_matches_hf_golden(tag, kind, K, gold):
    _, m = _model(tag)
    d = _draft(tag, kind)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    want = torch.from_numpy(gold[f"{tag}_seq"])
    margin = torch.from_numpy(gold[f"{tag}_margin"])
    eos = int(gold[f"{tag}_eos"])
    nnew = int(gold["max_new_tokens"])
    out = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(), max_new_tokens=nnew,
                     eos_token_id=eos, pad_token_id=0, assistant_model=d, num_assistant_tokens=K,
                     prefill_chunk=32 if K == 4 else None).cpu()  # K = 4 also prefills both models in chunks
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
        assert first >= trust, (tag, kind, K, b, "diverged at", first, "before the first near-tie", trust)
        if trust == 0:
            unchecked.append(b)
    assert unchecked == ([1] if tag == "tiny" else []), (tag, unchecked)
    st = m.last_assist_stats
    print(f"[assist] {tag} {kind} K={K}: {st}")
    assert st["tokens"] >= st["rounds"] >= 1 and 0 <= st["accepted"] <= st["proposed"]
    if kind == "same":
        assert st["rounds"] < new.shape[1], (tag, K, st)  # fewer target passes than tokens of the longest row


def _sampling_case(cfg):
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, cfg.vocab, (4, 16), generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0
    am[3, :11] = 0
    return ids, am, torch.tensor([40, 3, 1 << 33, 7])


@pytest.mark.parametrize("kind", ["same", "random"])
def test_assisted_sampling_replays_through_the_restatement(kind):
    cfg, m = _model("tiny")
    d = _draft("tiny", kind)
    ids, am, sample_ids = _sampling_case(cfg)
    K, nnew, T = 4, 20, ids.shape[1]
    bad = [[5], [11]]
    kw = dict(bad_words_ids=bad, do_sample=True, temperature=0.8, top_k=25, max_new_tokens=nnew, seed=SEED, sampler="engine",
              pad_token_id=0)
    plain = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=[], **kw).cpu()
    eos = [int(plain[1, T + 6]), int(plain[2, T + 13])]  # ids that occur: rows end at different steps
    m._assist_trace = trace = []
    try:
        out = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=eos, assistant_model=d,
                         num_assistant_tokens=K, **kw).cpu()
    finally:
        m._assist_trace = None
    new = out[:, T:].numpy()
    B, n = new.shape
    assert torch.equal(out[:, :T], ids) and len(trace) == m.last_assist_stats["rounds"] >= 1
    assert np.isin(new, eos).any(), "the case needs an EOS id that occurs"
    banned = np.zeros(cfg.vocab, np.uint8)
    banned[[w[0] for w in bad]] = 1
    plen = am.sum(1).numpy().astype(np.int32)
    # replay: token 0 as returned, then every round through the restatements
    rep = np.zeros((B, nnew), np.int64)
    rep[:, 0] = new[:, 0]
    n_new = np.ones(B, np.int32)
    done = np.isin(new[:, 0], eos).astype(np.uint8)
    chunk0 = new[:, 0].copy()
    draws = excluded = 0
    emitted = []  # (row, position among the new tokens, round, column): where every emitted token's logits are
    for r, (chunk, logits_all, n_before, tgt, n_after) in enumerate(trace):
        chunk, logits_all, tgt = chunk.numpy(), logits_all.numpy(), tgt.numpy()
        assert np.array_equal(n_before.numpy(), n_new) and np.array_equal(chunk[:, 0], chunk0), r
        live = [b for b in range(B) if not done[b]]
        ref, excl = S.target_tokens(logits_all, n_new, live, banned, True, 25, 0.8, 1.0, SEED, sample_ids.numpy())
        use = tgt.copy()
        for i, b in enumerate(live):
            ok = ~excl[i]
            assert np.array_equal(tgt[b][ok], ref[i][ok]), (kind, r, b, tgt[b], ref[i])
            use[b][ok] = ref[i][ok]
        draws += excl.size
        excluded += int(excl.sum())
        res = S.accept(chunk, use, n_new, done, plen, rep, K, nnew, 0, eos)
        for b in live:
            emitted += [(b, int(n_new[b]) + j, r, j) for j in range(int(res["n_new"][b] - n_new[b]))]
        rep, n_new, done, chunk0 = res["out"], res["n_new"], res["done"], res["chunk"][:, 0]
        assert np.array_equal(n_after.numpy(), n_new), r
    print(f"[assist] sampled, draft {kind}: {m.last_assist_stats}, tokens per row {n_new.tolist()}, {draws} draws, "
          f"{excluded} excluded, equal to the plain call: {[bool((new[b, :k] == plain[b, T:T + k].numpy()).all()) for b, k in enumerate(n_new)]}")
    assert done.all() and int(n_new.max()) == n
    assert excluded <= 0.03 * draws, (excluded, draws)
    for b in range(B):
        assert np.array_equal(rep[b, :n_new[b]], new[b, :n_new[b]]) and (new[b, n_new[b]:] == 0).all(), (kind, b)
    # the traced logits of every emitted position against one full forward of the finished rows: a wrong rollback shows here
    for b in range(B):
        row = torch.cat([ids[b][am[b].bool()], torch.from_numpy(new[b, :n_new[b]])])[None]
        fwd = m(input_ids=row).logits[0].float().cpu()
        for (bb, pos, r, j) in emitted:
            if bb == b:
                e = rel_err(trace[r][1][b, j], fwd[plen[b] + pos - 1])
                assert e <= LOGITS_TOL, (kind, b, pos, r, j, e)
    # global indices as sample_ids: a row alone draws what it draws in the batch
    for b in range(B):
        alone = m.generate(input_ids=ids[b:b + 1][:, am[b].bool()], sample_ids=sample_ids[b:b + 1], eos_token_id=eos,
                           assistant_model=d, num_assistant_tokens=K, **kw).cpu()
        assert np.array_equal(alone[0, plen[b]:].numpy(), new[b, :alone.shape[1] - plen[b]]), (kind, b)
        assert alone.shape[1] - plen[b] == n_new[b]


def test_plain_generate_is_its_own_loop_restated():
    """Without a draft generate is what it was: the engine-sampler path against prefill / slam_sample_tokens / slam_decode_step
    driven from here, token for token, with a fixed seed on the tiny model."""
    cfg, m = _model("tiny")
    ids, am, sample_ids = _sampling_case(cfg)
    nnew, T = 12, ids.shape[1]
    out = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, do_sample=True, temperature=0.8, top_k=25,
                     max_new_tokens=nnew, seed=SEED, sampler="engine", eos_token_id=[], pad_token_id=0).cpu()
    dev, B, V = m.device, ids.shape[0], cfg.vocab
    lens = am.sum(1).to(torch.int32).to(dev)
    P = int(lens.max())
    comp = torch.zeros(B, P, dtype=torch.long)
    for b in range(B):
        comp[b, :int(lens[b])] = ids[b][am[b].bool()]
    m._ensure_workspace(max(B * P, 2 * B))
    cap = -(-(P + nnew) // 64) * 64
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap) + 256, dtype=torch.uint8, device=dev)
    off = (-cache.data_ptr()) % 256
    m.engine.bind_kv_cache(cache[off:], B, cap)
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    m.engine.prefill(comp.to(dev), lens, B, P, logits)
    ws = torch.empty(E.sample_workspace_bytes(B, V, 25), dtype=torch.uint8, device=dev)
    nxt = torch.empty(B, dtype=torch.int64, device=dev)
    new = torch.empty(B, nnew, dtype=torch.int64, device=dev)
    rid = sample_ids.to(dev)
    for s in range(nnew):
        E.sample_tokens(logits, _desc(1, s), nxt, ws, None, rid, None, None, new)
        if s + 1 < nnew:
            m.engine.decode_step(nxt, lens, B, logits)
    sync()
    assert torch.equal(out[:, T:], new.cpu())
