"""-m gpu: the device sampler (slam_sample_tokens) and generate(sampler="engine").

The kernels against the fp64 restatement of the contract (tests/sampling_ref.py): the token must be the restatement's for every
(row, step) whose draw is further than 1e-5 (relative to the total weight) from a boundary of the cumulative weights and whose
row's top-p cut is further than 1e-5 from its threshold - fp32 sums of at most 256 weights are within 256 * 2^-24 = 1.5e-5 of the
fp64 ones in the worst case and within 1e-6 typically; such exclusions may make up at most 3 % of a configuration. Then the
structure of the contract (banned, -inf, NaN, ties, k' < top_k), its independence of batch, position and history, the EOS / done /
pad / out part, and the model level on the golden generation configs."""
import functools
import os

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate.npz")
SEED = 11
PAD = 0


def _sample(logits, do_sample=1, top_k=25, temperature=0.8, top_p=1.0, seed=SEED, step=0, banned=None, row_ids=None, eos=None,
            done=None, out=None, pad=PAD):
    """One slam_sample_tokens call on device tensors; returns next [B] on the CPU."""
    B, V = logits.shape
    desc = E.SlamSampleDesc(do_sample=do_sample, top_k=top_k, temperature=temperature, top_p=top_p, seed=seed, step=step,
                            pad_id=pad, n_eos=0 if eos is None else eos.numel())
    ws = torch.empty(E.sample_workspace_bytes(B, V, top_k if do_sample else 1), dtype=torch.uint8, device="cuda")
    nxt = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    E.sample_tokens(logits, desc, nxt, ws, banned, row_ids, eos, done, out)
    torch.cuda.synchronize()
    return nxt.cpu()


@functools.lru_cache(maxsize=None)
def _case(V, B):
    """(logits on the CPU, on the device, the 256 best candidates of every row in rank order): computed once per shape."""
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(V * 131 + B)) * 3.0
    ranked = [R.candidates(R.scores(x[b].numpy()), 256) for b in range(B)]
    return x, x.cuda(), ranked


SHAPES = [(17, 3), (502, 1), (502, 64), (2048, 3), (2049, 3), (4099, 8), (152167, 3), (152576, 64)]
PARAMS = [(25, 0.8, 1.0), (25, 0.8, 0.9), (256, 1.3, 0.7), (1, 1.0, 1.0), (40, 0.5, 1.0)]


@pytest.mark.parametrize("top_k,T,top_p", PARAMS)
@pytest.mark.parametrize("V,B", SHAPES)
def test_kernel_matches_fp64_restatement(V, B, top_k, T, top_p):
    x, xd, ranked = _case(V, B)
    n_steps = max(4, -(-192 // B))
    steps = [0, 1, 2, 77] + list(range(100, 100 + n_steps - 4))
    got = torch.stack([_sample(xd, 1, top_k, T, top_p, step=s) for s in steps], 1).numpy()
    want = np.empty_like(got)
    excluded = np.zeros(got.shape, dtype=bool)
    for b in range(B):
        tok, dist, margin = R.sample_row(x[b].numpy(), None, top_k, T, top_p, SEED, [b], steps, fp64=True, ranked=ranked[b])
        want[b] = tok[0]
        excluded[b] = (dist[0] <= 1e-5) | (margin <= 1e-5)
    frac = excluded.mean()
    print(f"V {V} B {B} k {top_k} T {T} p {top_p}: {got.size} draws, {frac:.3%} excluded, "
          f"{(got != want)[~excluded].sum()} mismatches")
    assert frac <= 0.03
    assert (got[~excluded] == want[~excluded]).all()
    kk = min(top_k, V)
    for b in range(B):
        assert set(got[b].tolist()) <= set(ranked[b][:kk].tolist()), b  # the excluded draws are candidates too


@pytest.mark.parametrize("V,B", SHAPES)
def test_greedy_is_lowest_index_argmax(V, B):
    x, xd, ranked = _case(V, B)
    got = _sample(xd, do_sample=0)
    assert got.tolist() == [int(r[0]) for r in ranked]
    # equal maxima: the lowest index, also across chunk boundaries and in the last, short chunk
    y = x.clone()
    top = float(y.max()) + 1.0
    for b in range(B):
        for i in {V - 1, V // 2, (7 * b + 3) % V}:
            y[b, i] = top
    got = _sample(y.cuda(), do_sample=0)
    assert got.tolist() == [min(V - 1, V // 2, (7 * b + 3) % V) for b in range(B)]


@pytest.mark.parametrize("V", [502, 4099, 152167])
def test_banned_inf_nan_and_ties(V):
    B = 4
    x, _, _ = _case(V, 8)
    x = x[:B].clone()
    steps = range(24)
    # a banned mask leaving 3 finite tokens: only those are ever drawn
    keep = [5, V // 2, V - 1]
    banned = torch.ones(V, dtype=torch.uint8)
    banned[keep] = 0
    bd = banned.cuda()
    xd = x.cuda()
    got = torch.stack([_sample(xd, 1, 25, 0.8, 1.0, step=s, banned=bd) for s in steps], 1)
    assert set(got.flatten().tolist()) <= set(keep)
    assert len(set(got.flatten().tolist())) > 1
    for b in range(B):  # k' = 3 < top_k: the restatement with the same mask
        tok, dist, _ = R.sample_row(x[b].numpy(), banned.numpy(), 25, 0.8, 1.0, SEED, [b], list(steps), fp64=True)
        ok = dist[0] > 1e-5
        assert (got[b].numpy()[ok] == tok[0][ok]).all()
    assert _sample(xd, 0, banned=bd).tolist() == [int(max(keep, key=lambda i: (float(x[b, i]), -i))) for b in range(B)]
    # an all-banned row emits pad_id and leaves its done flag alone; so does a row of -inf / NaN
    allb = torch.ones(V, dtype=torch.uint8, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    eos = torch.tensor([PAD, 77], dtype=torch.int32, device="cuda")  # even with pad_id among the EOS ids
    out = torch.full((B, 3), -1, dtype=torch.int64, device="cuda")
    for ds in (0, 1):
        assert _sample(xd, ds, banned=allb, done=done, eos=eos, out=out, step=1, pad=PAD).tolist() == [PAD] * B
        assert done.tolist() == [0] * B and out[:, 1].tolist() == [PAD] * B
    y = x.clone()
    y[0] = float("-inf")
    y[1] = float("nan")
    y[2, ::2] = float("nan")
    y[3, 1::2] = float("-inf")
    y[:, 9] = float("-inf")  # the pad id of this part: never a candidate, so only the fallback emits it
    yd = y.cuda()
    eos9 = torch.tensor([9], dtype=torch.int32, device="cuda")
    for ds in (0, 1):
        got = torch.stack([_sample(yd, ds, 256, 1.3, 1.0, step=s, done=done, eos=eos9, pad=9) for s in range(8)], 1)
        assert (got[:2] == 9).all() and done.tolist() == [0] * B
        assert (got[2] % 2 == 1).all() and (got[3] % 2 == 0).all()  # -inf and NaN logits are never drawn
    # an all-equal row with k 25 draws only ids 0 .. 24 (every one of them over 256 draws), greedy takes id 0
    eq = torch.full((B, V), 0.25, device="cuda")
    got = torch.stack([_sample(eq, 1, 25, 0.8, 1.0, step=s) for s in range(64)], 1)
    assert set(got.flatten().tolist()) == set(range(25))
    assert _sample(eq, 0).tolist() == [0] * B
    z = torch.zeros(B, V)
    z[:, ::3] = -0.0  # -0 ties with +0
    assert _sample(z.cuda(), 0).tolist() == [0] * B


@pytest.mark.parametrize("V", [502, 152167])
def test_independent_of_batch_position_and_history(V):
    x, xd, _ = _case(V, 64) if V == 502 else _case(152576, 64)
    x, xd = x[:, :V].contiguous(), xd[:, :V].contiguous()  # odd V: rows after the first are only 4-byte aligned
    kw = dict(do_sample=1, top_k=25, temperature=0.8, top_p=0.9)
    full = _sample(xd, step=5, **kw)
    assert torch.equal(_sample(xd, step=5, **kw), full)  # a repeated call
    for b in (0, 1, 37, 63):
        ids = torch.tensor([b], dtype=torch.int64, device="cuda")
        assert int(_sample(xd[b:b + 1].contiguous(), step=5, row_ids=ids, **kw)) == int(full[b]), b  # alone
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1))
    got = _sample(xd[perm.cuda()].contiguous(), step=5, row_ids=perm.cuda(), **kw)  # at another position of the batch
    assert torch.equal(got, full[perm])
    part = _sample(xd[10:30].contiguous(), step=5, row_ids=torch.arange(10, 30, device="cuda"), **kw)  # in another batch size
    assert torch.equal(part, full[10:30])
    # seed, step and row id each enter the draw
    assert not torch.equal(_sample(xd, step=5, seed=SEED + 1, **kw), full)
    assert not torch.equal(_sample(xd, step=5, seed=SEED + (1 << 32), **kw), full)
    assert not torch.equal(_sample(xd, step=6, **kw), full)
    assert not torch.equal(_sample(xd, step=5, row_ids=torch.arange(64, 128, device="cuda"), **kw), full)
    assert not torch.equal(_sample(xd, step=5, row_ids=torch.arange(64, device="cuda") + (1 << 32), **kw), full)


@pytest.mark.parametrize("V", [502, 4099])
def test_eos_done_pad_and_out(V):
    B = 8
    _, xd, ranked = _case(V, 8)
    greedy = [int(r[0]) for r in ranked]
    eos = torch.tensor([greedy[2], greedy[5], V + 5], dtype=torch.int32, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 7), -1, dtype=torch.int64, device="cuda")
    n0 = _sample(xd, 0, eos=eos, done=done, out=out, step=3, pad=1)
    assert n0.tolist() == greedy and out[:, 3].tolist() == greedy  # out[b * stride + step] and next[b] agree
    assert (out[:, :3] == -1).all() and (out[:, 4:] == -1).all()
    want_done = [int(g in (greedy[2], greedy[5])) for g in greedy]
    assert done.tolist() == want_done
    n1 = _sample(xd, 1, eos=eos, done=done, out=out, step=4, pad=1)  # finished rows emit pad_id from now on
    for b in range(B):
        if want_done[b]:
            assert int(n1[b]) == 1 and int(out[b, 4]) == 1
        else:
            assert int(n1[b]) == int(out[b, 4]) and int(n1[b]) in ranked[b][:25].tolist()
    # a view of a wider buffer: the stride is the buffer's
    wide = torch.full((B, 20), -1, dtype=torch.int64, device="cuda")
    view = wide[:, 4:10]
    n2 = _sample(xd, 0, out=view, step=2)
    assert wide[:, 6].tolist() == n2.tolist() == greedy and int((wide != -1).sum()) == B
    # done = NULL and out = NULL are accepted (with and without EOS ids)
    assert _sample(xd, 0, eos=eos).tolist() == greedy
    assert _sample(xd, 0).tolist() == greedy


# ---- model level ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _model(tag):
    from tests.test_gpu_generate import _mk, _tiny, _wide
    cfg, sd = _tiny() if tag == "tiny" else _wide()
    return cfg, _mk(cfg, sd, max_tokens=512)


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_generate_engine_greedy_equals_torch_greedy(tag, gold):
    _, m = _model(tag)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    kw = dict(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(),
              max_new_tokens=int(gold["max_new_tokens"]), eos_token_id=int(gold[f"{tag}_eos"]), pad_token_id=0)
    want = m.generate(**kw).cpu()
    got = m.generate(sampler="engine", **kw).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, want)
    new = want[:, ids.shape[1]:]
    hit = (new == int(gold[f"{tag}_eos"]))
    assert hit.any() and (new[hit.cumsum(1) - hit.long() > 0] == 0).all()  # the golden case has a row that ends mid-way


def _sampling_inputs(cfg):
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, cfg.vocab, (4, 16), generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0
    am[3, :11] = 0
    return ids, am


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_generate_engine_sampling(tag):
    cfg, m = _model(tag)
    ids, am = _sampling_inputs(cfg)
    first = m(input_ids=ids[:1]).logits[0, -1].float()
    bad = [[int(t)] for t in first.topk(3).indices]
    sample_ids = torch.tensor([40, 3, 1 << 33, 7])
    kw = dict(bad_words_ids=bad, do_sample=True, temperature=0.8, top_k=25, max_new_tokens=24, eos_token_id=[], seed=11,
              sampler="engine")
    a = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, **kw).cpu()
    b = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, **kw).cpu()
    assert torch.equal(a, b)  # the same seed twice
    new = a[:, 16:]
    assert new.shape == (4, 24)
    assert not torch.isin(new, torch.tensor([w[0] for w in bad])).any()
    c = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, **{**kw, "seed": 12}).cpu()
    assert not torch.equal(a, c)
    # a left-padded batch of 4 equals each row generated alone with its sample_ids entry
    for r in range(4):
        alone = m.generate(input_ids=ids[r:r + 1][:, am[r].bool()], sample_ids=sample_ids[r:r + 1], **kw).cpu()
        assert torch.equal(alone[0, -24:], new[r]), r
    # every token within the top 25 of its step (teacher-forced logits of the compacted rows, bad words removed)
    for r in range(4):
        row = torch.cat([ids[r][am[r].bool()], new[r]])[None]
        lg = m(input_ids=row).logits[0].float().cpu()
        n0 = int(am[r].sum())
        for k in range(new.shape[1]):
            s = lg[n0 - 1 + k].clone()
            s[[w[0] for w in bad]] = float("-inf")
            kth = s.topk(25).values[-1]
            assert s[new[r, k]] >= kth - 0.05 * float(s[torch.isfinite(s)].pow(2).mean().sqrt()), (r, k)


def test_generate_engine_eos_and_trim():
    cfg, m = _model("tiny")
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, cfg.vocab, (3, 12), generator=g)
    ref = m.generate(ids, max_new_tokens=6, eos_token_id=[], sampler="engine").cpu()
    assert torch.equal(ref, m.generate(ids, max_new_tokens=6, eos_token_id=[]).cpu())
    eos = [int(ref[b, 12 + 1]) for b in range(3)]  # every row has emitted one of these by step 1
    out = m.generate(input_ids=ids, max_new_tokens=30, eos_token_id=eos, pad_token_id=0, sampler="engine").cpu()
    assert torch.equal(out, m.generate(input_ids=ids, max_new_tokens=30, eos_token_id=eos, pad_token_id=0).cpu())
    assert out.shape[1] <= 12 + 2


def test_generate_engine_limits_and_torch_default():
    cfg, m = _model("tiny")
    ids, am = _sampling_inputs(cfg)
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=4)
    with pytest.raises(ValueError, match="top_k"):
        m.generate(sampler="engine", do_sample=True, top_k=0, **kw)
    with pytest.raises(ValueError, match="256"):
        m.generate(sampler="engine", do_sample=True, top_k=300, **kw)
    with pytest.raises(ValueError, match="16 EOS"):
        m.generate(sampler="engine", eos_token_id=list(range(2, 19)), **kw)
    with pytest.raises(ValueError, match="temperature"):
        m.generate(sampler="engine", do_sample=True, top_k=25, temperature=0.0, **kw)
    with pytest.raises(ValueError, match="sampler"):
        m.generate(sampler="device", **kw)
    with pytest.raises(ValueError, match="sample_ids"):
        m.generate(sample_ids=torch.arange(4), **kw)
    with pytest.raises(ValueError, match="sample_ids"):
        m.generate(sampler="engine", sample_ids=torch.arange(3), **kw)
    m.generate(sampler="engine", eos_token_id=list(range(2, 18)), **kw)  # 16 EOS ids are fine
    skw = dict(do_sample=True, temperature=0.8, top_k=25, top_p=0.9, eos_token_id=[], seed=11, **{**kw, "max_new_tokens": 12})
    assert torch.equal(m.generate(sampler="torch", **skw), m.generate(**skw))
    assert torch.equal(m.generate(sampler=None, **skw), m.generate(**skw))
    # seed=None: a fresh seed from torch's default CPU generator, so seeding that generator repeats the run
    torch.manual_seed(123)
    a = m.generate(sampler="engine", **{**skw, "seed": None})
    torch.manual_seed(123)
    assert torch.equal(a, m.generate(sampler="engine", **{**skw, "seed": None}))
