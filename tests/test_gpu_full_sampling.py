"""-m gpu: slam_sample_tokens_full (the whole-vocabulary sampler, top_k = 0) against tests/full_sample_ref.py, and
generate(sampler="engine_full").

Both forms: 502 (one block), the switch constant and one more, 6,147 (four chunks, the last of 3 scores, odd: rows are 4-byte
aligned only) and two rows of 152,167. Every (row, step) draw outside the reference's own band (a cut or the draw within
2^-20 Q of flipping; capped at 2 % per case by tests/test_full_sampling_host.py, from the reference alone) must be the
reference's token, with next equal to the out column and no done flag set. Then: EOS / done / pad, rows alone against rows in a
batch, two runs, steps / group / out_col, one statistical check, and the model level."""
import functools

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import full_sample_ref as R

pytestmark = pytest.mark.gpu

SMALL = E.SAMPLE_FULL_SMALL_MAX
CASES = [(502, 5), (SMALL, 5), (SMALL + 1, 5), (6147, 5), (152167, 2)]


@functools.lru_cache(maxsize=None)
def _device(V, B):
    return torch.from_numpy(R.logits(V, B)).cuda(), torch.from_numpy(R.banned(V)).cuda()


def _desc(setting, step=0, n_eos=0, seed=R.SEED):
    do_sample, temperature, top_p, min_p, eps = R.SETTINGS[setting] if isinstance(setting, str) else setting
    return (E.SlamSampleDesc(do_sample=do_sample, top_k=0, temperature=temperature, top_p=top_p, seed=seed, step=step,
                             pad_id=R.PAD, n_eos=n_eos), E.SlamWarpDesc(min_p=min_p, epsilon_cutoff=eps))


def _draws(xd, bn, setting, row_ids, n_steps=R.STEPS, eos=None, seed=R.SEED):
    """Steps 0 .. n_steps - 1, one call each -> (out [B, n_steps], done [B]) on the CPU; next must be the out column."""
    B, V = xd.shape
    ws = torch.full((E.sample_full_workspace_bytes(B, V),), 0xA5, dtype=torch.uint8, device="cuda")  # nothing may rely on zeros
    nxt = torch.empty(B, dtype=torch.int64, device="cuda")
    out = torch.full((B, n_steps), -7, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    desc, warp = _desc(setting, n_eos=0 if eos is None else eos.numel(), seed=seed)
    rid = torch.tensor(row_ids, dtype=torch.int64, device="cuda")
    for s in range(n_steps):
        desc.step = s
        E.sample_tokens_full(xd, desc, nxt, ws, warp, None, 1, None, bn, rid, eos, done, out)
    assert torch.equal(nxt, out[:, n_steps - 1])
    return out.cpu().numpy(), done.cpu().numpy()


@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("V,B", CASES)
def test_tokens_are_the_reference(V, B, setting):
    xd, bn = _device(V, B)
    got, done = _draws(xd, bn, setting, R.ROW_IDS[:B])
    want, near = R.sample_rows(R.logits(V, B), R.banned(V), setting, R.ROW_IDS[:B], range(R.STEPS))
    want = np.where(want < 0, R.PAD, want)  # a row without a score emits pad_id ...
    print(f"V {V} {setting}: {near.mean():.3%} near, {int((got != want).sum())} differ")
    assert not ((got != want) & ~near).any(), (np.argwhere((got != want) & ~near)[:5], got[got != want][:5], want[got != want][:5])
    assert not done.any()                   # ... and is not marked done; no EOS ids were given


@pytest.mark.parametrize("V", [502, 6147])
def test_eos_done_and_pad(V):
    """The draw is stateless, so a run with EOS ids is the run without them cut behind each row's first EOS."""
    xd, bn = _device(V, 5)
    free, _ = _draws(xd, bn, "t1.3", R.ROW_IDS, 16)
    eos = torch.tensor([int(free[0, 3]), int(free[3, 5])], dtype=torch.int32, device="cuda")
    got, done = _draws(xd, bn, "t1.3", R.ROW_IDS, 16, eos=eos)
    hit = np.isin(free, eos.cpu().numpy())
    behind = (np.cumsum(hit, 1) - hit) > 0
    assert np.array_equal(got, np.where(behind, R.PAD, free)) and np.array_equal(done, hit.any(1).astype(np.uint8))


@pytest.mark.parametrize("V,B", [(502, 5), (6147, 5), (152167, 2)])
def test_rows_alone_in_a_batch_and_twice(V, B):
    xd, bn = _device(V, B)
    for setting in ("t1.3", "all"):
        full, _ = _draws(xd, bn, setting, R.ROW_IDS[:B], 8)
        assert np.array_equal(_draws(xd, bn, setting, R.ROW_IDS[:B], 8)[0], full)
        for b in range(B):
            alone, _ = _draws(xd[b:b + 1].contiguous(), bn, setting, R.ROW_IDS[b:b + 1], 8)
            assert np.array_equal(alone[0], full[b]), (setting, b)


@pytest.mark.parametrize("V", [502, 6147])
def test_steps_group_and_out_col(V):
    """Row b = column b % 2 of sequence b // 2 draws what the plain form draws with that row id at steps[q] + step + column."""
    xd, bn = _device(V, 5)
    x4 = xd[[0, 0, 3, 3]].contiguous()
    steps = torch.tensor([4, 9], dtype=torch.int32, device="cuda")
    rid = torch.tensor([R.ROW_IDS[0], R.ROW_IDS[3]], dtype=torch.int64, device="cuda")
    desc, warp = _desc("all", step=1)
    nxt = torch.empty(4, dtype=torch.int64, device="cuda")
    out = torch.full((4, 3), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(E.sample_full_workspace_bytes(4, V), dtype=torch.uint8, device="cuda")
    E.sample_tokens_full(x4, desc, nxt, ws, warp, steps, 2, 2, bn, rid, None, None, out)
    plain, _ = _draws(xd, bn, "all", R.ROW_IDS, 12)
    assert nxt.tolist() == [plain[0, 5], plain[0, 6], plain[3, 10], plain[3, 11]] and torch.equal(out[:, 2], nxt)
    assert (out[:, :2] == -7).all()


def test_draws_follow_the_kept_distribution():
    """4096 draws of the N(0, 3^2) row of 502 under top_p = 0.9 against the exact kept distribution q_i / Q2: the largest
    deviation of a token's count stays inside 5 binomial standard deviations (plus the 0.5 of a count's granularity)."""
    xd, bn = _device(502, 5)
    n = 4096
    got, _ = _draws(xd[:1].contiguous(), bn, "top_p", R.ROW_IDS[:1], n)
    q = R.masses(R.logits(502)[0], R.banned(502), 1.0)
    c, _ = R.cut(q, 0.9, 0.0, 0.0)
    p = np.where(q >= c, q, 0) / float(q[q >= c].sum())
    counts = np.bincount(got[0], minlength=502)
    assert (counts[p == 0] == 0).all()
    assert (np.abs(counts - n * p) <= 5 * np.sqrt(n * p * (1 - p)) + 0.5).all()


def test_generate_engine_full():
    """The golden Qwen2 model: a prompt alone draws what it draws inside a batch of 4 (its sample_ids), two samples per prompt,
    and the log-probs are the replayed log-softmax at the returned tokens within slam_token_logprobs' tolerance."""
    from tests.test_gpu_nbest import _mk, _replay_logprobs, _tiny, logprob_tol
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=512)
    ids = torch.randint(2, cfg.vocab, (4, 128), generator=torch.Generator().manual_seed(5))  # 128: the prefill tiles fall alike
    kw = dict(max_new_tokens=12, do_sample=True, top_k=0, top_p=0.9, temperature=0.9, num_return_sequences=2, return_logprobs=True,
              eos_token_id=[], seed=17, sampler="engine_full")
    batch = m.generate(input_ids=ids, **kw)
    assert batch.sequences.shape == (8, 140) and len(batch.sequences[:, 128:].unique()) > 8
    alone = m.generate(input_ids=ids[2:3], sample_ids=torch.tensor([4, 5]), **kw)
    assert torch.equal(alone.sequences, batch.sequences[4:6]) and torch.equal(alone.logprobs, batch.logprobs[4:6])
    want = _replay_logprobs(m, cfg, ids, torch.ones_like(ids), batch.sequences.cpu(), 2)
    assert float((batch.logprobs.cpu().double() - want.double()).abs().max()) <= logprob_tol()
    g = m.generate(input_ids=ids, max_new_tokens=6, eos_token_id=[], sampler="engine_full")
    assert torch.equal(g, m.generate(input_ids=ids, max_new_tokens=6, eos_token_id=[], sampler="engine"))
