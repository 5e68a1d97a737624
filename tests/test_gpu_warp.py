"""-m gpu: slam_sample_tokens_warped (min_p, typical_p, epsilon_cutoff, eta_cutoff inside the device sampler) and generate's four
arguments under both samplers.

The kernel against the fp64 restatement (tests/warp_ref.py) on the inputs of tests/warp_cases.py: the token must be the
restatement's for every (row, draw) outside the 1e-5 band (the draw's distance from a boundary of the cumulative weights, or the
row's smallest decision margin); a token inside the band must still be one of the row's top-k candidates. How many pairs the band
may excuse is capped on the CPU (tests/test_warp_host.py), from the reference alone. Then: off means slam_sample_tokens_at bit
for bit, row independence and determinism, the corners of the contract, and the model level."""
import functools

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import spec_ref as S
from tests import warp_cases as WC
from tests import warp_ref as W

pytestmark = pytest.mark.gpu

PAD = 0


def _desc(do_sample=1, top_k=25, temperature=WC.TEMPERATURE, top_p=1.0, seed=WC.SEED, step=0, pad=PAD, n_eos=0):
    return E.SlamSampleDesc(do_sample=do_sample, top_k=top_k, temperature=temperature, top_p=top_p, seed=seed, step=step,
                            pad_id=pad, n_eos=n_eos)


@functools.lru_cache(maxsize=None)
def _device(V, B):
    return torch.from_numpy(WC.logits(V, B)).cuda(), torch.from_numpy(WC.banned(V)).cuda()


def _draws(xd, warp, top_k, top_p, n_steps, banned=None, row_ids=None, eos=None, done=None, pad=PAD, temperature=WC.TEMPERATURE):
    """Steps 0 .. n_steps-1 of slam_sample_tokens_warped, one call each, into out [B, n_steps]; returns it on the CPU."""
    B, V = xd.shape
    ws = torch.empty(E.sample_workspace_bytes(B, V, top_k), dtype=torch.uint8, device="cuda")
    nxt = torch.empty(B, dtype=torch.int64, device="cuda")
    out = torch.full((B, n_steps), -7, dtype=torch.int64, device="cuda")
    desc = _desc(top_k=top_k, top_p=top_p, pad=pad, n_eos=0 if eos is None else eos.numel(), temperature=temperature)
    wd = E.SlamWarpDesc(*warp) if warp is not None else None
    for s in range(n_steps):
        desc.step = s
        E.sample_tokens_warped(xd, desc, nxt, ws, wd, None, 1, None, banned, row_ids, eos, done, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("warp", list(WC.WARPS))
@pytest.mark.parametrize("V,B", WC.SHAPES)
def test_kernel_matches_fp64_restatement(V, B, warp):
    xd, bn = _device(V, B)
    ranked = WC.ranked(V, B)
    for k in WC.TOP_K:
        for p in WC.TOP_P:
            got = _draws(xd, WC.WARPS[warp], k, p, WC.STEPS, bn)
            want, band = WC.reference(V, B, warp, k, p)
            bad = (got != want) & ~band
            print(f"V {V} B {B} {warp} k {k} p {p}: {band.mean():.3%} in the band, {int((got != want).sum())} differ there")
            assert not bad.any(), (V, B, warp, k, p, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
            for b, s in np.argwhere(band):  # inside the band: still one of the row's top-k candidates
                assert got[b, s] in ranked[b][:k], (V, B, warp, k, p, b, s)


@pytest.mark.parametrize("V,B,group", [(502, 64, 4), (2049, 3, 3), (152167, 3, 3), (152576, 64, 8)])
def test_off_is_sample_tokens_at(V, B, group):
    """warp = NULL and {0, 1, 0, 0} against slam_sample_tokens_at: next, out and done, with steps, group > 1, EOS ids and a
    finished row in use; greedy ignores a description that is on."""
    xd, bn = _device(V, B)
    ranked = WC.ranked(V, B)
    Q = B // group
    steps = (torch.arange(Q, dtype=torch.int32) * 3 + 1).cuda()
    row_ids = (torch.arange(Q, dtype=torch.int64) * 5 + (1 << 33)).cuda()
    eos = torch.tensor([int(ranked[0][0]), int(ranked[B - 1][1])], dtype=torch.int32, device="cuda")
    ws = torch.empty(E.sample_workspace_bytes(B, V, 25), dtype=torch.uint8, device="cuda")

    def run(fn, do_sample, top_p):
        nxt = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        out = torch.full((B, 5), -7, dtype=torch.int64, device="cuda")
        done = torch.zeros(B, dtype=torch.uint8, device="cuda")
        done[1] = 1
        fn(_desc(do_sample, 25 if do_sample else 1, top_p=top_p, step=2, n_eos=2), nxt, out, done)
        torch.cuda.synchronize()
        return nxt.cpu(), out.cpu(), done.cpu()

    def at(desc, nxt, out, done):
        E.sample_tokens_at(xd, desc, nxt, ws, steps, group, 3, bn, row_ids, eos, done, out)

    def warped(wd):
        return lambda desc, nxt, out, done: E.sample_tokens_warped(xd, desc, nxt, ws, wd, steps, group, 3, bn, row_ids, eos, done,
                                                                   out)

    for do_sample, top_p in ((1, 1.0), (1, 0.9), (0, 1.0)):
        want = run(at, do_sample, top_p)
        assert int(want[0][1]) == PAD and (want[1][:, 3] == want[0]).all()
        for wd in (None, E.SlamWarpDesc(), E.SlamWarpDesc(0.0, 1.0, 0.0, 0.0)):
            got = run(warped(wd), do_sample, top_p)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (V, do_sample, top_p)
    want = run(at, 0, 1.0)
    got = run(warped(E.SlamWarpDesc(*WC.WARPS["all"])), 0, 1.0)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("V,B", [(502, 64), (152576, 64)])
def test_row_independence_and_determinism(V, B):
    xd, bn = _device(V, B)
    for warp in ("typical_p", "all"):
        full = _draws(xd, WC.WARPS[warp], 25, 0.9, 4, bn)
        assert np.array_equal(_draws(xd, WC.WARPS[warp], 25, 0.9, 4, bn), full)  # two runs: identical bits
        for b in (0, 1, 37, 63):
            rid = torch.tensor([b], dtype=torch.int64, device="cuda")
            alone = _draws(xd[b:b + 1].contiguous(), WC.WARPS[warp], 25, 0.9, 4, bn, row_ids=rid)
            assert np.array_equal(alone[0], full[b]), (warp, b)
        part = _draws(xd[10:30].contiguous(), WC.WARPS[warp], 25, 0.9, 4, bn, row_ids=torch.arange(10, 30, device="cuda"))
        assert np.array_equal(part, full[10:30]), warp


@pytest.mark.parametrize("V", [502, 2049])
def test_corners(V):
    """Rows whose outcome is decided exactly (weights 0 or 1), so the fp32 restatement is the kernel's token bit for bit."""
    ninf = float("-inf")
    x = torch.full((7, V), ninf)
    x[0, V - 3] = 1.5                                # 0: one finite score
    #                                                  1: none
    x[2] = 0.25                                      # 2: all equal - every weight, every s and every p ties
    x[3] = torch.randn(V, generator=torch.Generator().manual_seed(3)) * 0.5
    x[3, V - 5] = ninf
    top2 = x[3].topk(2).indices
    x[3, top2] = 10.0                                # 3: a two-way tie far above the rest (min_p = 1, the cutoffs' exemption)
    x[4] = x[3]                                      # 4: the same row, finished before the call
    x[5, V - 5] = 2.0                                # 5: one finite score that is an EOS id
    x[6] = torch.randn(V, generator=torch.Generator().manual_seed(6)) * 3.0  # 6: typical_p on k' = 1 (top_k = 1 below)
    xd = x.cuda()
    eos = torch.tensor([V - 5], dtype=torch.int32, device="cuda")
    n, pad = 16, V - 1
    for warp, k in (((0.0, 0.5, 0.0, 0.0), 25), ((1.0, 1.0, 0.0, 0.0), 25), ((0.0, 1.0, 0.9, 0.0), 25), ((0.0, 1.0, 0.0, 0.9), 25),
                    ((1.0, 0.5, 0.9, 0.9), 256), ((0.0, 0.5, 0.0, 0.0), 1)):
        done = torch.zeros(7, dtype=torch.uint8, device="cuda")
        done[4] = 1
        got = _draws(xd, warp, k, 1.0, n, eos=eos, done=done, pad=pad, temperature=1.0)
        assert (got[0] == V - 3).all() and (got[1] == pad).all() and (got[4] == pad).all(), (warp, k)
        assert got[5, 0] == V - 5 and (got[5, 1:] == pad).all()  # the EOS id survives the chain, sets done, pads follow
        assert done.tolist() == [0, 0, 0, 0, 1, 1, 0], (warp, k)  # the row without a score is not marked done
        for b in (2, 3, 6) if k == 1 else (2, 3):
            want = W.sample_row(x[b].numpy(), None, k, 1.0, 1.0, warp, WC.SEED, [b], np.arange(n))[0]
            assert np.array_equal(got[b], want), (warp, k, b, got[b], want)
        if k == 1:
            assert (got[2] == 0).all() and (got[6] == int(x[6].argmax())).all()
        else:
            assert set(got[2]) <= set(range(k)) and len(set(got[2])) > 4  # all-equal scores: nothing leaves
        if k > 1:  # every setting leaves exactly the two ties at the top, and both are drawn
            assert set(got[3]) == set(top2.tolist()), (warp, got[3])


# ---- model level --------------------------------------------------------------------------------------------------------------
SEED = 11


@functools.lru_cache(maxsize=None)
def _model():
    from tests.test_gpu_generate import _mk, _tiny
    cfg, sd = _tiny()
    return cfg, _mk(cfg, sd, max_tokens=512)


@functools.lru_cache(maxsize=None)
def _draft():
    import dataclasses
    from tests.test_gpu_generate import _mk, _tiny
    cfg, _ = _tiny()
    return _mk(dataclasses.replace(cfg, n_layers=1), None, max_tokens=512, seed=5)


def _case(cfg):
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, cfg.vocab, (4, 16), generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0
    am[3, :11] = 0
    return ids, am, torch.tensor([40, 3, 1 << 33, 7])


WARP_KW = dict(min_p=0.1, typical_p=0.9)
WARP = (0.1, 0.9, 0.0, 0.0)


def test_generate_engine_batch_equals_rows_alone():
    cfg, m = _model()
    ids, am, sample_ids = _case(cfg)
    kw = dict(do_sample=True, temperature=0.8, top_k=25, max_new_tokens=24, eos_token_id=[], seed=SEED, sampler="engine", **WARP_KW)
    a = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, **kw).cpu()
    assert torch.equal(a, m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, **kw).cpu())
    plain = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, **{**kw, "min_p": None, "typical_p": None}).cpu()
    assert not torch.equal(a, plain)  # the warpers do change what is drawn
    for r in range(4):
        alone = m.generate(input_ids=ids[r:r + 1][:, am[r].bool()], sample_ids=sample_ids[r:r + 1], **kw).cpu()
        assert torch.equal(alone[0, -24:], a[r, 16:]), r
    cfgd = __import__("types").SimpleNamespace(**WARP_KW)  # the same values from generation_config
    c = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, generation_config=cfgd,
                   **{k: v for k, v in kw.items() if k not in WARP_KW}).cpu()
    assert torch.equal(a, c)


def _warped_targets(logits_all, n_new, rows, banned, sample_ids):
    """spec_ref.target_tokens with the warper chain: the fp64 restatement of the verify pass, and its 1e-5 exclusions."""
    K1 = logits_all.shape[1]
    tgt = np.zeros((len(rows), K1), np.int64)
    excl = np.zeros((len(rows), K1), bool)
    for i, b in enumerate(rows):
        for j in range(K1):
            tok, dist, margin = W.sample_row(logits_all[b, j], banned, 25, 0.8, 1.0, WARP, SEED, [int(sample_ids[b])],
                                             [int(n_new[b]) + j], fp64=True)
            tgt[i, j] = tok[0, 0]
            excl[i, j] = dist[0, 0] <= 1e-5 or margin <= 1e-5
    return tgt, excl


@pytest.mark.parametrize("mode", ["lookup", "draft"])
def test_generate_proposals_keep_the_targets_own_warped_draws(mode):
    """prompt_lookup_num_tokens=4 and a draft model with the warpers on, by the comparison of test_gpu_lookup.py /
    test_gpu_spec.py: the traced rounds replayed through the restatements (every verified token is the fp64 restatement's warped
    draw from the traced logits, at most 3 % of the draws inside the 1e-5 band, acceptance by spec_ref.accept), the first token -
    drawn from the same prefill logits - equal to the plain engine-sampler call's, and the rest compared with it and printed
    (chunk attention and decode-step attention round differently: a draw at a boundary may differ, as without warpers)."""
    cfg, m = _model()
    ids, am, sample_ids = _case(cfg)
    K, nnew, T = 4, 20, ids.shape[1]
    bad = [[5], [11]]
    kw = dict(bad_words_ids=bad, do_sample=True, temperature=0.8, top_k=25, max_new_tokens=nnew, seed=SEED, sampler="engine",
              pad_token_id=0, **WARP_KW)
    plain = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=[], **kw).cpu()
    eos = [int(plain[1, T + 6]), int(plain[2, T + 13])]
    plain = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=eos, **kw).cpu()
    extra = dict(prompt_lookup_num_tokens=K) if mode == "lookup" else dict(assistant_model=_draft(), num_assistant_tokens=K)
    name = "_lookup_trace" if mode == "lookup" else "_assist_trace"
    trace = []
    setattr(m, name, trace)
    try:
        out = m.generate(input_ids=ids, attention_mask=am, sample_ids=sample_ids, eos_token_id=eos, **extra, **kw).cpu()
    finally:
        setattr(m, name, None)
    new = out[:, T:].numpy()
    B, n = new.shape
    assert torch.equal(out[:, :T], ids) and len(trace) == m.last_assist_stats["rounds"] >= 1
    assert np.array_equal(new[:, 0], plain[:, T].numpy())
    banned = np.zeros(cfg.vocab, np.uint8)
    banned[[w[0] for w in bad]] = 1
    plen = am.sum(1).numpy().astype(np.int32)
    rep = np.zeros((B, nnew), np.int64)
    rep[:, 0] = new[:, 0]
    n_new = np.ones(B, np.int32)
    done = np.isin(new[:, 0], eos).astype(np.uint8)
    draws = excluded = 0
    for r, rec in enumerate(trace):
        chunk, logits_all, n_before, tgt, n_after = (t.numpy() for t in rec[:5])
        assert np.array_equal(n_before, n_new), r
        live = [b for b in range(B) if not done[b]]
        ref, excl = _warped_targets(logits_all, n_new, live, banned, sample_ids.numpy())
        use = tgt.copy()
        for i, b in enumerate(live):
            ok = ~excl[i]
            assert np.array_equal(tgt[b][ok], ref[i][ok]), (mode, r, b, tgt[b], ref[i])
            use[b][ok] = ref[i][ok]
        draws += excl.size
        excluded += int(excl.sum())
        res = S.accept(chunk, use, n_new, done, plen, rep, K, nnew, 0, eos)
        rep, n_new, done = res["out"], res["n_new"], res["done"]
        assert np.array_equal(n_after, n_new), r
    pl = plain[:, T:].numpy()
    same = [bool((new[b, :min(k, pl.shape[1])] == pl[b, :min(k, pl.shape[1])]).all()) for b, k in enumerate(n_new)]
    print(f"[warp] {mode}: {m.last_assist_stats}, tokens per row {n_new.tolist()}, {draws} draws, {excluded} excluded, equal to "
          f"the plain call: {same}")
    assert done.all() and int(n_new.max()) == n
    assert excluded <= 0.03 * draws, (excluded, draws)
    for b in range(B):
        assert np.array_equal(rep[b, :n_new[b]], new[b, :n_new[b]]) and (new[b, n_new[b]:] == 0).all(), (mode, b)


def test_generate_without_the_arguments_is_unchanged():
    """All four absent, None or off: token for token the call that never mentions them, under both samplers, plain and lookup."""
    cfg, m = _model()
    ids, am, sample_ids = _case(cfg)
    off = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    base = dict(input_ids=ids, attention_mask=am, do_sample=True, temperature=0.8, top_k=25, top_p=0.9, max_new_tokens=16,
                eos_token_id=[], seed=SEED)
    for extra in (dict(sampler="engine", sample_ids=sample_ids), dict(sampler=None),
                  dict(sampler="engine", sample_ids=sample_ids, prompt_lookup_num_tokens=4)):
        want = m.generate(**base, **extra).cpu()
        assert torch.equal(m.generate(**base, **extra, **off).cpu(), want)
        assert torch.equal(m.generate(**base, **extra, **{k: None for k in off}).cpu(), want)
    # greedy ignores them
    g = dict(input_ids=ids, attention_mask=am, max_new_tokens=8, eos_token_id=[])
    for sampler in ("engine", None):
        assert torch.equal(m.generate(sampler=sampler, **g).cpu(), m.generate(sampler=sampler, min_p=0.3, typical_p=0.5, **g).cpu())


@pytest.mark.parametrize("top_k", [0, 25])
def test_generate_torch_sampler_is_warp_restated(top_k):
    """sampler=None with a fixed generator seed against the same prefill / decode_step loop driven from here, the tokens drawn
    by torch.multinomial from `_warp`'s scores; top_k = 0 works under this sampler."""
    from slamkit_amd.model.unit_lm import _warp
    cfg, m = _model()
    ids, am, _ = _case(cfg)
    nnew, T = 10, ids.shape[1]
    w = dict(min_p=0.05, typical_p=0.95, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    out = m.generate(input_ids=ids, attention_mask=am, do_sample=True, temperature=0.8, top_k=top_k, top_p=0.9, max_new_tokens=nnew,
                     seed=SEED, eos_token_id=[], pad_token_id=0, **w).cpu()
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
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    new = torch.empty(B, nnew, dtype=torch.int64)
    for s in range(nnew):
        scores = _warp(logits, 0.8, top_k, 0.9, **w)
        nxt = torch.multinomial(torch.softmax(scores, -1), 1, generator=g)[:, 0]
        new[:, s] = nxt.cpu()
        if s + 1 < nnew:
            m.engine.decode_step(nxt.contiguous(), lens, B, logits)
    assert torch.equal(out[:, T:], new)
