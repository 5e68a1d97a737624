"""-m gpu: KV-cached generation (slam_prefill / slam_decode_step / UnitLM.generate) and its two kernels.

Kernels through the single-op entries against torch fp32; teacher-forced decode logits against one full forward and the fp32
oracle (logits rel-RMS <= 2e-2, the model tolerance of test_gpu_model.py); greedy generation against HuggingFace's own
`generate` (tests/golden/generate.npz, make_golden_generate.py) up to the first step whose golden top-1 / top-2 margin is within
that tolerance; sampling, batch independence and the capacity checks."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests.gpu_util import lib, ptr, rel_err, stream, sync

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate.npz")
LOGITS_TOL = 2e-2


def _mk(cfg: O.OracleConfig, sd, max_tokens=4096, seed=0):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base = dict(num_hidden_layers=cfg.n_layers, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads,
                num_key_value_heads=cfg.n_kv_heads, head_dim=cfg.head_dim, intermediate_size=cfg.intermediate,
                rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, tie_word_embeddings=True)
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=max_tokens),
               allocate_grads=False, seed=seed)
    if sd is not None:
        m.load_state_dict(sd)
    return m


# ---- kernels --------------------------------------------------------------------------------------------------------------
SLAM = dict(H=896, I=4864, QKV=1152, HD=896, V=502)
CFG3 = dict(H=1536, I=8960, QKV=2048, HD=1536, V=152576)


def _shapes(c):
    return [(c["QKV"], c["H"]), (c["H"], c["HD"]), (2 * c["I"], c["H"]), (c["H"], c["I"]), (c["V"], c["H"])]


def _skinny(X, W, bias, resid, f32):
    M, K = X.shape
    N = W.shape[0]
    Y = torch.empty(M, N, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda")
    nws = lib().slam_op_gemm_skinny_workspace(M, N, K)
    ws = torch.empty(max(nws // 4, 1), dtype=torch.float32, device="cuda")
    rc = lib().slam_op_gemm_skinny(ptr(X), ptr(W), ptr(Y), int(f32), ptr(bias), ptr(resid), M, N, K, ptr(ws), nws, stream())
    assert rc == 0
    sync()
    return Y


@pytest.mark.parametrize("dims", [SLAM, CFG3], ids=["slam358m", "configs3"])
def test_gemm_skinny_vs_torch(dims):
    g = torch.Generator(device="cuda").manual_seed(1)
    for N, K in _shapes(dims):
        W = (torch.randn(N, K, device="cuda", generator=g) * 0.03).to(torch.bfloat16)
        bias = (torch.randn(N, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
        for M in (1, 3, 8, 16, 64):
            X = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
            resid = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
            ref = X.float() @ W.float().t()
            for use_bias, use_res in ((False, False), (True, False), (True, True)):
                r = ref + (bias.float() if use_bias else 0) + (resid.float() if use_res else 0)
                b, rs = (bias if use_bias else None), (resid if use_res else None)
                for f32 in (False, True):
                    Y = _skinny(X, W, b, rs, f32)
                    e = rel_err(Y.float(), r)
                    assert e <= (1e-5 if f32 else 5e-3), (N, K, M, use_bias, use_res, f32, e)
                    Y2 = _skinny(X, W, b, rs, f32)
                    assert torch.equal(Y.view(torch.int16) if not f32 else Y.view(torch.int32),
                                       Y2.view(torch.int16) if not f32 else Y2.view(torch.int32)), "not bit-identical"
            del resid


def _rope_ref(x, pos, hd, theta):
    cos, sin = O.rope_cos_sin(pos.view(1, -1).cpu(), hd, theta)
    cos, sin = cos[0].to(x.device), sin[0].to(x.device)  # [B, hd]
    return x * cos[:, None] + O.rotate_half(x) * sin[:, None]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("heads", [(14, 2), (12, 2), (4, 2)], ids=["14-2", "12-2", "4-2"])
def test_attn_decode_vs_torch(hd, heads):
    nH, nKV = heads
    G = nH // nKV
    theta = 10000.0 if hd == 64 else 1e6
    QKV = (nH + 2 * nKV) * hd
    qscale = 1.0 / math.sqrt(hd) * 1.4426950408889634
    gen = torch.Generator(device="cuda").manual_seed(hd + nH)
    for nk in (1, 63, 64, 65, 1023, 2048, 8192):
        B = 2
        lens = torch.tensor([nk - 1, max(nk - 1 - 7, 0)], dtype=torch.int32, device="cuda")
        cap = -(-nk // 64) * 64 + 64
        kc = (torch.randn(B, nKV, cap, hd, device="cuda", generator=gen)).to(torch.bfloat16)
        vc = (torch.randn(B, nKV, cap, hd, device="cuda", generator=gen)).to(torch.bfloat16)
        qkv = torch.randn(B, QKV, device="cuda", generator=gen) * 2
        bias = (torch.randn(QKV, device="cuda", generator=gen) * 0.5).to(torch.bfloat16)
        kc0, vc0 = kc.clone(), vc.clone()
        o = torch.empty(B, nH * hd, dtype=torch.bfloat16, device="cuda")
        nws = lib().slam_op_attn_decode_workspace(B, nH, nKV, hd, nk)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

        def run():
            kc.copy_(kc0)
            vc.copy_(vc0)
            rc = lib().slam_op_attn_decode(ptr(qkv), ptr(bias), ptr(lens), ptr(kc), ptr(vc), ptr(o), ptr(ws), nws, B, nH, nKV,
                                           hd, cap, nk, theta, stream())
            assert rc == 0
            sync()
            return o.clone(), kc.clone(), vc.clone()

        o1, k1, v1 = run()
        o2, k2, v2 = run()
        assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(k1.view(torch.int16), k2.view(torch.int16))
        x = (qkv + bias.float()).view(B, nH + 2 * nKV, hd)
        pos = lens.long()
        q = (_rope_ref(x[:, :nH], pos, hd, theta) * qscale).to(torch.bfloat16).float()
        k_new = _rope_ref(x[:, nH:nH + nKV], pos, hd, theta).to(torch.bfloat16)
        v_new = x[:, nH + nKV:].to(torch.bfloat16)
        for b in range(B):
            p = int(lens[b])
            # the appended rows: the reference's rotated K (within one bf16 rounding of the table) and V (exact)
            assert rel_err(k1[b, :, p].float(), k_new[b].float()) <= 4e-3, (nk, b)
            assert torch.equal(v1[b, :, p], v_new[b]), (nk, b)
            assert torch.equal(k1[b, :, :p], kc0[b, :, :p]) and torch.equal(k1[b, :, p + 1:], kc0[b, :, p + 1:])
            K = torch.cat([kc0[b, :, :p].float(), k_new[b][:, None].float()], 1)  # [nKV, p+1, hd]
            Vv = torch.cat([vc0[b, :, :p].float(), v_new[b][:, None].float()], 1)
            Kh, Vh = K.repeat_interleave(G, 0), Vv.repeat_interleave(G, 0)
            s = torch.einsum("hd,hjd->hj", q[b], Kh)  # log2 domain
            pr = torch.exp2(s - s.max(-1, keepdim=True).values)
            ref = torch.einsum("hj,hjd->hd", pr, Vh) / pr.sum(-1, keepdim=True)
            e = rel_err(o1[b].view(nH, hd).float(), ref)
            assert e <= 1e-2, (nk, hd, heads, b, e)


# ---- model-level ------------------------------------------------------------------------------------------------------------
def _tiny():
    import json
    meta = json.load(open(os.path.join(os.path.dirname(GOLDEN), "data.json")))["meta"]
    cfg = O.OracleConfig(**meta["config"])
    return cfg, O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"])


def _wide():
    from tests.conftest import load_wide_golden
    _, wcfg, seed, bias_std, jit = load_wide_golden()
    cfg = O.OracleConfig(**wcfg)
    return cfg, O.init_weights(cfg, seed=seed, bias_std=bias_std, norm_jitter=jit)


def _slam():
    return O.SLAM_358M, None  # random init inside the engine (the state dict is read back for the oracle)


@pytest.mark.parametrize("which", ["tiny", "wide", "slam358m"])
def test_teacher_forced_decode_matches_forward_and_oracle(which):
    cfg, sd = {"tiny": _tiny, "wide": _wide, "slam358m": _slam}[which]()
    m = _mk(cfg, sd, max_tokens=1024, seed=7)
    sd_bf = {k: v.float() for k, v in m.state_dict(torch.bfloat16).items()}
    g = torch.Generator().manual_seed(3)
    lens = [37, 20, 5]
    NEW = 40
    B, T = len(lens), max(lens)
    rows = [[1] + torch.randint(2, cfg.vocab, (n - 1,), generator=g).tolist() for n in lens]
    given = torch.randint(2, cfg.vocab, (B, NEW), generator=g)
    ids = torch.zeros(B, T, dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.tensor(r)
    dev = m.device
    ids_d = ids.to(dev).contiguous()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    cap = -(-(T + NEW) // 64) * 64
    nb = m.engine.kv_cache_bytes(B, cap)
    cache = torch.empty(nb, dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    logits = torch.empty(B, cfg.vocab, dtype=torch.float32, device=dev)
    steps = []
    m.engine.prefill(ids_d, lens_d, B, T, logits)
    steps.append(logits.clone())
    given_d = given.to(dev)
    for k in range(NEW - 1):
        m.engine.decode_step(given_d[:, k].contiguous(), lens_d, B, logits)
        steps.append(logits.clone())
    sync()
    assert lens_d.tolist() == [n + NEW - 1 for n in lens]
    dec = torch.stack(steps, 1).cpu()  # [B, NEW, V]: step k predicts the token after prompt + given[:k]
    full = torch.zeros(B, T + NEW, dtype=torch.long)
    for b, r in enumerate(rows):
        full[b, :len(r)] = torch.tensor(r)
        full[b, len(r):len(r) + NEW] = given[b]
    fwd = m(input_ids=full).logits.float().cpu()
    ref = O.model_forward(cfg, sd_bf, full) if which != "slam358m" else None
    for b, n in enumerate(lens):
        f = fwd[b, n - 1:n - 1 + NEW]
        e = rel_err(dec[b], f)
        assert e <= LOGITS_TOL, (which, b, "decode vs forward", e)
        if ref is not None:
            e2 = rel_err(dec[b], ref[b, n - 1:n - 1 + NEW])
            assert e2 <= LOGITS_TOL, (which, b, "decode vs oracle", e2)
    if which == "slam358m":  # the fp32 oracle on the 24-layer body: the shortest row only (CPU time)
        b = 2
        n = lens[b]
        ref = O.model_forward(cfg, sd_bf, full[b:b + 1, :n + NEW])
        e2 = rel_err(dec[b], ref[0, n - 1:n - 1 + NEW])
        assert e2 <= LOGITS_TOL, ("slam358m decode vs oracle", e2)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_generate_matches_hf_golden(tag, gold):
    cfg, sd = _tiny() if tag == "tiny" else _wide()
    m = _mk(cfg, sd, max_tokens=512)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    want = torch.from_numpy(gold[f"{tag}_seq"])
    margin = torch.from_numpy(gold[f"{tag}_margin"])
    eos = int(gold[f"{tag}_eos"])
    bad = gold["bad_words"].tolist()
    out = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=bad, max_new_tokens=int(gold["max_new_tokens"]),
                     eos_token_id=eos, pad_token_id=0).cpu()
    assert out.dtype == torch.int64 and out.shape == want.shape, (out.shape, want.shape)
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids)  # the prompt exactly as passed, left padding included
    tol = 2 * LOGITS_TOL * float(gold[f"{tag}_score_rms"])
    new, wnew = out[:, T:], want[:, T:]
    matched = total = 0
    for b in range(want.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else wnew.shape[1]  # steps before the first near-tie must agree exactly
        diff = (new[b] != wnew[b]).nonzero()
        first = int(diff[0]) if len(diff) else wnew.shape[1]
        assert first >= trust, (tag, b, "diverged at", first, "before the first near-tie", trust)
        hit = (wnew[b] == eos).nonzero()
        length = int(hit[0]) + 1 if len(hit) else wnew.shape[1]
        matched += min(first, length)
        total += length
        if len(hit) and first >= length:  # finished row: EOS then pad only
            assert (new[b, length:] == 0).all()
    assert matched >= 0.75 * total, (tag, matched, total)


def test_generate_eos_pad_and_early_stop():
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=512)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, cfg.vocab, (3, 12), generator=g)
    ref = m.generate(ids, max_new_tokens=6, eos_token_id=[]).cpu()  # positional form
    assert ref.shape == (3, 18)
    eos = [int(ref[b, 12 + 1]) for b in range(3)]  # every row has emitted one of these by step 1
    out = m.generate(input_ids=ids, max_new_tokens=30, eos_token_id=eos, pad_token_id=0).cpu()
    new = out[:, 12:]
    fin = torch.isin(new, torch.tensor(eos)).cumsum(1) > 0
    assert fin[:, -1].all() and not fin[:, -2].all() if new.shape[1] > 1 else fin.all()
    assert new.shape[1] <= 2
    for b in range(3):
        k = int(torch.isin(new[b], torch.tensor(eos)).nonzero()[0])
        assert torch.equal(new[b, :k + 1], ref[b, 12:12 + k + 1]) and (new[b, k + 1:] == 0).all()


def test_generate_sampling():
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=512)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, cfg.vocab, (4, 16), generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0
    am[3, :11] = 0
    first = m(input_ids=ids[:1]).logits[0, -1].float()
    bad = [[int(t)] for t in first.topk(3).indices]
    kw = dict(input_ids=ids, attention_mask=am, bad_words_ids=bad, do_sample=True, temperature=0.8, top_k=25,
              max_new_tokens=24, eos_token_id=[], seed=11)
    a = m.generate(**kw).cpu()
    b = m.generate(**kw).cpu()
    assert torch.equal(a, b)
    new = a[:, 16:]
    assert not torch.isin(new, torch.tensor([w[0] for w in bad])).any()
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


def test_generate_batch_independence():
    cfg, sd = _wide()
    m = _mk(cfg, sd, max_tokens=512)
    g = torch.Generator().manual_seed(13)
    lens = [9, 30, 17]
    T = max(lens)
    ids = torch.zeros(3, T, dtype=torch.long)
    am = torch.zeros(3, T, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, T - n:] = torch.randint(2, cfg.vocab, (n,), generator=g)
        am[b, T - n:] = 1
    batch = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=20, eos_token_id=[]).cpu()
    for b, n in enumerate(lens):
        alone = m.generate(input_ids=ids[b:b + 1, T - n:], max_new_tokens=20, eos_token_id=[]).cpu()
        assert torch.equal(alone[0, n:], batch[b, T:]), b


def test_capacity_and_state_checks():
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=256)
    ids = torch.randint(2, cfg.vocab, (2, 200))
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, max_new_tokens=57)
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, max_new_tokens=4, num_beams=2)
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, max_new_tokens=4, repetition_penalty=1.3)
    # engine: a step past the bound capacity is refused (host-side bound, before any launch)
    dev = m.device
    cache = torch.empty(m.engine.kv_cache_bytes(2, 64), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, 2, 64)
    ids_d = torch.randint(2, cfg.vocab, (2, 60), device=dev)
    lens = torch.tensor([60, 41], dtype=torch.int32, device=dev)
    logits = torch.empty(2, cfg.vocab, dtype=torch.float32, device=dev)
    m.engine.prefill(ids_d, lens, 2, 60, logits)
    tok = torch.ones(2, dtype=torch.long, device=dev)
    for _ in range(4):
        m.engine.decode_step(tok, lens, 2, logits)
    with pytest.raises(E.EngineError):
        m.engine.decode_step(tok, lens, 2, logits)
    sync()
    assert lens.tolist() == [64, 45]
