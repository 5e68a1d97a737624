"""-m gpu: k tokens per row appended to a live KV cache (slam_op_attn_extend, slam_extend) and generate(prefill_chunk=).

The attention op against torch fp32 built from the same bf16 q|k|v and cache, exp2-domain softmax as in
test_attn_decode_vs_torch and with its bound (rel-RMS <= 1e-2), on a cache poisoned with a bf16 NaN pattern (the poison is
data: nothing is read out of bounds): the appended rows bit-equal to the chunk's K / V columns, every other cache row
bit-unchanged, padded rows of the output exactly zero, two runs bit-identical. Every shape runs twice: with the workspace the
op asks for (key splits + combine where the launch takes more than one) and with none (one split, direct store).

slam_extend against one full forward and the fp32 oracle at the matching positions (logits rel-RMS <= LOGITS_TOL = 2e-2, the
model tolerance), inert rows bit-unchanged; the cache fan-out behind a chunked prefill; generate(prefill_chunk=32) against
HuggingFace's own generate (tests/golden/generate.npz) by the near-tie rule of test_generate_matches_hf_golden."""
import math

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests.gpu_util import lib, ptr, rel_err, stream, sync
from tests.test_gpu_generate import GOLDEN, LOGITS_TOL, _mk, _tiny, _wide

pytestmark = pytest.mark.gpu

POISON = 0x7FC1  # a bf16 NaN
OP_TOL = 1e-2    # test_attn_decode_vs_torch's bound


def _i16(t):
    return t.view(torch.int16)


def _op_case(hd, nH, nKV, T, base, new, cap, seed):
    """One launch over B = len(base) rows. Returns (o, k, v) of the run with the op's workspace after checking it against the
    reference, the cache contract, the run without a workspace and a second run."""
    B, G = len(base), nH // nKV
    QKV = (nH + 2 * nKV) * hd
    qscale = 1.0 / math.sqrt(hd) * 1.4426950408889634
    gen = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(B * T, QKV, device="cuda", generator=gen)
    qkv[:, :nH * hd] *= 2 * qscale  # queries as the forward stores them: pre-scaled
    qkv = qkv.to(torch.bfloat16)
    kc0 = torch.full((B, nKV, cap, hd), POISON, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    vc0 = kc0.clone()
    for b in range(B):
        kc0[b, :, :base[b]] = torch.randn(nKV, base[b], hd, device="cuda", generator=gen).to(torch.bfloat16)
        vc0[b, :, :base[b]] = torch.randn(nKV, base[b], hd, device="cuda", generator=gen).to(torch.bfloat16)
    base_d = torch.tensor(base, dtype=torch.int32, device="cuda")
    new_d = torch.tensor(new, dtype=torch.int32, device="cuda")
    bound = max(b_ + n_ for b_, n_ in zip(base, new))  # the tightest host bound the contract allows
    assert 0 < bound <= cap
    nws = lib().slam_op_attn_extend_workspace(B, T, nH, nKV, hd, bound)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device="cuda")
    kc, vc = kc0.clone(), vc0.clone()
    o = torch.empty(B * T, nH * hd, dtype=torch.bfloat16, device="cuda")

    def run(with_ws):
        kc.copy_(kc0)
        vc.copy_(vc0)
        _i16(o).fill_(POISON)
        rc = lib().slam_op_attn_extend(ptr(qkv), ptr(base_d), ptr(new_d), ptr(kc), ptr(vc), ptr(o), ptr(ws) if with_ws else None,
                                       nws if with_ws else 0, B, T, nH, nKV, hd, cap, bound, stream())
        assert rc == 0, rc
        sync()
        return o.clone(), kc.clone(), vc.clone()

    o1, k1, v1 = run(True)
    o2, k2, v2 = run(True)
    assert torch.equal(_i16(o1), _i16(o2)) and torch.equal(_i16(k1), _i16(k2)) and torch.equal(_i16(v1), _i16(v2)), "not bit-identical"
    o3, k3, v3 = run(False)
    assert torch.equal(_i16(k3), _i16(k1)) and torch.equal(_i16(v3), _i16(v1))
    x = qkv.view(B, T, nH + 2 * nKV, hd)
    tag = (hd, nH, nKV, T, tuple(base), tuple(new))
    for b in range(B):
        p, n = base[b], new[b]
        k_new = x[b, :n, nH:nH + nKV].transpose(0, 1)  # [nKV, n, hd]
        v_new = x[b, :n, nH + nKV:].transpose(0, 1)
        # the cache: appended rows bit-equal to the chunk's columns, everything else (poison included) bit-unchanged
        assert torch.equal(_i16(k1[b, :, p:p + n]), _i16(k_new)) and torch.equal(_i16(v1[b, :, p:p + n]), _i16(v_new)), (tag, b)
        assert torch.equal(_i16(k1[b, :, :p]), _i16(kc0[b, :, :p])) and torch.equal(_i16(v1[b, :, :p]), _i16(vc0[b, :, :p])), (tag, b)
        assert torch.equal(_i16(k1[b, :, p + n:]), _i16(kc0[b, :, p + n:])), (tag, b)
        assert torch.equal(_i16(v1[b, :, p + n:]), _i16(vc0[b, :, p + n:])), (tag, b)
        for oo, how in ((o1, "split"), (o3, "one split")):
            got = oo.view(B, T, nH, hd)[b]
            assert (_i16(got[n:]) == 0).all(), (tag, b, how, "padded rows are not zero")
            if n == 0:
                continue
            K = torch.cat([kc0[b, :, :p], k_new], 1).float().repeat_interleave(G, 0)  # [nH, p + n, hd]
            V = torch.cat([vc0[b, :, :p], v_new], 1).float().repeat_interleave(G, 0)
            q = x[b, :n, :nH].float()  # [n, nH, hd]
            s = torch.einsum("thd,hjd->htj", q, K)  # log2 domain
            j = torch.arange(p + n, device="cuda")[None, None, :]
            t = torch.arange(n, device="cuda")[None, :, None]
            s = s.masked_fill(j > p + t, float("-inf"))
            pr = torch.exp2(s - s.max(-1, keepdim=True).values)
            ref = (torch.einsum("htj,hjd->thd", pr, V) / pr.sum(-1).transpose(0, 1)[..., None])
            e = rel_err(got[:n].float(), ref)
            print(f"[attn_extend] {tag} row {b} {how}: rel_rms={e:.3e}")
            assert torch.isfinite(got[:n].float()).all(), (tag, b, how)
            assert e <= OP_TOL, (tag, b, how, e)
    return o1, k1, v1


@pytest.mark.parametrize("T", [1, 16, 17, 48])
@pytest.mark.parametrize("heads", [(14, 2), (12, 2), (4, 2), (2, 2)], ids=["14-2", "12-2", "4-2", "2-2"])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_extend_vs_torch(hd, heads, T):
    nH, nKV = heads
    _op_case(hd, nH, nKV, T, base=[0, 31, 65], new=[T, min(T, 17), 0], cap=128, seed=hd + nH + T)


@pytest.mark.parametrize("new", [1, 15, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_extend_base_edges(hd, new):
    base = [1, 32, 63, 64, 200]
    _op_case(hd, 14, 2, 16, base=base, new=[new] * len(base), cap=256, seed=hd + new)


@pytest.mark.parametrize("hd", [64, 128])
def test_attn_extend_long_base(hd):
    _op_case(hd, 14, 2, 32, base=[2047], new=[17], cap=2112, seed=hd)


# ---- engine -------------------------------------------------------------------------------------------------------------------
def _poisoned_cache(m, cfg, rows, cap):
    nb = m.engine.kv_cache_bytes(rows, cap)
    cache = torch.full((nb // 2,), POISON, dtype=torch.int16, device=m.device)
    m.engine.bind_kv_cache(cache, rows, cap)
    return cache.view(cfg.n_layers, 2, rows, cfg.n_kv_heads, cap, cfg.head_dim)


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_extend_matches_forward_and_oracle(which):
    cfg, sd = _tiny() if which == "tiny" else _wide()
    m = _mk(cfg, sd, max_tokens=1024, seed=7)
    sd_bf = {k: v.float() for k, v in m.state_dict(torch.bfloat16).items()}
    g = torch.Generator().manual_seed(3)
    lens = [37, 20, 5]
    ext = [[16, 0, 3], [1, 7, 0]]
    TE, NDEC = 16, 8
    B, T = len(lens), max(lens)
    total = [lens[b] + ext[0][b] + ext[1][b] + NDEC for b in range(B)]
    full = torch.zeros(B, max(total), dtype=torch.long)
    for b in range(B):
        full[b, 0] = 1
        full[b, 1:total[b]] = torch.randint(2, cfg.vocab, (total[b] - 1,), generator=g)
    dev = m.device
    cap = 128
    kv = _poisoned_cache(m, cfg, B, cap)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    logits = torch.full((B, cfg.vocab), float("nan"), dtype=torch.float32, device=dev)
    ids = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        ids[b, :lens[b]] = full[b, :lens[b]]
    m.engine.prefill(ids.to(dev).contiguous(), lens_d, B, T, logits)
    sync()
    got = [[(lens[b] - 1, logits[b].clone())] for b in range(B)]  # per row: (position, logits row)
    cur = list(lens)
    SENT = 123.25
    for new in ext:
        chunk = torch.zeros(B, TE, dtype=torch.long)
        for b in range(B):
            chunk[b, :new[b]] = full[b, cur[b]:cur[b] + new[b]]
        inert = [b for b in range(B) if new[b] == 0]
        for b in inert:
            logits[b].fill_(SENT)
        kv0 = kv.clone()
        m.engine.extend(chunk.to(dev).contiguous(), torch.tensor(new, dtype=torch.int32, device=dev), lens_d, B, TE, logits)
        sync()
        for b in range(B):
            if new[b] == 0:
                assert (logits[b] == SENT).all(), (which, b, "inert row's logits were written")
                assert int(lens_d[b]) == cur[b]
                assert torch.equal(kv[:, :, b], kv0[:, :, b]), (which, b, "inert row's cache was written")
                continue
            # appended keys only: everything outside [cur, cur + new) keeps its bits, poison included
            assert torch.equal(kv[:, :, b, :, :cur[b]], kv0[:, :, b, :, :cur[b]]), (which, b)
            assert torch.equal(kv[:, :, b, :, cur[b] + new[b]:], kv0[:, :, b, :, cur[b] + new[b]:]), (which, b)
            assert not (kv[:, :, b, :, cur[b]:cur[b] + new[b]] == POISON).all(-1).any(), (which, b)
            cur[b] += new[b]
            got[b].append((cur[b] - 1, logits[b].clone()))
        assert lens_d.tolist() == cur
    for k in range(NDEC):
        tok = torch.tensor([int(full[b, cur[b]]) for b in range(B)], dtype=torch.long, device=dev)
        m.engine.decode_step(tok, lens_d, B, logits)
        sync()
        for b in range(B):
            got[b].append((cur[b], logits[b].clone()))
            cur[b] += 1
    assert lens_d.tolist() == cur == total
    # slam_extend with T = 1 and slam_decode_step on the same state agree
    h = m.engine.h
    tok = torch.arange(7, 7 + B, dtype=torch.long, device=dev)
    kv0, lens0 = kv.clone(), lens_d.clone()
    one = torch.ones(B, dtype=torch.int32, device=dev)
    assert lib().slam_extend(h, ptr(tok), ptr(one), ptr(lens_d), B - 1, 1, ptr(logits), stream()) == -1  # another batch: EINVAL
    la = torch.empty_like(logits)
    m.engine.extend(tok.view(B, 1), one, lens_d, B, 1, la)
    sync()
    assert lens_d.tolist() == [c + 1 for c in cur]
    kv.copy_(kv0)
    lens_d.copy_(lens0)
    lb = torch.empty_like(logits)
    m.engine.decode_step(tok, lens_d, B, lb)
    sync()
    e = rel_err(la, lb)
    print(f"[extend] {which} extend(T=1) vs decode_step: rel_rms={e:.3e}")
    assert e <= LOGITS_TOL, (which, "extend T=1 vs decode_step", e)
    # the full forward and the oracle at the matching positions
    fwd = m(input_ids=full).logits.float().cpu()
    ref = O.model_forward(cfg, sd_bf, full)
    for b in range(B):
        pos = [p for p, _ in got[b]]
        rows = torch.stack([r for _, r in got[b]]).cpu()
        assert torch.isfinite(rows).all()
        e1, e2 = rel_err(rows, fwd[b, pos]), rel_err(rows, ref[b, pos])
        print(f"[extend] {which} row {b}: {len(pos)} logits rows, vs forward {e1:.3e}, vs oracle {e2:.3e}")
        assert e1 <= LOGITS_TOL, (which, b, "vs forward", e1)
        assert e2 <= LOGITS_TOL, (which, b, "vs oracle", e2)
        # the rows the two extends produced, on their own
        for i in range(1, len(pos) - NDEC):
            ee = rel_err(rows[i], ref[b, pos[i]])
            assert ee <= LOGITS_TOL, (which, b, "extend row", i, ee)


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_kv_repeat_behind_chunked_prefill(which):
    cfg, sd = _tiny() if which == "tiny" else _wide()
    m = _mk(cfg, sd, max_tokens=1024)
    lens, n, Cc = [70, 37, 5], 3, 32
    B, T = len(lens), max(lens)
    g = torch.Generator().manual_seed(5)
    ids = torch.zeros(B, T, dtype=torch.long)
    for b, ln in enumerate(lens):
        ids[b, :ln] = torch.randint(2, cfg.vocab, (ln,), generator=g)
    dev = m.device
    rows, cap = B * n + 1, 128  # one row more than needed: it must keep its poison
    kv = _poisoned_cache(m, cfg, rows, cap)
    ids_d = ids.to(dev)
    full = torch.tensor(lens, dtype=torch.int32, device=dev)
    lens_d = torch.zeros(rows, dtype=torch.int32, device=dev)
    lens_d[:B] = full.clamp(max=Cc)
    logits = torch.full((rows, cfg.vocab), float("nan"), dtype=torch.float32, device=dev)
    m.engine.prefill(ids_d[:, :Cc].contiguous(), lens_d, B, Cc, logits)
    for c0 in range(Cc, T, Cc):
        w = min(Cc, T - c0)
        m.engine.extend(ids_d[:, c0:c0 + w].contiguous(), (full - c0).clamp(min=0, max=w).contiguous(), lens_d, B, w, logits)
    sync()
    assert lens_d[:B].tolist() == lens
    # the chunked prefill's last-token logits against the one-shot forward
    fwd = m(input_ids=ids).logits.float().cpu()
    for b, ln in enumerate(lens):
        e = rel_err(logits[b].cpu(), fwd[b, ln - 1])
        assert e <= LOGITS_TOL, (which, b, "chunked prefill vs forward", e)
    kv0, lens0, logits0 = kv.clone(), lens_d.clone(), logits.clone()
    assert (kv0[:, :, B:] == POISON).all()
    m.engine.kv_repeat(n, lens_d, logits)
    sync()
    for b, ln in enumerate(lens):
        for i in range(n):
            r = b * n + i
            assert torch.equal(kv[:, :, r, :, :ln], kv0[:, :, b, :, :ln]), (which, b, i)
            assert int(lens_d[r]) == ln, (which, b, i)
            assert torch.equal(logits[r].view(torch.int32), logits0[b].view(torch.int32)), (which, b, i)
    assert (kv[:, :, B * n] == POISON).all() and int(lens_d[B * n]) == 0 and torch.isnan(logits[B * n]).all()
    assert not torch.isnan(logits[:B * n]).any()
    BN = B * n
    tok = torch.arange(5, 5 + BN, dtype=torch.long, device=dev)
    m.engine.decode_step(tok, lens_d, BN, logits)
    sync()
    assert not torch.isnan(logits[:BN]).any()
    assert lib().slam_kv_repeat(m.engine.h, 1, ptr(lens_d), ptr(logits), stream()) == -2  # after a decode step: ESTATE
    with pytest.raises(E.EngineError):
        m.engine.kv_repeat(n, lens_d, logits)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_generate_chunked_matches_hf_golden(tag, gold):
    cfg, sd = _tiny() if tag == "tiny" else _wide()
    m = _mk(cfg, sd, max_tokens=512)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    want = torch.from_numpy(gold[f"{tag}_seq"])
    margin = torch.from_numpy(gold[f"{tag}_margin"])
    eos = int(gold[f"{tag}_eos"])
    bad = gold["bad_words"].tolist()
    nnew = int(gold["max_new_tokens"])
    kw = dict(input_ids=ids, attention_mask=am, bad_words_ids=bad, max_new_tokens=nnew, eos_token_id=eos, pad_token_id=0)
    out = m.generate(prefill_chunk=32, **kw).cpu()
    assert out.dtype == torch.int64 and out.shape == want.shape, (out.shape, want.shape)
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids)  # the prompt exactly as passed, left padding included
    tol = 2 * LOGITS_TOL * float(gold[f"{tag}_score_rms"])
    new, wnew = out[:, T:], want[:, T:]
    plen = am.sum(1).tolist()
    unchecked = []
    for b in range(want.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else wnew.shape[1]  # steps before the first near-tie must agree exactly
        diff = (new[b] != wnew[b]).nonzero()
        first = int(diff[0]) if len(diff) else wnew.shape[1]
        assert first >= trust, (tag, b, "diverged at", first, "before the first near-tie", trust)
        if trust == 0:
            unchecked.append(b)
        if plen[b] == 70:  # crosses every chunk boundary: all steps are checked
            assert trust == nnew == wnew.shape[1], (tag, b, trust)
        if plen[b] == 37:  # crosses one boundary: its checked first token is its EOS
            assert trust >= 1 and int(wnew[b, 0]) == eos, (tag, b, trust)
    assert sorted(plen) == [1, 5, 37, 70]
    assert unchecked == ([1] if tag == "tiny" else []), (tag, unchecked)  # what the golden alone leaves without a checked step
    # log-probs and the device sampler's n-best with the chunked prefill
    res = m.generate(prefill_chunk=32, return_logprobs=True, **kw)
    assert torch.equal(res.sequences.cpu(), out)
    lp = res.logprobs.cpu()
    assert lp.shape == (ids.shape[0], out.shape[1] - T) and lp.dtype == torch.float32 and torch.isfinite(lp).all()
    assert (lp <= 0).all()
    two = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=6, eos_token_id=[], do_sample=True, top_k=20, temperature=0.9,
                     seed=3, sampler="engine", num_return_sequences=2, prefill_chunk=32).cpu()
    assert two.shape == (2 * ids.shape[0], T + 6)
    assert torch.equal(two[:, :T], ids.repeat_interleave(2, 0))
    assert int(two[:, T:].min()) >= 0 and int(two[:, T:].max()) < cfg.vocab
