"""-m gpu: slam_extend_score / slam_extend_logits in the shared-prompt mode (two-region chunk attention) and
score_continuations(share_prompt_cache=True). Tiny 2-layer models, G = 7, 1, 8 at head_dim 64, G = 6 at 128, and the Qwen3 tiny;
3 prompts of 1, 33 and 65 tokens x n rows; two successive blocks of width T with ragged new_lens. The prompt store and the cache
are filled with a bf16 NaN pattern before the prefill, so a key read beyond a prompt or a row's own keys shows as a non-finite
output. Reference: the full forward over prompt + continuation; bars: LOGITS_TOL for last-token logits, test_gpu_score_model's
_bars rule for log-probs."""
import functools

import pytest
import torch

from oracle import slam_oracle as O
from tests.gpu_util import rel_err, sync
from tests.test_gpu_generate import LOGITS_TOL, _mk, _tiny
from tests.test_gpu_kv_fp8 import _models
from tests.test_gpu_score_model import _bars, _concat, _rms

pytestmark = pytest.mark.gpu

POISON = 0x7FC1  # a bf16 NaN
SHAPES = {"g7": (14, 2, 64), "g1": (4, 4, 64), "g8": (8, 1, 64), "g6hd128": (12, 2, 128)}
PLENS, TP, PCAP, CAP = [1, 33, 65], 65, 128, 64
# real tokens per row in the two blocks (clamped to T): the rows of a prompt leave block 1 with different bases; block 2 has a 0 and a 1
NL1 = [17, 5, 16, 1, 17, 9, 0, 17, 12]
NL2 = [0, 1, 17, 17, 3, 16, 17, 0, 1]


@functools.lru_cache(maxsize=None)
def _model(tag):
    if tag == "qwen3":
        return _models()["qwen3"]()
    nH, nKV, hd = SHAPES[tag]
    cfg = O.OracleConfig(n_layers=2, hidden=256, n_heads=nH, n_kv_heads=nKV, head_dim=hd, intermediate=512)
    return _mk(cfg, O.init_weights(cfg, seed=5, bias_std=0.02, norm_jitter=0.1), max_tokens=1024)


def _poisoned(nbytes):
    return torch.full((nbytes // 2,), POISON, dtype=torch.int16, device="cuda")


def _case(m, n, T, seed=3):
    """Prompts, the rows' continuations cut into two blocks, and the forward's logits over prompt + continuation with the bars."""
    V, B, rows = m.engine.desc.vocab, len(PLENS), len(PLENS) * n
    g = torch.Generator().manual_seed(seed)
    ids, am = torch.zeros(B, TP, dtype=torch.long), torch.zeros(B, TP, dtype=torch.long)
    for b, p in enumerate(PLENS):
        ids[b, :p] = torch.randint(2, V, (p,), generator=g)
        am[b, :p] = 1
    nls = [[min(v, T) for v in pat[:rows]] for pat in (NL1, NL2)]
    clen = [a + b for a, b in zip(*nls)]
    cont = torch.randint(2, V, (rows, 2 * T), generator=g)
    full, _, plen = _concat(ids, am, n, cont, clen)
    bars, lg = _bars(m, full, plen, clen)
    blocks, off = [], [0] * rows
    for nl in nls:
        blk = torch.zeros(rows, T, dtype=torch.long)
        for r in range(rows):
            blk[r, :nl[r]] = cont[r, off[r]:off[r] + nl[r]]
        blocks.append((blk.cuda(), torch.tensor(nl, dtype=torch.int32, device="cuda"), list(off)))
        off = [o + v for o, v in zip(off, nl)]
    return dict(n=n, T=T, B=B, rows=rows, V=V, ids=ids.cuda(), cont=cont, plen=plen, clen=clen, bars=bars, lg=lg, blocks=blocks)


def _run(m, c, shared, logits_all=False):
    """prefill(_prefix) + kv_share / kv_repeat + the two blocks; returns per block (logits, lp | logits_all, argmax) and the buffers."""
    eng, rows, T, V = m.engine, c["rows"], c["T"], c["V"]
    m._ensure_workspace(max(c["B"] * TP, rows * T, 2 * rows))
    lens = torch.zeros(rows, dtype=torch.int32, device="cuda")
    lens[:c["B"]] = torch.tensor(PLENS, dtype=torch.int32)
    logits = torch.full((rows, V), float("nan"), dtype=torch.float32, device="cuda")
    store = store0 = None
    if shared:
        store, cache = _poisoned(eng.kv_prefix_bytes(c["B"], PCAP)), _poisoned(eng.kv_cache_bytes(rows, CAP))
        eng.bind_kv_prefix(store.view(torch.uint8), c["B"], PCAP)
        eng.bind_kv_cache(cache.view(torch.uint8), rows, CAP)
        eng.prefill_prefix(c["ids"], lens, c["B"], TP, logits)
        store0 = store.clone()
        eng.kv_share(c["n"], lens, logits)
    else:
        cache = _poisoned(eng.kv_cache_bytes(rows, PCAP + CAP))
        eng.bind_kv_cache(cache.view(torch.uint8), rows, PCAP + CAP)
        eng.prefill(c["ids"], lens, c["B"], TP, logits)
        eng.kv_repeat(c["n"], lens, logits)
    outs = []
    for blk, nl, _ in c["blocks"]:
        am = torch.full((rows, T), -7, dtype=torch.int64, device="cuda")
        if logits_all:
            res = torch.full((rows, T, V), 7.0, dtype=torch.float32, device="cuda")
            eng.extend_logits(blk, nl, lens, rows, T, res)
        else:
            res = torch.full((rows, T), 7.0, dtype=torch.float32, device="cuda")
            eng.extend_score(blk, nl, lens, rows, T, logits, res, am)
        outs.append((logits.clone(), res.clone(), am.clone()))
    sync()
    if shared:
        eng.bind_kv_prefix(None)
    return outs, lens.tolist(), cache, store, store0


def _check_blocks(c, outs, tag):
    want = torch.log_softmax(c["lg"].double(), -1)
    prev = None
    for k, ((logits, lp, am), (_, nl, off)) in enumerate(zip(outs, c["blocks"])):
        logits, lp, am, nl = logits.cpu(), lp.cpu(), am.cpu(), nl.tolist()
        for r in range(c["rows"]):
            p, v = c["plen"][r], nl[r]
            assert (lp[r, max(v, 1):] == 0).all() and (am[r, v:] == -1).all(), (tag, k, r, "pads")
            assert torch.isfinite(lp[r, 1:]).all() and (am[r, :v] >= 0).all(), (tag, k, r)
            pos = p + off[r] + torch.arange(max(v - 1, 0))  # forward positions that predict columns 1 .. v - 1
            ref = want[r, pos].gather(1, c["cont"][r, off[r] + 1:off[r] + v, None])[:, 0]
            d = _rms(lp[r, 1:v], ref)
            print(f"[shared score] {tag} block {k} row {r} ({v} tokens behind {p}+{off[r]}): rms {d:.3e} (bar {c['bars'][r]:.3e})")
            assert d <= c["bars"][r], (tag, k, r, d, c["bars"][r])
            if v == 0:
                if prev is not None:
                    assert torch.equal(logits[r], prev[r]), (tag, k, r, "an inert row keeps its logits")
                continue
            e = rel_err(logits[r], c["lg"][r, p + off[r] + v - 1])
            assert torch.isfinite(logits[r]).all() and e <= LOGITS_TOL, (tag, k, r, e)
        prev = logits


@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("tag", ["g7", "g1", "g8", "g6hd128", "qwen3"])
def test_extend_score_in_the_shared_mode(tag, n, T):
    m = _model(tag)
    c = _case(m, n, T)
    outs, lens, cache, store, store0 = _run(m, c, True)
    _check_blocks(c, outs, (tag, n, T, "shared"))
    assert lens == [p + t for p, t in zip(c["plen"], c["clen"])], "lens stay absolute"
    assert torch.equal(store, store0), "the prompt store was written"
    d = m.engine.desc
    rows_written = (cache.view(d.n_layers, 2, c["rows"], d.n_kv_heads, CAP, d.head_dim) != POISON).any(-1)
    expect = torch.arange(CAP)[None] < torch.tensor(c["clen"])[:, None]  # row r: exactly the indices lens - plen + t
    assert torch.equal(rows_written.cpu(), expect[None, None, :, None, :].expand_as(rows_written)), "cache written elsewhere"
    outs2, _, cache2, _, _ = _run(m, c, True)
    assert all(torch.equal(a, b) for x, y in zip(outs, outs2) for a, b in zip(x, y)) and torch.equal(cache, cache2), \
        "not bit-identical run to run"
    _check_blocks(c, _run(m, c, False)[0], (tag, n, T, "prefill + kv_repeat"))


def test_extend_logits_in_the_shared_mode():
    m = _model("g7")
    c = _case(m, 3, 17, seed=4)
    outs = _run(m, c, True, logits_all=True)[0]
    for k, ((_, la, _), (_, nl, off)) in enumerate(zip(outs, c["blocks"])):
        la = la.cpu()
        for r, v in enumerate(nl.tolist()):
            assert (la[r, v:] == 7.0).all(), (k, r, "rows t >= new_lens keep their bits")
            for t in range(v):
                e = rel_err(la[r, t], c["lg"][r, c["plen"][r] + off[r] + t])
                assert torch.isfinite(la[r, t]).all() and e <= LOGITS_TOL, (k, r, t, e)


def test_score_continuations_share_prompt_cache():
    m = _mk(*_tiny(), max_tokens=512)
    V, n, Tc, B, T, plens = m.engine.desc.vocab, 3, 12, 3, 70, [70, 41, 5]
    g = torch.Generator().manual_seed(2)
    ids, mask = torch.randint(2, V, (B, T), generator=g), torch.zeros(B, T, dtype=torch.long)
    for b, ln in enumerate(plens):  # left-padded
        mask[b, T - ln:] = 1
        ids[b, :T - ln] = 0
    cont = torch.randint(2, V, (B * n, Tc), generator=g)
    clen = torch.tensor([Tc, 0, 7, 1, Tc, 5, 11, Tc, 6])
    kw = dict(continuations=cont, continuation_lengths=clen, num_per_prompt=n, score_chunk=5, return_argmax=True)
    lp0, am0 = (t.cpu() for t in m.score_continuations(ids, mask, **kw))
    bound = []
    for name in ("bind_kv_cache", "bind_kv_prefix"):  # record the bytes each binding gets
        setattr(m.engine, name, lambda buf, *a, _f=getattr(m.engine, name): (bound.append(0 if buf is None else buf.numel()), _f(buf, *a))[1])
    lp1, am1 = (t.cpu() for t in m.score_continuations(ids, mask, share_prompt_cache=True, **kw))
    assert 0 < sum(bound) < m.engine.kv_cache_bytes(B * n, -(-(T + Tc) // 64) * 64), bound
    full, _, plen = _concat(ids, mask, n, cont, clen)
    bars, lg = _bars(m, full, plen, clen)
    want = torch.log_softmax(lg.double(), -1)
    assert torch.equal(lp1[:, 0], lp0[:, 0]) and torch.equal(am1[:, 0], am0[:, 0]), "column 0: the same prefill bits"
    for r, (p, v) in enumerate(zip(plen, clen.tolist())):
        assert (lp1[r, v:] == 0).all() and (am1[r, v:] == -1).all() and torch.isfinite(lp1[r]).all(), (r, "pads")
        ref = want[r, p - 1:p - 1 + v].gather(1, cont[r, :v, None])[:, 0]
        assert _rms(lp1[r, :v], ref) <= bars[r] and _rms(lp1[r, :v], lp0[r, :v]) <= bars[r], (r, bars[r])
        top = lg[r, p - 1:p - 1 + v].topk(2, -1)
        clear = (top.values[:, 0] - top.values[:, 1]) > bars[r]
        assert torch.equal(am1[r, :v][clear], top.indices[:, 0][clear]), (r, "argmax away from a near-tie")
