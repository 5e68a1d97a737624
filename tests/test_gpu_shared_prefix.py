"""-m gpu: the shared-prompt cache (slam_kv_share). slam_op_attn_decode_shared against decode_ref.attn_decode_ref (fp64) fed each
row's materialised cache - its prompt's keys, then its own - at decode_ref.ATTN_TOL per (row, head), the prompt store and the
cache poisoned with a bf16 NaN pattern wherever they may not be read and compared as integers afterwards; prefill_prefix +
kv_share + decode steps against prefill + kv_repeat + the same steps; generate(share_prompt_cache=True) against the unshared call."""
import pytest
import torch

from slamkit_amd.model.generation import _bind_cache, _bind_prefix
from tests import decode_ref as R
from tests.gpu_util import lib, ptr, rel_err, stream, sync
from tests.test_gpu_generate import LOGITS_TOL, _mk, _tiny
from tests.test_gpu_kv_fp8 import _models

pytestmark = pytest.mark.gpu

POISON, SENTINEL, GUARD = 0x7FC1, -8192.0, 1024  # a bf16 NaN; what fills outputs and the guard words behind a workspace
NKV, PCAP, CAP = 2, 192, 128
SUFFIX = [0, 1, 63, 64, 65]  # keys a row holds behind its prompt: none, one, and both sides of the 64-key suffix split
_i16 = lambda t: t.view(torch.int16)  # noqa: E731


def _case(hd, G, n, pbig, seed):
    """Device inputs of one call over 3 prompts x n rows, and the fp64 reference over the materialised caches."""
    nH, P = G * NKV, 3
    rows = P * n
    plens = [1, 33, pbig]
    suf = [SUFFIX[(r + r // n) % len(SUFFIX)] for r in range(rows)]
    lens = [plens[r // n] + suf[r] for r in range(rows)]
    g = torch.Generator().manual_seed(seed)
    QKV = (nH + 2 * NKV) * hd
    qkv = torch.randn(rows, QKV, generator=g) * 2
    bias = (torch.randn(QKV, generator=g) * 0.5).to(torch.bfloat16)
    pk, pv = (torch.randn(P, NKV, PCAP, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    kc, vc = (torch.randn(rows, NKV, CAP, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    full_k, full_v = (torch.zeros(rows, NKV, max(lens) + 1, hd, dtype=torch.bfloat16) for _ in range(2))
    for r in range(rows):
        for full, store, cache in ((full_k, pk, kc), (full_v, pv, vc)):
            full[r, :, :lens[r]] = torch.cat([store[r // n, :, :plens[r // n]], cache[r, :, :suf[r]]], 1)
    for t, ends in ((pk, plens), (pv, plens), (kc, suf), (vc, suf)):
        for i, e in enumerate(ends):
            _i16(t)[i, :, e:] = POISON
    theta = 10000.0 if hd == 64 else 1e6
    ref = R.attn_decode_ref(qkv, bias, lens, full_k, full_v, nH, NKV, hd, theta)[0]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    return dict(hd=hd, nH=nH, n=n, P=P, rows=rows, plens=plens, suf=suf, lens=lens, theta=theta, ref=ref, qkv=qkv.cuda(),
                bias=bias.cuda(), pk=pk.cuda(), pv=pv.cuda(), kc=kc.cuda(), vc=vc.cuda(), lens_d=i32(lens), plens_d=i32(plens),
                pbound=max(plens), sbound=max(suf) + 1)


def _run(c, ws_bytes):
    kc, vc, pk, pv = c["kc"].clone(), c["vc"].clone(), c["pk"].clone(), c["pv"].clone()
    o = torch.full((c["rows"], c["nH"] * c["hd"]), SENTINEL, dtype=torch.bfloat16, device="cuda")
    ws = torch.full((ws_bytes // 4 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib().slam_op_attn_decode_shared(ptr(c["qkv"]), ptr(c["bias"]), ptr(c["lens_d"]), ptr(c["plens_d"]), c["n"], ptr(pk), ptr(pv),
                                          PCAP, ptr(kc), ptr(vc), CAP, ptr(o), ptr(ws), ws_bytes, c["P"], c["nH"], NKV, c["hd"],
                                          c["pbound"], c["sbound"], c["theta"], stream())
    sync()
    return rc, o, kc, vc, pk, pv, ws


def _check(c, ws_bytes, tag):
    rc, o, kc, vc, pk, pv, ws = _run(c, ws_bytes)
    assert rc == 0, (tag, rc)
    assert bool((ws[ws_bytes // 4:] == SENTINEL).all()), (tag, "wrote past the workspace")
    got = o.view(c["rows"], c["nH"], c["hd"]).double().cpu()
    assert torch.isfinite(got).all(), tag
    err = (got - c["ref"]).norm(dim=-1) / c["ref"].norm(dim=-1)
    assert float(err.max()) <= R.ATTN_TOL, (tag, float(err.max()), divmod(int(err.argmax()), c["nH"]))
    assert torch.equal(_i16(pk), _i16(c["pk"])) and torch.equal(_i16(pv), _i16(c["pv"])), (tag, "prompt store written")
    keep = torch.ones(c["rows"], CAP, dtype=torch.bool, device="cuda")
    keep[torch.arange(c["rows"], device="cuda"), torch.tensor(c["suf"], device="cuda")] = False
    for new, old in ((kc, c["kc"]), (vc, c["vc"])):
        assert torch.equal(_i16(new).transpose(1, 2)[keep], _i16(old).transpose(1, 2)[keep]), (tag, "cache written elsewhere")
    # the store kept every bit, the cache changed at the new token's index alone; there: what the unshared step appends
    capA = max(c["lens"]) + 1
    ka, va = (torch.zeros(c["rows"], NKV, capA, c["hd"], dtype=torch.bfloat16, device="cuda") for _ in range(2))
    nws = lib().slam_op_attn_decode_workspace(c["rows"], c["nH"], NKV, c["hd"], capA)
    wsa = torch.empty(nws, dtype=torch.uint8, device="cuda")
    oa = torch.empty_like(o)
    assert lib().slam_op_attn_decode(ptr(c["qkv"]), ptr(c["bias"]), ptr(c["lens_d"]), ptr(ka), ptr(va), ptr(oa), ptr(wsa), nws, c["rows"],
                                     c["nH"], NKV, c["hd"], capA, capA, c["theta"], stream()) == 0
    sync()
    for r in range(c["rows"]):
        assert torch.equal(_i16(kc[r, :, c["suf"][r]]), _i16(ka[r, :, c["lens"][r]])), (tag, r, "appended K")
        assert torch.equal(_i16(vc[r, :, c["suf"][r]]), _i16(va[r, :, c["lens"][r]])), (tag, r, "appended V")
    rc2, o2, kc2, vc2 = _run(c, ws_bytes)[:4]
    assert rc2 == 0 and torch.equal(_i16(o), _i16(o2)) and torch.equal(_i16(kc), _i16(kc2)) and torch.equal(_i16(vc), _i16(vc2)), \
        (tag, "not bit-identical run to run")


PSPLIT = 128  # the first prefix split's end at these shapes (slam::attn_shared_plan's floor): asserted below


@pytest.mark.parametrize("n", [1, 3, 10, 16])
@pytest.mark.parametrize("G", [1, 6, 7, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_shared_vs_fp64(hd, G, n):
    """n G = 1 .. 128 queries per (prompt, KV head): below one tile, 16, 48, 70 (past one 64-query block), 128."""
    for pbig in (32, 65, PSPLIT + 1):
        c = _case(hd, G, n, pbig, seed=1000 * hd + 100 * G + n)
        full = lib().slam_op_attn_decode_shared_workspace(c["P"], n, c["nH"], NKV, hd, c["pbound"], c["sbound"])
        splits = (full - R.attn_op_head(c["rows"], hd)) // (c["rows"] * c["nH"] * (hd + 2) * 4)
        assert splits == (2 if pbig > PSPLIT else 1) + 2, (pbig, splits)  # prefix splits + the two suffix splits of 65 + 1 keys
        _check(c, full, (hd, G, n, pbig))


@pytest.mark.parametrize("hd,G,n", [(64, 7, 10), (128, 6, 3)])
def test_attn_decode_shared_workspace_limits(hd, G, n):
    """Room for one split of each part: the same bars. Four bytes less: SLAM_ENOMEM and nothing written, the workspace included."""
    c = _case(hd, G, n, PSPLIT + 1, seed=hd + G + n)
    one_each = R.attn_op_head(c["rows"], hd) + c["rows"] * c["nH"] * 2 * (hd + 2) * 4
    _check(c, one_each, (hd, G, n, "one split each"))
    rc, o, kc, vc, pk, pv, ws = _run(c, one_each - 4)
    assert rc == -3
    assert bool((o == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert all(torch.equal(_i16(a), _i16(c[k])) for a, k in ((kc, "kc"), (vc, "vc"), (pk, "pk"), (pv, "pv")))


# ---- engine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["qwen2", "qwen3"])
def test_prefill_prefix_share_and_decode_steps(family):
    m = _models()[family]()
    eng, dev, V = m.engine, m.device, m.engine.desc.vocab
    B, T, n, cap, steps, plens = 3, 9, 3, 64, 5, [9, 4, 6]
    rows = B * n
    ids, toks = (torch.randint(2, V, sh, generator=torch.Generator().manual_seed(11)).to(dev) for sh in ((B, T), (steps, rows)))
    m._ensure_workspace(max(B * T, 2 * rows))

    def run(shared):
        lens = torch.zeros(rows, dtype=torch.int32, device=dev)
        lens[:B] = torch.tensor(plens, dtype=torch.int32)
        logits = torch.full((rows, V), float("nan"), dtype=torch.float32, device=dev)
        raw = [_bind_cache(m, rows, cap)] + ([_bind_prefix(m, B, cap)] if shared else [])  # noqa: F841 - alive until run returns
        (eng.prefill_prefix if shared else eng.prefill)(ids, lens, B, T, logits)
        out = [logits[:B].clone()]
        (eng.kv_share if shared else eng.kv_repeat)(n, lens, logits)
        out.append(logits.clone())
        for s in range(steps):
            eng.decode_step(toks[s].contiguous(), lens, rows, logits)
            out.append(logits.clone())
        sync()
        return out, lens

    want, lens_r = run(False)
    got, lens_s = run(True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "prefill_prefix / fanned-out logits differ from prefill's"
    assert lens_s.tolist() == lens_r.tolist() == [plens[r // n] + steps for r in range(rows)]
    for s in range(steps):
        for r in range(rows):
            e = rel_err(got[2 + s][r], want[2 + s][r])
            assert torch.isfinite(got[2 + s][r]).all() and e <= LOGITS_TOL, (family, s, r, e)
    h, one = eng.h, torch.ones(rows, dtype=torch.int32, device=dev)
    lg = torch.empty(rows, V, dtype=torch.float32, device=dev)
    assert lib().slam_extend(h, ptr(toks[0]), ptr(one), ptr(lens_s), rows, 1, ptr(lg), stream()) == -2
    assert lib().slam_kv_repeat(h, 2, ptr(lens_s), None, stream()) == -2
    assert lib().slam_kv_rewind(h, 1) == -2 and b"shared" in lib().slam_last_error(h)
    lens = torch.tensor(plens, dtype=torch.int32, device=dev)
    eng.prefill(ids, lens, B, T, lg)
    sync()
    assert torch.equal(lg[:B], want[0])
    assert lib().slam_kv_rewind(h, T) == 0


@pytest.mark.parametrize("guidance", [None, 2.0])
def test_generate_share_prompt_cache(guidance):
    m = _mk(*_tiny())
    V, n, new = m.engine.desc.vocab, 3, 8
    B, T, plens = 3, 70, [70, 41, 5]
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(2, V, (B, T), generator=g)
    mask = torch.zeros(B, T, dtype=torch.long)
    for b, ln in enumerate(plens):  # left-padded
        mask[b, T - ln:] = 1
        ids[b, :T - ln] = 0
    kw = dict(attention_mask=mask, max_new_tokens=new, do_sample=True, sampler="engine", top_k=20, seed=5, num_return_sequences=n,
              pad_token_id=0, guidance_scale=guidance)
    plain = m.generate(ids, **kw).cpu()
    eos = int(plain[0, T])  # row 0's first draw: with it as EOS that row ends at once
    kw["eos_token_id"] = eos
    plain = m.generate(ids, **kw).cpu()
    bound = []
    for name in ("bind_kv_cache", "bind_kv_prefix"):  # record the bytes each binding gets
        setattr(m.engine, name, lambda buf, *a, _f=getattr(m.engine, name): (bound.append(0 if buf is None else buf.numel()), _f(buf, *a))[1])
    out = m.generate(ids, share_prompt_cache=True, **kw).cpu()
    assert out.shape[0] == B * n and T < out.shape[1] <= T + new
    assert torch.equal(out[:, :T], ids.repeat_interleave(n, 0)), "row r is not prompt r // n"
    assert torch.equal(out[:, T], plain[:, T]), "the first draw differs: same prefill bits, same draw"
    after_eos = (out[:, T:] == eos).cumsum(1).cumsum(1) > 1  # columns behind a row's first EOS
    assert (out[:, T:][after_eos] == 0).all() and bool(after_eos[0, 1:].all()), "no pad behind EOS"
    rows = B * n * (1 if guidance is None else 2)
    assert 0 < sum(bound) < m.engine.kv_cache_bytes(rows, -(-(T + new) // 64) * 64), bound
