"""-m gpu: the FP8 KV cache (include/slam_engine.h: SLAM_KV_FP8_E4M3) against tests/kv8_ref.py.
 * both scatter kernels: codes and exponents bit-equal to the rule, guard bytes and every unwritten byte intact;
 * decode and chunk attention over codes: bit-equal to the bf16 kernels over a bf16 cache of the dequantised values, and within
   the bf16 kernels' own tolerances of an fp64 softmax-attention over the dequantised cache;
 * prefill + decode steps and generate on the tiny Qwen2 / Qwen3 models."""
import math

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests import kv8_ref as K8
from tests.gpu_util import lib, ptr, rel_err, stream, sync
from tests.test_gpu_generate import LOGITS_TOL, _mk, _tiny

pytestmark = pytest.mark.gpu
FILL = 0xA5   # unwritten bytes and guards
NANCODE = 0x7F  # e4m3 NaN: a cache row no kernel may read
OP_TOL = 1e-2  # tests/test_gpu_extend.py OP_TOL: per-row rel-RMS of attn_extend against fp64 (the same arithmetic here)


def _guarded(n):
    full = torch.full((n + 512,), FILL, dtype=torch.uint8, device="cuda")
    return full, full[256:256 + n]


def _bits(t):
    return t.view(torch.int16)


def _fp8_cache(k, v, lens):
    """bf16 K / V [B][nKV][cap][hd] -> device codes / exponents (rows >= lens[b]: NaN codes) and the dequantised bf16 caches."""
    dev, dq = [], []
    for x in (k, v):
        c, e = K8.quantize(x)
        d = K8.dequantize(c, e)
        for b, n in enumerate(lens):
            c[b, :, n:] = NANCODE
            d[b, :, n:] = math.nan
        dev += [torch.from_numpy(c).cuda(), torch.from_numpy(e).cuda()]
        dq.append(d)
    return dev[0], dev[2], dev[1], dev[3], dq[0], dq[1]  # kc, vc, ke, ve, Kdq, Vdq


def _edge_vectors(hd, g):
    z = torch.zeros(hd)
    top = torch.randn(hd, generator=g).clamp(-1, 1) * 40
    top[3] = -56.0  # 448 * 2^-3: the scaled maximum lands exactly on the largest e4m3 magnitude
    sub = torch.randn(hd, generator=g) * 2.0 ** -16  # amax 1 -> e = -8: everything below 2^-14 is an e4m3 subnormal
    sub[hd - 1] = 1.0
    return [z, top, sub]


@pytest.mark.parametrize("T", [1, 7, 65])
@pytest.mark.parametrize("nKV", [1, 2])
@pytest.mark.parametrize("hd", [64, 128])
def test_scatter_kernels_follow_the_rule(hd, nKV, T):
    B, nH = 3, 2 * nKV
    QKV = (nH + 2 * nKV) * hd
    g = torch.Generator().manual_seed(hd + 10 * nKV + T)
    x = torch.randn(B, T, nH + 2 * nKV, hd, generator=g) * torch.exp2(torch.randint(-12, 12, (B, T, nH + 2 * nKV, 1), generator=g))
    ev = _edge_vectors(hd, g)
    x[0, 0, nH], x[0, 0, nH + nKV], x[1, 0, nH] = ev[0], ev[1], ev[2]
    x[2, 0, nH + nKV], x[2, 0, nH], x[1, 0, nH + nKV] = ev[0], ev[1], ev[2]
    qkv = x.to(torch.bfloat16).view(B * T, QKV)
    qd = qkv.cuda()
    for base, new in (([0, 0, 0], [T, (T + 1) // 2, 1]), ([0, 5, 63], [T, T // 2, 0])):  # prefill lens; a chunk with an inert row
        extend = any(base)
        cap = 63 + T + 3
        bound = max(b + n for b, n in zip(base, new))
        bufs = [_guarded(B * nKV * cap * hd), _guarded(B * nKV * cap * hd), _guarded(B * nKV * cap), _guarded(B * nKV * cap)]
        (kc, vc, ke, ve) = [v for _, v in bufs]
        base_d, new_d = (torch.tensor(a, dtype=torch.int32, device="cuda") for a in (base, new))
        if extend:
            rc = lib().slam_op_kv_extend_scatter_fp8(ptr(qd), ptr(base_d), ptr(new_d), ptr(kc), ptr(vc), ptr(ke), ptr(ve), B, T, nH,
                                                     nKV, hd, cap, bound, stream())
        else:
            rc = lib().slam_op_kv_scatter_fp8(ptr(qd), ptr(new_d), ptr(kc), ptr(vc), ptr(ke), ptr(ve), B, T, nH, nKV, hd, cap, stream())
        assert rc == 0, rc
        sync()
        xb = qkv.view(B, T, nH + 2 * nKV, hd)
        for kv, (cbuf, ebuf) in enumerate(((bufs[0], bufs[2]), (bufs[1], bufs[3]))):
            want_c = np.full((B, nKV, cap, hd), FILL, np.uint8)
            want_e = np.full((B, nKV, cap), FILL, np.uint8).view(np.int8)
            for b in range(B):
                if new[b]:
                    src = xb[b, :new[b], nH + kv * nKV:nH + (kv + 1) * nKV].transpose(0, 1).contiguous()  # [nKV][n][hd]
                    want_c[b, :, base[b]:base[b] + new[b]], want_e[b, :, base[b]:base[b] + new[b]] = K8.quantize(src)
            for (full, view), want in ((cbuf, want_c), (ebuf, want_e.view(np.uint8))):
                assert np.array_equal(view.cpu().numpy().reshape(want.shape), want), (hd, nKV, T, extend, "K V"[2 * kv], want.ndim)
                assert bool((full[:256] == FILL).all()) and bool((full[-256:] == FILL).all()), "guard bytes overwritten"


def _decode_run(fp8, qkv, lens_d, caches, B, nH, nKV, hd, cap, bound, ws_bytes, theta):
    o = torch.zeros(B, nH * hd, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    if fp8:
        kc, vc, ke, ve = (c.clone() for c in caches)
        rc = lib().slam_op_attn_decode_fp8(ptr(qkv), None, ptr(lens_d), ptr(kc), ptr(vc), ptr(ke), ptr(ve), ptr(o), ptr(ws), ws_bytes, B,
                                           nH, nKV, hd, cap, bound, theta, stream())
        out = (kc, vc, ke, ve)
    else:
        kc, vc = (c.clone() for c in caches)
        rc = lib().slam_op_attn_decode(ptr(qkv), None, ptr(lens_d), ptr(kc), ptr(vc), ptr(o), ptr(ws), ws_bytes, B, nH, nKV, hd, cap,
                                       bound, theta, stream())
        out = (kc, vc)
    assert rc == 0, rc
    sync()
    return o.cpu(), [t.cpu() for t in out]


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: f"hd{i[0]}-g{i[1]}-kv{i[2]}")
def test_attn_decode_fp8(inst):
    """Row lengths 1, 63, 64, 65 (slot and wave strides) and chunk - 1, chunk, chunk + 1 of the 128-key split plan (a workspace
    with room for two splits), and the same rows under the full workspace (64-key splits). Check (a), through the doors as they
    are: a new token whose bf16 K / V are on their own e4m3 grid (K = 0, V small integers) leaves both kernels with the same
    cache, so the whole output must be bit-equal, old keys and new token; for a gaussian new token the appended codes and
    exponents are kv8_ref's of the bf16 kernel's appended row. Check (b): fp64 over the dequantised cache at R.ATTN_TOL, the
    per-(row, head) relative L2 bound tests/test_gpu_decode_edges.py holds the bf16 kernel to."""
    hd, G, nKV = inst
    nH, lens, cap, bound, theta = G * nKV, [1, 63, 64, 65, 127, 128, 129], 192, 130, 10000.0
    B = len(lens)
    g = torch.Generator().manual_seed(hd + G + nKV)
    k, v = (torch.randn(B, nKV, cap, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    kc, vc, ke, ve, Kdq, Vdq = _fp8_cache(k, v, lens)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    full = lib().slam_op_attn_decode_workspace(B, nH, nKV, hd, bound)
    two = R.attn_op_head(B, hd) + B * nH * 2 * (hd + 2) * 4
    assert R.attn_decode_chunk(B, nH, nKV, hd, bound, two - R.attn_op_head(B, hd)) == 128
    x = torch.randn(B, nH + 2 * nKV, hd, generator=g) * 2
    exact = x.clone()
    exact[:, nH:nH + nKV] = 0
    exact[:, nH + nKV:] = torch.randint(-7, 8, (B, nKV, hd), generator=g).float()
    exact[:, nH + nKV:, 0] = 7
    for ws_bytes in (two, full):
        for new_exact, qkv in ((True, exact), (False, x)):
            qd = qkv.reshape(B, -1).contiguous().cuda()
            o8, c8 = _decode_run(True, qd, lens_d, (kc, vc, ke, ve), B, nH, nKV, hd, cap, bound, ws_bytes, theta)
            ob, cb = _decode_run(False, qd, lens_d, (Kdq.cuda(), Vdq.cuda()), B, nH, nKV, hd, cap, bound, ws_bytes, theta)
            dq = [K8.dequantize(c8[i].numpy(), c8[i + 2].numpy()) for i in (0, 1)]
            for b, n in enumerate(lens):
                for i in (0, 1):  # the appended vector against the rule, everything else untouched
                    wc, we = K8.quantize(cb[i][b, :, n])
                    assert np.array_equal(c8[i][b, :, n].numpy(), wc) and np.array_equal(c8[i + 2][b, :, n].numpy(), we), (inst, b, i)
                    assert torch.equal(c8[i][b, :, :n], (kc, vc)[i][b, :, :n].cpu()) and bool((c8[i][b, :, n + 1:] == NANCODE).all())
                    if new_exact:
                        assert torch.equal(_bits(dq[i][b, :, n]), _bits(cb[i][b, :, n])), "the exact token is not exact"
            if new_exact:
                assert torch.equal(_bits(o8), _bits(ob)), (inst, ws_bytes, "not bit-equal to the bf16 kernel", (o8 != ob).sum())
            for b, n in enumerate(lens):  # (b)
                q = R._bf16(R._rope(qkv[b, :nH].double(), n, hd, theta) * (hd ** -0.5 * R.LOG2E)).double().view(nKV, G, hd)
                s = torch.einsum("kgd,kjd->kgj", q, dq[0][b, :, :n + 1].double())
                p = torch.exp2(s - s.max(-1, keepdim=True).values)
                ref = (torch.einsum("kgj,kjd->kgd", p, dq[1][b, :, :n + 1].double()) / p.sum(-1, keepdim=True)).reshape(nH, hd)
                err = ((o8[b].double().view(nH, hd) - ref).norm(dim=-1) / ref.norm(dim=-1)).max()
                assert float(err) <= R.ATTN_TOL, (inst, b, n, float(err))


@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_extend_fp8(hd, T):
    """The chunk's own K / V columns are put on their e4m3 grid first, so the bf16 kernel appends what the FP8 kernel reads back
    dequantised: the outputs must be bit-equal. The rule itself is test_scatter_kernels_follow_the_rule's."""
    nH, nKV, base, new = 4, 2, [0, 1, 63, 200, 63], [T, max(T - 2, 1), T, T, 0]
    B, G, cap = len(base), 2, 200 + T
    bound = max(b + n for b, n in zip(base, new))
    g = torch.Generator().manual_seed(hd + T)
    k, v = (torch.randn(B, nKV, cap, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    kc, vc, ke, ve, Kdq, Vdq = _fp8_cache(k, v, base)
    x = torch.randn(B, T, nH + 2 * nKV, hd, generator=g)
    x[:, :, :nH] *= 2 * hd ** -0.5 * R.LOG2E
    x = x.to(torch.bfloat16)
    x[:, :, nH:] = K8.dequantize(*K8.quantize(x[:, :, nH:].contiguous()))
    qd = x.view(B * T, -1).cuda()
    base_d, new_d = (torch.tensor(a, dtype=torch.int32, device="cuda") for a in (base, new))
    nws = lib().slam_op_attn_extend_workspace(B, T, nH, nKV, hd, bound)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device="cuda")
    o8, ob = (torch.empty(B * T, nH * hd, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    kb, vb = Kdq.cuda(), Vdq.cuda()
    assert lib().slam_op_attn_extend_fp8(ptr(qd), ptr(base_d), ptr(new_d), ptr(kc), ptr(vc), ptr(ke), ptr(ve), ptr(o8), ptr(ws), nws, B, T,
                                         nH, nKV, hd, cap, bound, stream()) == 0
    assert lib().slam_op_attn_extend(ptr(qd), ptr(base_d), ptr(new_d), ptr(kb), ptr(vb), ptr(ob), ptr(ws), nws, B, T, nH, nKV, hd, cap,
                                     bound, stream()) == 0
    sync()
    assert torch.equal(_bits(o8), _bits(ob)), ((hd, T), "not bit-equal to the bf16 kernel", int((o8 != ob).sum()))
    Kn, Vn = K8.dequantize(kc.cpu().numpy(), ke.cpu().numpy()), K8.dequantize(vc.cpu().numpy(), ve.cpu().numpy())
    for b, (p, n) in enumerate(zip(base, new)):
        assert torch.equal(_bits(Kn[b, :, :p + n]), _bits(kb[b, :, :p + n].cpu())) and torch.equal(_bits(Vn[b, :, :p + n]), _bits(vb[b, :, :p + n].cpu()))
        assert bool((kc[b, :, p + n:] == NANCODE).all()) and bool((vc[b, :, p + n:] == NANCODE).all()), "wrote past the chunk"
        if n == 0:
            continue
        q = x[b, :n, :nH].double()
        s = torch.einsum("thd,hjd->htj", q, Kn[b, :, :p + n].double().repeat_interleave(G, 0))
        s = s.masked_fill(torch.arange(p + n)[None, None, :] > p + torch.arange(n)[None, :, None], -math.inf)
        pr = torch.exp2(s - s.max(-1, keepdim=True).values)
        ref = torch.einsum("htj,hjd->thd", pr, Vn[b, :, :p + n].double().repeat_interleave(G, 0)) / pr.sum(-1).t()[..., None]
        e = rel_err(o8.view(B, T, nH, hd)[b, :n].float(), ref)
        assert e <= OP_TOL, ((hd, T), b, e)


def _models():
    from tests.test_gpu_qwen3 import _gen_model
    return {"qwen2": lambda: _mk(*_tiny()), "qwen3": lambda: _gen_model("A")[0]}


@pytest.mark.parametrize("family", ["qwen2", "qwen3"])
def test_prefill_and_decode_steps_on_the_fp8_cache(family):
    """Teacher-forced prefill + 6 decode steps on an FP8 cache, and on a bf16 cache (a second model, the same weights) that is
    overwritten before every step with the dequantised contents of the FP8 one, read back through the binding. Bit-exact: the
    prefill's logits; the FP8 cache against the rule applied to what the bf16 run stored - every layer after the prefill, layer 0
    after a step (its input is the embedding, which both runs share). A step's logits are held to LOGITS_TOL only: through the
    ABI the bf16 step always scores its own new token unquantised, so the two steps cannot be equal (the kernels' bit-equality
    is test_attn_decode_fp8's)."""
    m8, mb = _models()[family](), _models()[family]()
    d, dev = m8.engine.desc, m8.device
    L, nKV, hd, V = d.n_layers, d.n_kv_heads, d.head_dim, d.vocab
    B, T, cap, lens = 2, 9, 64, [9, 4]
    ids = torch.randint(2, V, (B, T + 6), generator=torch.Generator().manual_seed(5)).to(dev)
    c8 = torch.zeros(m8.engine.kv_cache_bytes(B, cap, "fp8_e4m3"), dtype=torch.uint8, device=dev)
    cb = torch.zeros(mb.engine.kv_cache_bytes(B, cap) // 2, dtype=torch.bfloat16, device=dev)
    assert c8.numel() == K8.cache_bytes(L, B, nKV, cap, hd)
    for m in (m8, mb):
        m._ensure_workspace(B * T)
    m8.engine.bind_kv_cache(c8, B, cap, "fp8_e4m3")
    mb.engine.bind_kv_cache(cb, B, cap)
    lg8, lgb = (torch.empty(B, V, dtype=torch.float32, device=dev) for _ in range(2))
    l8, lb = (torch.tensor(lens, dtype=torch.int32, device=dev) for _ in range(2))
    for step in range(7):
        if step == 0:
            m8.engine.prefill(ids[:, :T].contiguous(), l8, B, T, lg8)
            mb.engine.prefill(ids[:, :T].contiguous(), lb, B, T, lgb)
        else:
            tok = ids[:, T + step - 1].contiguous()
            m8.engine.decode_step(tok, l8, B, lg8)
            mb.engine.decode_step(tok, lb, B, lgb)
        sync()
        codes, exps = K8.split(c8, L, B, nKV, cap, hd)
        stored = cb.cpu().view(L, 2, B, nKV, cap, hd)
        for b, n in enumerate(lens):
            new = slice(0, n) if step == 0 else slice(n + step - 1, n + step)
            layers = slice(0, L if step == 0 else 1)
            wc, we = K8.quantize(stored[layers, :, b, :, new])
            assert np.array_equal(codes[layers, :, b, :, new], wc) and np.array_equal(exps[layers, :, b, :, new], we), (family, step, b)
        if step == 0:
            assert torch.equal(lg8, lgb), "prefill logits differ"
        for b in range(B):
            assert rel_err(lg8[b], lgb[b]) <= LOGITS_TOL, (family, step, b, rel_err(lg8[b], lgb[b]))
        cb.copy_(K8.dequantize(codes, exps).reshape(-1))
    assert l8.tolist() == lb.tolist() == [n + 6 for n in lens]


@pytest.mark.parametrize("family", ["qwen2", "qwen3"])
def test_generate_with_the_fp8_cache(family):
    m = _models()[family]()
    ids = torch.randint(2, m.engine.desc.vocab, (2, 11), generator=torch.Generator().manual_seed(1))
    assert m.kv_cache_dtype == "bfloat16"
    plain = m.generate(ids, max_new_tokens=5, do_sample=False)
    assert torch.equal(plain, m.generate(ids, max_new_tokens=5, do_sample=False, kv_cache_dtype="bfloat16"))
    out = m.generate(ids, max_new_tokens=5, do_sample=True, seed=3, num_return_sequences=2, prefill_chunk=4, kv_cache_dtype="fp8_e4m3")
    assert out.shape[0] == 4 and 11 < out.shape[1] <= 16 and torch.equal(out[::2, :11].cpu(), ids)
    m.kv_cache_dtype = "fp8_e4m3"
    assert m.generate(ids, max_new_tokens=5, do_sample=False).shape[0] == 2
    del m.kv_cache_dtype
    assert torch.equal(plain, m.generate(ids, max_new_tokens=5, do_sample=False)), "the default path changed"
    for call in (lambda: m.generate(ids, max_new_tokens=2, kv_cache_dtype="int8"),
                 lambda: m.score_continuations(ids, continuations=ids[:, :3], kv_cache_dtype="e5m2")):
        with pytest.raises(ValueError, match="bfloat16.*fp8_e4m3"):
            call()


def test_opt_refuses_the_fp8_cache():
    from tests.test_gpu_opt import _unit_lm
    m = _unit_lm(max_tokens=256)
    with pytest.raises(ValueError):
        m.generate(torch.ones(1, 4, dtype=torch.long), max_new_tokens=2, kv_cache_dtype="fp8_e4m3")
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=m.device)
    assert m.engine.kv_cache_bytes(1, 64, "fp8_e4m3") == 0
    rc = lib().slam_bind_kv_cache_ex(m.engine.h, ptr(buf), buf.numel(), 1, 64, 1)
    assert rc == -1 and b"OPT" in lib().slam_last_error(m.engine.h)
