"""-m gpu: the Qwen3 decoder family (arch 3). The three per-head q / k RMSNorm kernels through their slam_op_* entry points
against tests/qwen3_ref.py in fp64; the engine-backed UnitLM against HF Qwen3ForCausalLM (tests/golden/qwen3.npz) and against
the restatement's autograd - logits, loss, gradients, packed batches, log-likelihood, recomputation, the optimizer step,
checkpoints, TWIST initialisation - and KV-cached generation and scoring."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from slamkit_amd import engine as E
from tests import qwen3_ref as R
from tests.gpu_util import check, cosine, dev_bf16, lib, ptr, rel_err, rnd, stream, sync

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen3.npz")
LOGITS_TOL = 2e-2  # tests/test_gpu_generate.py
GUARD, SENT = 16, -7.0  # canary rows behind every output, and their value


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------------------- kernels
def _guarded(rows, cols, dtype):
    """[rows + GUARD][cols]: NaN body (every element must be written), sentinel canary rows behind it."""
    t = torch.full((rows + GUARD, cols), SENT, dtype=dtype, device="cuda")
    t[:rows] = float("nan")
    return t


def _positions(M):
    pos = (torch.arange(M) * 37) % 6000  # includes 0 and values above 4096 once M > 111
    pos[-1] = 5003
    pos[0] = 0
    return pos


@pytest.mark.parametrize("heads", [(16, 8, 128), (4, 2, 64), (3, 1, 128)], ids=["16-8-128", "4-2-64", "3-1-128"])
@pytest.mark.parametrize("M", [5, 300, 4099])
def test_qknorm_ops_vs_fp64(M, heads):
    nH, nKV, hd = heads
    nQK, QKV = nH + nKV, (nH + 2 * nKV) * hd
    theta, eps = 10000.0, 1e-6
    x = rnd(M, QKV, seed=1, scale=1.5)
    x[:, :hd] *= 4.0  # one head at another scale: the statistic is per head
    wq, wk = (1 + 0.1 * rnd(hd, seed=2)).to(torch.bfloat16).float(), (1 + 0.1 * rnd(hd, seed=3)).to(torch.bfloat16).float()
    pos = _positions(M)
    want, rstd_ref = R.qknorm_rope_fwd_ref(x, wq, wk, pos, nH, nKV, hd, theta, eps)
    xd = torch.full((M + GUARD, QKV), SENT, dtype=torch.bfloat16, device="cuda")
    xd[:M] = x.to(torch.bfloat16).cuda()
    wqd, wkd, posd = dev_bf16(wq), dev_bf16(wk), pos.cuda()
    raw = _guarded(M, nQK * hd, torch.bfloat16)
    rstd = _guarded(M, nQK, torch.float32)
    tab = torch.empty(4 * M * (hd // 2), dtype=torch.float32, device="cuda")
    assert lib().slam_op_qknorm_rope_fwd(ptr(xd), ptr(wqd), ptr(wkd), ptr(posd), theta, eps, M, M, nH, nKV, hd, ptr(raw),
                                         ptr(rstd), ptr(tab), stream()) == 0
    sync()
    check(f"qknorm_rope_fwd {M} {heads}", xd[:M, :nQK * hd].float(), want[:, :nQK * hd], 3e-3, 1e-2)
    check("qknorm rstd", rstd[:M], rstd_ref, 1e-5)
    assert torch.equal(raw[:M].cpu().view(torch.int16), x[:, :nQK * hd].to(torch.bfloat16).view(torch.int16))  # the input bits
    assert torch.equal(xd[:M, nQK * hd:].cpu().view(torch.int16), x[:, nQK * hd:].to(torch.bfloat16).view(torch.int16))  # v untouched
    for t in (xd, raw, rstd):
        assert bool((t[M:] == SENT).all()), "canary rows written"
    # without the saved copies: the same output bits
    x2 = xd.clone()
    x2[:M] = x.to(torch.bfloat16).cuda()
    assert lib().slam_op_qknorm_rope_fwd(ptr(x2), ptr(wqd), ptr(wkd), ptr(posd), theta, eps, M, M, nH, nKV, hd, None, None,
                                         ptr(tab), stream()) == 0
    sync()
    assert torch.equal(x2.view(torch.int16), xd.view(torch.int16))

    # backward, in place on the q|k columns of dqkv
    dy = rnd(M, QKV, seed=4)
    dx_ref, dwq_ref, dwk_ref = R.qknorm_bwd_ref(dy[:, :nQK * hd], x[:, :nQK * hd], wq, wk, nH, nKV, hd, eps)
    nws = lib().slam_op_qknorm_bwd_workspace(M, nH, nKV, hd)
    assert nws > 0 and nws % 4 == 0
    outs = []
    for _ in range(2):
        dq = torch.full((M + GUARD, QKV), SENT, dtype=torch.bfloat16, device="cuda")
        dq[:M] = dy.to(torch.bfloat16).cuda()
        ws = torch.full((nws // 4 + GUARD,), SENT, dtype=torch.float32, device="cuda")
        ws[:nws // 4] = float("nan")
        dwq = torch.full((hd + GUARD,), SENT, dtype=torch.float32, device="cuda")
        dwk = torch.full((hd + GUARD,), SENT, dtype=torch.float32, device="cuda")
        dwq[:hd] = float("nan")
        dwk[:hd] = float("nan")
        assert lib().slam_op_qknorm_bwd(ptr(dq), ptr(raw), ptr(rstd), ptr(wqd), ptr(wkd), ptr(dwq), ptr(dwk), ptr(ws), M, nH, nKV,
                                        hd, stream()) == 0
        sync()
        assert bool((dq[M:] == SENT).all()) and bool((ws[nws // 4:] == SENT).all())
        assert bool((dwq[hd:] == SENT).all()) and bool((dwk[hd:] == SENT).all())
        outs.append((dq[:M].clone(), dwq[:hd].clone(), dwk[:hd].clone()))
    dq, dwq, dwk = outs[0]
    check("qknorm_bwd dx", dq[:, :nQK * hd].float(), dx_ref, 3e-3, 1e-2)
    check("qknorm_bwd dw_q", dwq, dwq_ref, 1e-5)
    check("qknorm_bwd dw_k", dwk, dwk_ref, 1e-5)
    assert torch.equal(dq[:, nQK * hd:].cpu().view(torch.int16), dy[:, nQK * hd:].to(torch.bfloat16).view(torch.int16))  # dv untouched
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), "backward is not bit-identical"

    # decode form: fp32 rows in, fp32 rows out
    B = min(M, 67)
    rows = torch.randn(B, QKV, generator=torch.Generator().manual_seed(6)) * 2
    rd = torch.full((B + GUARD, QKV), SENT, dtype=torch.float32, device="cuda")
    rd[:B] = rows.cuda()
    assert lib().slam_op_qknorm_rows_f32(ptr(rd), ptr(wqd), ptr(wkd), eps, B, nH, nKV, hd, stream()) == 0
    sync()
    check("qknorm_rows_f32", rd[:B], R.qknorm_rows_ref(rows, wq, wk, nH, nKV, hd, eps), 1e-6)
    assert torch.equal(rd[:B, nQK * hd:].cpu(), rows[:, nQK * hd:]) and bool((rd[B:] == SENT).all())


# --------------------------------------------------------------------------------------------------------------- model
def _unit_lm(tag, max_tokens=1024, layers=None, allocate_grads=True, **kw):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    cfg = dict(R.CFGS[tag])
    if layers:
        cfg["num_hidden_layers"] = layers
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=cfg, vocab_size=R.VOCAB, max_tokens=max_tokens, **kw), seed=7,
               allocate_grads=allocate_grads)
    sd = R.weights(cfg, R.SEED[tag])
    m.load_state_dict(sd)
    return m, cfg, sd


@pytest.fixture(scope="module")
def ref_grads():
    """qwen3_ref autograd on the shared batch, computed once per config."""
    out = {}
    ids, mask, labels, _ = R.batch()
    for tag in ("A", "B"):
        out[tag] = R.loss_and_grads(R.CFGS[tag], R.weights(R.CFGS[tag], R.SEED[tag]), ids, mask, labels)
    return out


@pytest.mark.parametrize("tag", ["A", "B"])
def test_model_matches_hf_golden_and_ref_autograd(tag, gold, ref_grads):
    m, cfg, sd = _unit_lm(tag)
    assert m.engine.arch == 3 and "layers.0.q_norm" in m.engine.tensors and "layers.0.bqkv" not in m.engine.tensors
    ids, mask, labels, lens = R.batch()
    out = m(ids, attention_mask=mask, labels=labels)
    torch.cuda.synchronize()
    got = out.logits.float().cpu()
    ref_logits, ref_loss, rg = ref_grads[tag]
    want = torch.from_numpy(gold[f"{tag}_logits"])
    o = 0
    for b, n in enumerate(lens):  # real tokens only
        check(f"logits row {b} vs HF golden", got[b, :n], want[o:o + n], 1.5e-2, 5e-2)
        check(f"logits row {b} vs qwen3_ref", got[b, :n], ref_logits[b, :n], 1.5e-2, 5e-2)
        o += n
    assert abs(float(out.loss) - float(gold[f"{tag}_loss"])) < 1e-2, (float(out.loss), float(gold[f"{tag}_loss"]))
    assert abs(float(out.loss) - float(ref_loss)) < 1e-2
    out2 = m(ids, attention_mask=mask, labels=labels, num_items_in_batch=150)
    assert abs(float(out2.loss) - float(R.loss_of(ref_logits, labels, 150))) < 1e-2
    m.zero_grad()
    m(ids, attention_mask=mask, labels=labels)
    m.backward()
    grads = dict(m.named_grads())
    names = [k for k, _ in R.hf_keys(cfg)]
    assert set(grads) == set(names)  # the HF parameter names (under `lm.`, tied head)
    gnorm = dict(zip(names, gold[f"{tag}_grad_norms"]))
    for k, g in grads.items():
        c = cosine(g, rg[k])
        ratio = float(g.double().norm()) / float(gnorm[k])
        print(f"[parity] grad {k}: cosine {c:.6f} |engine| / |HF| {ratio:.4f}")
        assert c >= (0.99 if g.dim() == 1 else 0.998), (k, c)
        assert 0.9 <= ratio <= 1.1, (k, ratio)
    for short, key in (("input_layernorm", "input_layernorm"), ("post_attention_layernorm", "post_attention_layernorm"),
                       ("q_norm", "self_attn.q_norm"), ("k_norm", "self_attn.k_norm")):
        c = cosine(grads[f"lm.model.layers.0.{key}.weight"], torch.from_numpy(gold[f"{tag}_grad_{short}"]))
        assert c >= 0.99, (short, c)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_packed_batch_and_log_likelihood(tag):
    m, cfg, sd = _unit_lm(tag)
    g = torch.Generator().manual_seed(9)
    seg = [70, 33, 90]
    toks = [torch.randint(2, R.VOCAB, (n,), generator=g) for n in seg]
    ids = torch.cat(toks)[None]
    pos = torch.cat([torch.arange(n) for n in seg])[None]
    labels = torch.cat([torch.cat([torch.tensor([-100]), t[1:]]) for t in toks])[None]
    out = m(ids, position_ids=pos, labels=labels, num_items_in_batch=sum(n - 1 for n in seg))
    total, o = 0.0, 0
    got = out.logits.float().cpu()[0]
    for t in toks:
        r = R.forward(cfg, sd, t[None])[0]
        check("packed logits", got[o:o + len(t)], r, 1.5e-2, 5e-2)
        total += float(F.cross_entropy(r[:-1], t[1:], reduction="sum"))
        o += len(t)
    assert abs(float(out.loss) - total / sum(n - 1 for n in seg)) < 1e-2
    ids2, mask2, _, lens2 = R.batch()
    logits = R.forward(cfg, sd, ids2, attention_mask=mask2).float()
    lp = logits[:, :-1].log_softmax(-1).gather(-1, ids2[:, 1:, None])[..., 0]
    want = torch.where(mask2[:, 1:] == 1, lp, torch.zeros_like(lp)).sum(1)
    for pf in (False, True):
        ll = m.log_likelihood(ids2, mean_nll=False, padding_free=pf).cpu()
        for b in range(3):
            assert abs(float(ll[b]) - float(want[b])) < 2e-2 * max(1.0, abs(float(want[b])) / 100), (pf, b, ll, want)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_recompute_levels_give_the_bits_of_level0(tag):
    m, cfg, sd = _unit_lm(tag, layers=5)  # five layers: the three shared slots wrap
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(2, R.VOCAB, (3, 96), generator=g)
    res = {}
    for two in (1, 0):
        m.engine.set_option("bwd_wgrad_stream", two)
        for level in (0, 1, 2, 0):
            if level:
                m.gradient_checkpointing_enable(level=level)
            else:
                m.gradient_checkpointing_disable()
            for rep in range(2):
                m.zero_grad()
                out = m(input_ids=ids, labels=ids)
                m.backward()
                sync()
                cur = (out.loss.detach().clone(), out.logits.clone(), m.flat_grads.clone())
                ref = res.setdefault(two, cur)
                for a, b, name in zip(ref, cur, ("loss", "logits", "grads")):
                    assert torch.equal(a, b), (tag, two, level, rep, name, int((a != b).sum()))
        assert float(res[two][2].abs().max()) > 0 and bool(torch.isfinite(res[two][2]).all())
        t = m.engine.tensors["layers.3.q_norm"]
        assert float(res[two][2][t.offset:t.offset + t.numel].abs().max()) > 0


@pytest.mark.parametrize("final", [0, 1, 2])
def test_grad_norm_clip_and_adamw(final):
    """slam_grad_norm equals the norm of named_grads under every final-value mode (q_norm / k_norm final-stored exactly once, in
    the image and in the norm partials); one clip-0.5 + AdamW step under the HF decay rule matches torch.optim.AdamW; the
    sharded-range update over cuts inside the norm vectors leaves the bits of the whole-buffer update."""
    m, cfg, sd = _unit_lm("A")
    ids, mask, labels, _ = R.batch()
    m.engine.set_option("grad_overwrite_next", 1)
    m(ids, attention_mask=mask, labels=labels)
    m.backward(final=final)
    norm = torch.zeros(2, dtype=torch.float32, device=m.device)
    m.engine.grad_norm(0.5, norm)
    torch.cuda.synchronize()
    grads = {k: g.detach().double().cpu().clone() for k, g in m.named_grads()}
    want = math.sqrt(sum(float(g.pow(2).sum()) for g in grads.values()))
    assert abs(float(norm[0]) - want) <= 1e-4 * want, (float(norm[0]), want)
    flags = m.hf_decay_flags()
    decayed = dict(zip(m.engine.tensors, flags))
    assert not decayed["layers.0.q_norm"] and not decayed["layers.1.k_norm"] and decayed["layers.0.wqkv"]
    m.engine.set_decay_mask(flags)
    w0 = {k: v.clone() for k, v in m.state_dict(torch.float32).items()}
    n = m.engine.n_params
    p0, t0, master0 = m.flat_params.clone(), m.flat_params_t.clone(), m.flat_master.clone()
    g0 = (m.flat_grads16 if final == 2 else m.flat_grads).clone()
    ea = torch.zeros(n, dtype=torch.float32, device=m.device)
    eq = torch.zeros(n, dtype=torch.float32, device=m.device)
    m.engine.adamw_step(m.flat_master, ea, eq, norm, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, zero_grad=False)
    torch.cuda.synchronize()
    after = m.state_dict(torch.float32)
    whole = (m.flat_params.clone(), m.flat_params_t.clone(), m.flat_master.clone(), ea.clone(), eq.clone())
    clip = min(1.0, 0.5 / (want + 1e-6))
    no_decay = {k for k in grads if k.endswith("norm.weight")}
    groups = [([k for k in grads if k not in no_decay], 0.1), (sorted(no_decay), 0.0)]
    for keys, wd in groups:
        params = [torch.nn.Parameter(w0[k].double()) for k in keys]
        for p, k in zip(params, keys):
            p.grad = grads[k] * clip
        torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd).step()
        for p, k in zip(params, keys):
            check(f"adamw {k}", after[k] - w0[k], (p.detach() - w0[k].double()).float(), 2e-2)
    # the same step as three ranges cut inside layer 0's q_norm and layer 1's k_norm
    m.flat_params.copy_(p0)
    m.flat_params_t.copy_(t0)
    m.flat_master.copy_(master0)
    (m.flat_grads16 if final == 2 else m.flat_grads).copy_(g0)
    ea.zero_()
    eq.zero_()
    c1 = m.engine.tensors["layers.0.q_norm"].offset + 12
    c2 = m.engine.tensors["layers.1.k_norm"].offset + 4
    for lo, hi in ((c2, n), (0, c1), (c1, c2)):
        m.engine.adamw_range(lo, hi - lo, m.flat_master, ea, eq, norm, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, zero_grad=False)
    m.engine.refresh_transposed()
    torch.cuda.synchronize()
    m.engine.set_decay_mask(None)
    for a, b, name in zip(whole, (m.flat_params, m.flat_params_t, m.flat_master, ea, eq),
                          ("params", "params_t", "master", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), (name, int((a != b).sum()))


def _norm_ranges(m):
    return [(t.offset, t.offset + t.numel) for n, t in m.engine.tensors.items() if n.endswith(("q_norm", "k_norm"))]


@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("first", [True, False], ids=["store", "accumulate"])
def test_final_backward_modes_equal_the_plain_backward(tag, first):
    """"grad_final_next" under its existing contract (tests/test_gpu_final_grads.py): final = 1 leaves the fp32 gradients of the
    plain backward bit for bit, final = 2 leaves their round-to-nearest-even bf16 image, and one AdamW step from either equals
    the step from the plain backward's gradients (rounded, for 2) - for the whole buffer and, named, for every q_norm / k_norm
    range (the two new colsum_finish_many launches: image, img_only, accumulate and sink slots). `first`: the backward stores
    ("grad_overwrite_next") or adds to gradients an earlier micro-batch left."""
    m, cfg, sd = _unit_lm(tag, layers=3)
    ids, mask, labels, _ = R.batch()
    g = torch.Generator().manual_seed(12)
    ids0 = torch.randint(2, R.VOCAB, (3, 100), generator=g)  # the earlier micro-batch of the accumulating case
    n = m.engine.n_params
    ranges = _norm_ranges(m)
    assert len(ranges) == 6
    p0, t0, w0 = m.flat_params.clone(), m.flat_params_t.clone(), m.flat_master.clone()
    m.enable_bf16_grads()

    def run(final, from_grads=None):
        """One backward in `final` mode, then clip (never active: the coefficient is exactly 1) + AdamW; from_grads: the step
        reads these fp32 gradients instead (a plain backward's buffer overwritten with them)."""
        m.flat_params.copy_(p0)
        m.flat_params_t.copy_(t0)
        m.flat_master.copy_(w0)
        m.flat_grads16.fill_(float("nan"))
        if first:
            m.engine.set_option("grad_overwrite_next", 1)
        else:
            m.engine.set_option("grad_overwrite_next", 1)
            m(ids0, labels=ids0)
            m.backward()
        m(ids, attention_mask=mask, labels=labels)
        m.backward(final=0 if from_grads is not None else final)
        if from_grads is not None:
            m.flat_grads.copy_(from_grads)
        norm = torch.zeros(2, dtype=torch.float32, device=m.device)
        m.engine.grad_norm(1e6, norm)
        ea = torch.zeros(n, dtype=torch.float32, device=m.device)
        eq = torch.zeros(n, dtype=torch.float32, device=m.device)
        m.engine.adamw_step(m.flat_master, ea, eq, norm, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, zero_grad=False)
        sync()
        assert float(norm[1]) == 1.0
        return dict(g32=m.flat_grads.clone(), g16=m.flat_grads16.clone(), norm=float(norm[0]), params=m.flat_params.clone(),
                    params_t=m.flat_params_t.clone(), master=m.flat_master.clone(), ea=ea, eq=eq)

    def same(a, b, keys, what):
        for k in keys:
            x, y = a[k], b[k]
            for lo, hi in ranges:
                assert torch.equal(x[lo:hi], y[lo:hi]), (tag, what, k, "q_norm / k_norm range", lo)
            assert torch.equal(x, y), (tag, what, k, int((x != y).sum()))

    state = ("params", "params_t", "master", "ea", "eq")
    plain = run(0)
    for lo, hi in ranges:
        assert float(plain["g32"][lo:hi].abs().max()) > 0
    f1 = run(1)
    same(plain, f1, ("g32",) + state, "final=1 vs plain")
    assert abs(f1["norm"] - plain["norm"]) <= 2e-6 * plain["norm"], (f1["norm"], plain["norm"])  # partials vs the chunked pass
    f2 = run(2)
    rounded = plain["g32"].to(torch.bfloat16)
    for lo, hi in ranges:
        assert torch.equal(f2["g16"][lo:hi], rounded[lo:hi]), (tag, "final=2 image, q_norm / k_norm range", lo)
    assert torch.equal(f2["g16"], rounded), int((f2["g16"] != rounded).sum())
    same(run(0, from_grads=rounded.float()), f2, state, "final=2 vs the step from the rounded plain gradients")


def test_bucket_ranges_cover_the_norm_vectors():
    """The bucketed backward (data parallel's callback) reports ranges that tile the buffer, with q_norm / k_norm final inside
    their layer's range by the time it is reported; its gradients are those of the plain backward."""
    m, cfg, sd = _unit_lm("A", layers=5)
    for k, v in (("gemm_tn_bal_bg_max_split", 8), ("gemm_tn224_bg_min_m", 1 << 30), ("gemm_nt224", 0)):
        m.engine.set_option(k, v)
    ids, mask, labels, _ = R.batch()
    m.zero_grad()
    m(ids, attention_mask=mask, labels=labels)
    m.backward()
    sync()
    plain = m.flat_grads.clone()
    seen = []
    m.zero_grad()
    m(ids, attention_mask=mask, labels=labels)
    m.backward(bucket_layers=2, bucket_cb=lambda off, cnt, st: seen.append((off, cnt)))
    sync()
    assert torch.equal(plain, m.flat_grads)
    assert sorted(seen)[0][0] == 0 and sum(c for _, c in seen) == m.engine.n_params
    ends = sorted((o, o + c) for o, c in seen)
    assert all(ends[i][1] == ends[i + 1][0] for i in range(len(ends) - 1))


def test_checkpoint_round_trip_fresh_init_and_untied_head(tmp_path):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    m, cfg, sd = _unit_lm("A")
    ids, mask, labels, _ = R.batch()
    loss0 = float(m(ids, attention_mask=mask, labels=labels).loss)
    m.save_pretrained(str(tmp_path / "ck"))
    c = json.load(open(tmp_path / "ck" / "config.json"))
    assert c["base_config"]["model_type"] == "qwen3" and c["base_config"]["head_dim"] == 128
    m2 = UnitLM.from_pretrained(str(tmp_path / "ck"))
    assert m2.engine.arch == 3
    assert float(m2(ids, attention_mask=mask, labels=labels).loss) == loss0
    # a fresh model: unit norms, the rest random
    f = UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(R.CFG_B), vocab_size=502, max_tokens=256), seed=1)
    fs = f.state_dict(torch.float32)
    assert bool((fs["lm.model.layers.0.self_attn.q_norm.weight"] == 1).all()) and float(fs["lm.model.layers.0.self_attn.q_proj.weight"].std()) > 0
    # the untied head works as with Qwen2
    u = UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(R.CFG_B), vocab_size=502, max_tokens=512,
                            tie_word_embeddings=False), seed=1)
    u.zero_grad()
    out = u(ids, attention_mask=mask, labels=labels)
    u.backward()
    sync()
    ug = dict(u.named_grads())
    assert math.isfinite(float(out.loss)) and float(ug["lm.lm_head.weight"].abs().max()) > 0
    assert float(ug["lm.model.layers.0.self_attn.k_norm.weight"].abs().max()) > 0


def test_twist_init_from_a_sharded_hf_qwen3_directory(tmp_path):
    """TWIST initialisation from a raw HF Qwen3 directory with a larger vocabulary, written here in several shards (the one
    test of this file that needs transformers to write its input)."""
    transformers = pytest.importorskip("transformers")
    from slamkit_amd.model import UnitLM, UnitLMConfig
    hc = transformers.Qwen3Config(vocab_size=600, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                  num_attention_heads=4, num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6,
                                  tie_word_embeddings=True, max_position_embeddings=4096, pad_token_id=0)
    hf = transformers.Qwen3ForCausalLM(hc).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, p in hf.named_parameters():
            if "q_norm" in k or "k_norm" in k:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    hf.save_pretrained(str(tmp_path / "text"), max_shard_size="1MB")
    assert os.path.exists(tmp_path / "text" / "model.safetensors.index.json")
    t = UnitLM(UnitLMConfig(base_model_name=str(tmp_path / "text"), vocab_size=502, twist_init=True, max_tokens=256))
    assert t.config.is_qwen3 and t.engine.arch == 3
    got, ref = t.state_dict(torch.float32), hf.state_dict()
    assert torch.equal(got["lm.model.embed_tokens.weight"], ref["model.embed_tokens.weight"][:502])
    for l in range(2):
        for k in ("q_norm", "k_norm"):
            assert torch.equal(got[f"lm.model.layers.{l}.self_attn.{k}.weight"], ref[f"model.layers.{l}.self_attn.{k}.weight"])
    assert torch.equal(got["lm.model.layers.1.mlp.up_proj.weight"], ref["model.layers.1.mlp.up_proj.weight"])


# ---------------------------------------------------------------------------------------------------------- generation
def _gen_model(tag, max_tokens=1024):
    return _unit_lm(tag, max_tokens=max_tokens, allocate_grads=False)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_decode_and_extend_match_forward(tag):
    """Teacher-forced slam_decode_step logits, and the same tokens through slam_extend in chunks of 7, against one forward and
    against qwen3_ref."""
    m, cfg, sd = _gen_model(tag)
    g = torch.Generator().manual_seed(3)
    lens, NEW = [37, 20, 5], 29
    B, T = len(lens), max(lens)
    full = torch.zeros(B, T + NEW, dtype=torch.long)
    for b, n in enumerate(lens):
        full[b, 0] = 1
        full[b, 1:n + NEW] = torch.randint(2, R.VOCAB, (n + NEW - 1,), generator=g)
    dev = m.device
    ids = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = full[b, :n]
    cap = 128
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    logits = torch.empty(B, R.VOCAB, dtype=torch.float32, device=dev)
    fwd = m(input_ids=full).logits.float().cpu()
    ref = R.forward(cfg, sd, full)

    def prefill():
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        m.engine.prefill(ids.to(dev).contiguous(), lens_d, B, T, logits)
        return lens_d, [logits.clone()]

    lens_d, steps = prefill()
    for k in range(NEW - 1):
        tok = torch.stack([full[b, lens[b] + k] for b in range(B)]).to(dev)
        m.engine.decode_step(tok, lens_d, B, logits)
        steps.append(logits.clone())
    sync()
    assert lens_d.tolist() == [n + NEW - 1 for n in lens]
    dec = torch.stack(steps, 1).cpu()
    for b, n in enumerate(lens):
        e1, e2 = rel_err(dec[b], fwd[b, n - 1:n - 1 + NEW]), rel_err(dec[b], ref[b, n - 1:n - 1 + NEW])
        print(f"[parity] {tag} row {b}: decode vs forward {e1:.3e}, vs qwen3_ref {e2:.3e}")
        assert e1 <= LOGITS_TOL and e2 <= LOGITS_TOL, (tag, b, e1, e2)
    # chunks of 7 through slam_extend: the logits of each chunk's last token
    lens_d, _ = prefill()
    CH = 7
    for c0 in range(0, NEW - 1, CH):
        chunk = torch.stack([full[b, lens[b] + c0:lens[b] + c0 + CH] for b in range(B)]).contiguous().to(dev)
        new = torch.full((B,), CH, dtype=torch.int32, device=dev)
        m.engine.extend(chunk, new, lens_d, B, CH, logits)
        sync()
        for b, n in enumerate(lens):
            p = n + c0 + CH - 1
            e = rel_err(logits[b].cpu(), fwd[b, p])
            assert e <= LOGITS_TOL, (tag, b, c0, "extend vs forward", e)
    assert lens_d.tolist() == [n + 28 for n in lens]


@pytest.mark.parametrize("tag", ["A", "B"])
def test_score_continuations_match_ref_log_softmax(tag):
    """slam_extend_score through UnitLM.score_continuations against qwen3_ref's log-softmax, at the bar of
    tests/test_gpu_score_model.py: 2 LOGITS_TOL rms(logits at the positions that predict the continuation)."""
    m, cfg, sd = _gen_model(tag)
    g = torch.Generator().manual_seed(4)
    P, TC = 12, 15
    ids = torch.randint(2, R.VOCAB, (3, P), generator=g)
    cont = torch.randint(2, R.VOCAB, (3, TC), generator=g)
    clen = torch.tensor([15, 9, 1])
    lp, am = m.score_continuations(ids, continuations=cont, continuation_lengths=clen, score_chunk=7, return_argmax=True)
    lp, am = lp.cpu(), am.cpu()
    lg = R.forward(cfg, sd, torch.cat([ids, cont], 1)).float()
    for r in range(3):
        c = int(clen[r])
        rows = lg[r, P - 1:P - 1 + c]
        want = rows.log_softmax(-1).gather(-1, cont[r, :c, None])[:, 0]
        bar = 2 * LOGITS_TOL * float(rows.pow(2).mean().sqrt())
        assert float((lp[r, :c] - want).abs().max()) <= bar, (tag, r, float((lp[r, :c] - want).abs().max()), bar)
        assert bool((lp[r, c:] == 0).all()) and bool((am[r, c:] == -1).all())
        top = rows.topk(2, -1).values
        clear = (top[:, 0] - top[:, 1]) > bar
        assert torch.equal(am[r, :c][clear], rows.argmax(-1)[clear])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_generate_matches_hf_golden(tag, gold):
    m, cfg, sd = _gen_model(tag, max_tokens=512)
    ids, am = torch.from_numpy(gold[f"{tag}_ids"]), torch.from_numpy(gold[f"{tag}_mask"])
    want = torch.from_numpy(gold[f"{tag}_seq"])
    margin = torch.from_numpy(gold[f"{tag}_margin"])
    eos = int(gold[f"{tag}_eos"])
    out = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(),
                     max_new_tokens=int(gold["max_new_tokens"]), eos_token_id=eos, pad_token_id=0).cpu()
    assert out.dtype == torch.int64 and out.shape == want.shape, (out.shape, want.shape)
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids)
    tol = 2 * LOGITS_TOL * float(gold[f"{tag}_score_rms"])
    new, wnew = out[:, T:], want[:, T:]
    for b in range(want.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else wnew.shape[1]  # steps before the first near-tie must agree exactly
        diff = (new[b] != wnew[b]).nonzero()
        first = int(diff[0]) if len(diff) else wnew.shape[1]
        hit = (wnew[b] == eos).nonzero()
        length = int(hit[0]) + 1 if len(hit) else wnew.shape[1]
        assert min(trust, length) >= 10  # the golden's own promise (make_golden_qwen3.py)
        assert first >= trust, (tag, b, "diverged at", first, "before the first near-tie", trust)
        if len(hit) and first >= length:
            assert (new[b, length:] == 0).all()
    # the chunked prefill gives the same tokens on the trusted steps
    out2 = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(),
                      max_new_tokens=int(gold["max_new_tokens"]), eos_token_id=eos, pad_token_id=0, prefill_chunk=16).cpu()
    assert torch.equal(out2[:, T:T + 10], want[:, T:T + 10])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_n_samples_equal_rows_sampled_alone(tag):
    m, cfg, sd = _gen_model(tag, max_tokens=512)
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(2, R.VOCAB, (2, 11), generator=g)
    kw = dict(do_sample=True, temperature=1.3, top_k=40, max_new_tokens=12, eos_token_id=[], seed=5, sampler="engine")
    sid = torch.tensor([40, 7, 19, 3, 1000003, 5])
    a = m.generate(ids, num_return_sequences=3, sample_ids=sid, **kw).cpu()
    assert a.shape == (6, 23)
    assert not all(torch.equal(a[0], a[i]) for i in (1, 2))
    for r in range(6):
        alone = m.generate(ids[r // 3:r // 3 + 1], sample_ids=sid[r:r + 1], **kw).cpu()
        assert torch.equal(alone[0], a[r]), (tag, r)
