"""OPT decoder family on the GPU: the new kernels through their slam_op_* entry points, and the engine-backed UnitLM against
HF OPTForCausalLM in fp32 (same bf16-representable weights) - logits, loss, gradients, packed batches, log-likelihood,
clipping and the optimizer step, checkpoints and the CLI."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import check, cosine, dev_bf16, lib, ptr, rnd, stream, sync

pytestmark = pytest.mark.gpu
try:
    import transformers
except ImportError:  # only the model-parity tests need it (HF OPT is their fp32 reference); the kernel tests do not
    transformers = None
needs_hf = pytest.mark.skipif(transformers is None, reason="HF transformers provides the fp32 OPT reference")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TINY = dict(vocab_size=502, hidden_size=256, num_hidden_layers=2, ffn_dim=512, num_attention_heads=4,
            max_position_embeddings=128, word_embed_proj_dim=256, pad_token_id=0, bos_token_id=1, eos_token_id=1,
            dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0, init_std=0.02)


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("M,H", [(5, 256), (300, 768), (4099, 2048), (8192, 768)])
def test_layernorm_fwd_bwd(M, H):
    x = (rnd(M, H, seed=1) + 0.5 * rnd(1, H, seed=5)).to(torch.bfloat16).float()  # an offset per column: the mean matters
    w, b = (1 + 0.1 * rnd(H, seed=2)).to(torch.bfloat16).float(), (0.1 * rnd(H, seed=6)).to(torch.bfloat16).float()
    dy, dres = rnd(M, H, seed=3), rnd(M, H, seed=4)
    xd, wd, bd = dev_bf16(x), dev_bf16(w), dev_bf16(b)
    y = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
    mean = torch.empty(M, dtype=torch.float32, device="cuda")
    rstd = torch.empty(M, dtype=torch.float32, device="cuda")
    assert lib().slam_op_layernorm_fwd(ptr(xd), ptr(wd), ptr(bd), ptr(y), ptr(mean), ptr(rstd), M, H, 1e-5, stream()) == 0
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = F.layer_norm(xr, (H,), wr, br, 1e-5)
    sync()
    check(f"layernorm_fwd {M}x{H}", y.float(), yr.detach(), 3e-3, 1e-2)
    check("layernorm mean", mean.cpu(), x.mean(-1), 1e-6)
    check("layernorm rstd", rstd.cpu(), torch.rsqrt(x.var(-1, unbiased=False) + 1e-5), 1e-5)
    yr.backward(dy)
    ws = torch.empty(lib().slam_op_layernorm_bwd_workspace(M, H) // 4 + 16, dtype=torch.float32, device="cuda")
    dx = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
    dw = torch.full((H,), 7.0, dtype=torch.float32, device="cuda")
    db = torch.full((H,), 7.0, dtype=torch.float32, device="cuda")
    dyd, dresd = dev_bf16(dy), dev_bf16(dres)
    for use_res in (False, True):
        assert lib().slam_op_layernorm_bwd(ptr(dyd), ptr(xd), ptr(wd), ptr(mean), ptr(rstd), ptr(dresd) if use_res else None,
                                           ptr(dx), ptr(dw), ptr(db), ptr(ws), M, H, stream()) == 0
        sync()
        check(f"layernorm_bwd dx res={use_res}", dx.float(), xr.grad + (dres if use_res else 0), 3e-3, 1e-2)
        check("layernorm_bwd dw", dw, wr.grad, 1e-5)
        check("layernorm_bwd db", db, br.grad, 1e-5)


# M = 8192 (8 x 1024 tokens): fc1 of OPT-125m and of the OPT-1.3B step - both take the 256 x 256 tile kernel; the others
# the 128 x 128 kernels
@pytest.mark.parametrize("M,F_,H", [(8192, 3072, 768), (8192, 8192, 2048), (1000, 8192, 2048), (300, 512, 256)])
def test_relu_ffn_fwd_and_backward(M, F_, H, mf32):
    X, W1, b1 = rnd(M, H, seed=1), rnd(F_, H, seed=2, scale=0.05), rnd(F_, seed=3, scale=0.5)
    Xd, W1d, b1d = dev_bf16(X), dev_bf16(W1), dev_bf16(b1)
    act = torch.full((M, F_), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib().slam_op_gemm_nt_relu(ptr(Xd), ptr(W1d), ptr(act), ptr(b1d), M, F_, H, stream()) == 0
    sync()
    pre = Xd.float() @ W1d.float().t() + b1d.float()  # fp32 reference on the device (the big shapes)
    check(f"fc1 relu {M}x{F_}x{H} mf32={mf32}", act.float(), pre.clamp_min(0), 4e-3, 2e-2)
    assert bool((act.float() >= 0).all())
    del pre
    # backward through the stored activation: fused into the fc2 dgrad (transposed image W2^T [F][H]) and elementwise
    dY, W2 = rnd(M, H, seed=4), rnd(H, F_, seed=5, scale=0.05)
    dYd, W2t = dev_bf16(dY), dev_bf16(W2.t().contiguous())
    mask = act.float() > 0
    ref = (dYd.float() @ W2t.float().t()) * mask
    dact = torch.full((M, F_), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib().slam_op_gemm_nt_drelu(ptr(dYd), ptr(W2t), ptr(dact), ptr(act), M, F_, H, stream()) == 0
    sync()
    check("fc2 dgrad + relu bwd (fused)", dact.float(), ref, 4e-3, 2e-2)
    assert bool((dact.float()[~mask] == 0).all())
    del ref
    # the same GEMM on the same (one-block-per-tile) kernel plus the elementwise pass: the fused epilogue's bits
    plain = torch.full((M, F_), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib().slam_set_option(None, b"gemm_256_persist", 0) == 0
    try:
        assert lib().slam_op_gemm_nt(ptr(dYd), ptr(W2t), ptr(plain), None, None, M, F_, H, 1, stream()) == 0
    finally:
        lib().slam_set_option(None, b"gemm_256_persist", 1)
    assert lib().slam_op_relu_bwd(ptr(plain), ptr(act), M * F_, stream()) == 0
    sync()
    assert torch.equal(plain, dact)


@pytest.mark.parametrize("packed", [False, True])
def test_embed_pos_fwd_and_position_grad(packed):
    M, H, V, T, npos = 700, 256, 502, 350, 130
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, V, (M,), generator=g)
    pos = torch.cat([torch.arange(300), torch.arange(128), torch.arange(272)]) if packed else None
    E_, P_ = rnd(512, H, seed=1), rnd(npos, H, seed=2)
    Ed, Pd = dev_bf16(E_), dev_bf16(P_)
    idd = ids.cuda()
    pd = pos.cuda() if packed else None
    out = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
    prow = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    assert lib().slam_op_embed_pos_fwd(ptr(idd), ptr(pd), ptr(Ed), ptr(Pd), ptr(out), ptr(prow), M, H, V, T, npos, stream()) == 0
    sync()
    # both indices are clamped to their tables (the packed case has positions past the 128-row table)
    assert torch.equal(prow.cpu(), (pos if packed else torch.arange(M) % T).add(2).clamp(max=npos - 1))
    ref = (E_[ids] + P_[(pos if packed else torch.arange(M) % T).add(2).clamp(max=npos - 1)]).to(torch.bfloat16)
    assert torch.equal(out.cpu(), ref)  # one rounding of the fp32 sum
    # the position gradient is the token-ordered scatter by row (no padding row): index_add, bit-identical run to run
    dh = rnd(M, H, seed=3)
    dhd = dev_bf16(dh)
    ws = torch.empty(lib().slam_op_embed_bwd_workspace(M, npos), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        dP = torch.zeros(npos, H, dtype=torch.float32, device="cuda")
        assert lib().slam_op_embed_bwd(ptr(prow), ptr(dhd), ptr(dP), M, H, npos, npos, -1, ptr(ws), stream()) == 0
        sync()
        outs.append(dP.cpu())
    want = torch.zeros(npos, H, dtype=torch.float64).index_add_(0, prow.cpu(), dh.double())
    check("position grad", outs[0], want, 1e-6)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("seg_lens", [[512], [37, 100, 5, 130, 64, 176]])
def test_attention_mha_12_heads(seg_lens):
    """OPT-125m's attention: 12 query heads and 12 K/V heads (G = 1), dense and packed."""
    from tests.test_gpu_ops import _attn_case, _attn_prescale, _attn_ref
    nH = nKV = 12
    hd = 64
    M, ld, qkv, seg_s, seg_e = _attn_case(seg_lens, nH, nKV, seed=3, spike=False, hd=hd)
    d_o = rnd(M, nH * hd, seed=9)
    qkv_dev, qkv = _attn_prescale(qkv, nH, hd)
    o_ref, dqkv_ref = _attn_ref(qkv, seg_s, nH, nKV, d_o, hd=hd)
    qd = dev_bf16(qkv_dev)
    o = torch.full((M, nH * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(nH * M, dtype=torch.float32, device="cuda")
    ss, se = seg_s.cuda(), seg_e.cuda()
    assert lib().slam_op_attn_fwd(ptr(qd), ptr(o), ptr(lse), ptr(ss), M, nH, nKV, hd, stream()) == 0
    sync()
    check(f"attn fwd 12/12 {seg_lens}", o.float(), o_ref, 6e-3, 3e-2)
    ws = torch.empty(lib().slam_op_attn_bwd_workspace(M, nH, hd) // 4 + 16, dtype=torch.float32, device="cuda")
    dqkv = torch.full((M, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
    dod = dev_bf16(d_o)
    assert lib().slam_op_attn_bwd(ptr(qd), ptr(o), ptr(dod), ptr(lse), ptr(dqkv), ptr(ws), ptr(ss), ptr(se),
                                  M, nH, nKV, hd, stream()) == 0
    sync()
    check("attn bwd 12/12", dqkv.float().cpu(), dqkv_ref, 1.5e-2, 6e-2)


# --------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(params=[0, 1], ids=["mf16", "mf32"])
def mf32(request):
    """Both MFMA shapes of the tile kernels (GemmTune::mf32): epilogue8 and epilogue32 carry the ReLU paths."""
    assert lib().slam_set_option(None, b"gemm_mf32", request.param) == 0
    yield request.param
    lib().slam_set_option(None, b"gemm_mf32", 0)


def _hf_cfg():
    return transformers.OPTConfig(**TINY)


def _unit_lm(max_tokens=2048, **kw):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    return UnitLM(UnitLMConfig(base_model_name="local-tiny-opt", base_config=_hf_cfg().to_dict(), vocab_size=502,
                               max_tokens=max_tokens, **kw), seed=7)


def _perturb(m):
    """Non-trivial LayerNorm / bias values (HF's init has unit norms and zero biases), bf16-representable."""
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "layer_norm" in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


def _hf_from(m):
    """HF OPTForCausalLM in fp32 with exactly the engine's bf16 weights."""
    hf = transformers.OPTForCausalLM(_hf_cfg()).float().eval()
    sd = {k[3:]: v.float() for k, v in m.state_dict(torch.bfloat16).items()}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert set(missing) <= {"lm_head.weight"} and not unexpected
    hf.tie_weights()
    return hf


def _batch():
    g = torch.Generator().manual_seed(5)
    B, T = 3, 100
    ids = torch.randint(2, 502, (B, T), generator=g)
    lens = [100, 61, 17]
    mask = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    ids = ids.masked_fill(mask == 0, 0)
    labels = ids.masked_fill(mask == 0, -100)
    return ids, mask, labels, lens


def _ref_loss(logits, labels, num_items=None):
    lg, lb = logits[:, :-1].reshape(-1, logits.shape[-1]).float(), labels[:, 1:].reshape(-1)
    if num_items:
        return F.cross_entropy(lg, lb, ignore_index=-100, reduction="sum") / num_items
    return F.cross_entropy(lg, lb, ignore_index=-100)


@needs_hf
def test_opt_model_matches_hf_fp32():
    m = _perturb(_unit_lm())
    hf = _hf_from(m)
    ids, mask, labels, lens = _batch()
    out = m(ids, attention_mask=mask, labels=labels)
    ref = hf(input_ids=ids, attention_mask=mask)
    ref_loss = _ref_loss(ref.logits, labels)
    torch.cuda.synchronize()
    got = out.logits.float().cpu()
    for b, n in enumerate(lens):  # real tokens only (HF sends right-pad positions elsewhere; the engine ignores the mask)
        check(f"logits row {b}", got[b, :n], ref.logits[b, :n].detach(), 1.5e-2, 5e-2)
    assert abs(float(out.loss) - float(ref_loss)) < 1e-2, (float(out.loss), float(ref_loss))
    # num_items_in_batch: sum / num_items
    out2 = m(ids, attention_mask=mask, labels=labels, num_items_in_batch=150)
    assert abs(float(out2.loss) - float(_ref_loss(ref.logits, labels, 150))) < 1e-2
    # gradients of every tensor
    m.zero_grad()
    m(ids, attention_mask=mask, labels=labels)
    m.backward()
    ref_loss.backward()
    hfp = dict(hf.named_parameters())
    grads = dict(m.named_grads())
    assert set(grads) == {"lm." + k for k in hfp if k != "lm_head.weight"}
    # per-tensor cosine >= 0.998 (>= 0.99 for the small bias / LayerNorm vectors): the first layer's gradients, behind two
    # layers of bf16 backward, measure 0.9989 - 0.9993 against fp32 HF (the Qwen2 golden tests use 0.999 on another init)
    for k, g in grads.items():
        r = hfp[k[3:]].grad
        if k.endswith("k_proj.bias"):  # exactly zero in exact arithmetic (a constant key shift leaves each softmax row unchanged)
            qb = hfp[k[3:].replace("k_proj", "q_proj")].grad
            print(f"[parity] grad {k}: |engine| {float(g.norm()):.3e} |hf| {float(r.norm()):.3e} |q bias grad| {float(qb.norm()):.3e}")
            assert float((g.cpu() - r).norm()) <= 0.1 * float(qb.norm()), k
            continue
        c = cosine(g, r)
        print(f"[parity] grad {k}: cosine {c:.6f}")
        bar = 0.99 if g.dim() == 1 else 0.998
        assert c >= bar, (k, c)
    # position rows no token uses get no gradient (the batch's rows are 0..99 + 2)
    assert float(grads["lm.model.decoder.embed_positions.weight"][102:].abs().max()) == 0.0


@needs_hf
def test_opt_packed_batch_and_log_likelihood():
    m = _perturb(_unit_lm())
    hf = _hf_from(m)
    g = torch.Generator().manual_seed(9)
    seg = [70, 33, 90]
    toks = [torch.randint(2, 502, (n,), generator=g) for n in seg]
    ids = torch.cat(toks)[None]
    pos = torch.cat([torch.arange(n) for n in seg])[None]
    labels = torch.cat([torch.cat([torch.tensor([-100]), t[1:]]) for t in toks])[None]
    out = m(ids, position_ids=pos, labels=labels, num_items_in_batch=sum(n - 1 for n in seg))
    total, o = 0.0, 0
    got = out.logits.float().cpu()[0]
    for t in toks:
        r = hf(input_ids=t[None]).logits[0].detach()
        check("packed logits", got[o:o + len(t)], r, 1.5e-2, 5e-2)
        total += float(F.cross_entropy(r[:-1], t[1:], reduction="sum"))
        o += len(t)
    assert abs(float(out.loss) - total / sum(n - 1 for n in seg)) < 1e-2
    # log_likelihood with and without ignore_tokens (right-padded rows, pad 0)
    ids2, mask2, _, lens2 = _batch()
    for ignore in (None, [3, 4, 5, 200]):
        ll = m.log_likelihood(ids2, mean_nll=False, ignore_tokens=ignore).cpu()
        logits = hf(input_ids=ids2, attention_mask=mask2).logits.detach().float()
        if ignore:
            logits[:, :, ignore] = float("-inf")
        lp = logits[:, :-1].log_softmax(-1).gather(-1, ids2[:, 1:, None])[..., 0]
        valid = mask2[:, 1:] == 1
        want = torch.where(valid, lp, torch.zeros_like(lp)).sum(1)
        for b in range(3):
            if ignore and bool(torch.isin(ids2[b, 1:lens2[b]], torch.tensor(ignore)).any()):
                assert not math.isfinite(float(ll[b]))
            else:
                assert abs(float(ll[b]) - float(want[b])) < 2e-2 * max(1.0, abs(float(want[b])) / 100), (b, ll, want)


@needs_hf
@pytest.mark.parametrize("final", [0, 1, 2])
def test_opt_grad_norm_clip_and_adamw(final):
    """slam_grad_norm equals the norm of named_grads under every final-value mode (every tensor final-stored exactly once,
    in the image and in the norm partials); one clip-0.5 + AdamW step matches torch.optim.AdamW on those gradients."""
    m = _perturb(_unit_lm())
    ids, mask, labels, _ = _batch()
    m.engine.set_option("grad_overwrite_next", 1)
    m(ids, attention_mask=mask, labels=labels)
    m.backward(final=final)
    norm = torch.zeros(2, dtype=torch.float32, device=m.device)
    m.engine.grad_norm(0.5, norm)
    torch.cuda.synchronize()
    grads = {k: g.detach().double().cpu().clone() for k, g in m.named_grads()}
    want = math.sqrt(sum(float(g.pow(2).sum()) for g in grads.values()))
    assert abs(float(norm[0]) - want) <= 1e-4 * want, (float(norm[0]), want)
    # a key-ordered step: every padded / unused element of the flat buffer has a zero gradient
    w0 = {k: v.clone() for k, v in m.state_dict(torch.float32).items()}
    n = m.engine.n_params
    ea = torch.zeros(n, dtype=torch.float32, device=m.device)
    eq = torch.zeros(n, dtype=torch.float32, device=m.device)
    m.engine.adamw_step(m.flat_master, ea, eq, norm, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1)
    after = m.state_dict(torch.float32)
    clip = min(1.0, 0.5 / (want + 1e-6))
    params = [torch.nn.Parameter(w0[k].double()) for k in grads]
    for p, k in zip(params, grads):
        p.grad = grads[k] * clip
    torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1).step()
    for p, k in zip(params, grads):
        check(f"adamw {k}", after[k] - w0[k], (p.detach() - w0[k].double()).float(), 2e-2)


@needs_hf
def test_opt_bucket_ranges_and_wgrad_stream_bit_identical():
    ids, mask, labels, _ = _batch()
    res = {}
    for two in (0, 1):
        m = _perturb(_unit_lm())
        m.engine.set_option("bwd_wgrad_stream", two)
        # the same K-split plans on both paths (as the Qwen2 test does): the side stream's "background" plans only move fp32
        # summation order
        m.engine.set_option("gemm_tn_bal_bg_max_split", 8)
        m.engine.set_option("gemm_tn224_bg_min_m", 1 << 30)
        m.engine.set_option("gemm_nt224", 0)
        seen = []
        m.zero_grad()
        m(ids, attention_mask=mask, labels=labels)
        m.backward(bucket_layers=1, bucket_cb=lambda off, cnt, *_: seen.append((off, cnt)))
        torch.cuda.synchronize()
        res[two] = m.flat_grads.clone()
        # the reported ranges tile the flat gradient buffer, top layers first
        seen.sort()
        assert seen[0][0] == 0 and sum(c for _, c in seen) == m.engine.n_params
        assert all(a + c == b for (a, c), (b, _) in zip(seen, seen[1:]))
    assert torch.equal(res[0], res[1])


@needs_hf
def test_opt_checkpoints_twist_and_generate(tmp_path):
    from slamkit_amd.model import UnitLM
    m = _perturb(_unit_lm())
    ids, mask, labels, _ = _batch()
    loss0 = float(m(ids, attention_mask=mask, labels=labels).loss)
    m.save_pretrained(str(tmp_path / "ck"))
    cfg = json.load(open(tmp_path / "ck" / "config.json"))
    assert cfg["base_config"]["model_type"] == "opt"
    m2 = UnitLM.from_pretrained(str(tmp_path / "ck"))
    assert float(m2(ids, attention_mask=mask, labels=labels).loss) == loss0
    # TWIST init from a raw HF OPT text-LM directory (model.decoder.* keys, a larger vocabulary cut to 502 rows)
    big = dict(TINY, vocab_size=600)
    hf = transformers.OPTForCausalLM(transformers.OPTConfig(**big)).eval()
    hf.save_pretrained(str(tmp_path / "text"))
    from slamkit_amd.model import UnitLMConfig
    t = UnitLM(UnitLMConfig(base_model_name=str(tmp_path / "text"), vocab_size=502, twist_init=True, max_tokens=2048))
    sd = t.state_dict(torch.float32)
    ref = hf.state_dict()
    assert torch.equal(sd["lm.model.decoder.embed_tokens.weight"], ref["model.decoder.embed_tokens.weight"][:502])
    assert torch.equal(sd["lm.model.decoder.embed_positions.weight"], ref["model.decoder.embed_positions.weight"])
    assert torch.equal(sd["lm.model.decoder.layers.1.fc2.bias"], ref["model.decoder.layers.1.fc2.bias"])
    with pytest.raises(ValueError):
        m.generate(ids[:, :5], max_new_tokens=2)


@needs_hf
def test_cli_train_gslm_on_example_tokens(golden_data, tmp_path):
    """The reference's GSLM recipe body (OPT-125m) through cli/train.py."""
    from slamkit_amd.cli.train import main
    from tests.test_gpu_train import _write_tokens
    p = tmp_path / "tokens.jsonl"
    _write_tokens(golden_data, p)
    out = tmp_path / "run"
    state = main([f"data.train_path={p}", f"data.val_path={p}", "model=gslm", "model.context_len=512",
                  "training_args.per_device_train_batch_size=2", "training_args.num_train_epochs=12",
                  "training_args.warmup_steps=2", "training_args.warmup_ratio=0", "training_args.logging_steps=1",
                  "training_args.eval_strategy=no", "training_args.learning_rate=1e-3",
                  f"training_args.output_dir={out}"])
    logs = [r for r in state.log_history if "loss" in r]
    assert state.global_step == 12 and len(logs) == 12
    assert all(math.isfinite(r["loss"]) for r in logs)
    assert logs[-1]["loss"] < logs[0]["loss"] - 0.5, [r["loss"] for r in logs]
    assert abs(logs[0]["loss"] - math.log(502)) < 0.3
    from safetensors.torch import load_file
    sd = load_file(os.path.join(out, "final", "model.safetensors"))
    hf = transformers.OPTForCausalLM(transformers.OPTConfig(vocab_size=502, hidden_size=768, num_hidden_layers=12, ffn_dim=3072,
                                                            num_attention_heads=12, word_embed_proj_dim=768))
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"lm." + k: tuple(v.shape) for k, v in hf.state_dict().items()
                                                          if k != "lm_head.weight"}


def _golden():
    import numpy as np
    return dict(np.load(os.path.join(GOLDEN, "opt_model.npz")))


def test_opt_reference_checkpoint_matches_golden():
    """A checkpoint written by the reference's UnitLM.save_pretrained over OPT (tests/golden/make_golden_opt.py: serialised
    OPTConfig under base_config, lm.model.decoder.* keys) loads and reproduces the reference's fp32 outputs: logits of the
    real tokens, loss (mean and num_items), per-tensor gradient norms, log_likelihood with and without ignore_tokens."""
    from slamkit_amd.model import UnitLM
    g = _golden()
    m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_opt_ckpt"), max_tokens=512)
    assert m.config.is_opt and m.engine.tensors["pos_embed"].rows == 130
    ids, mask, labels = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels"))
    m.zero_grad()
    out = m(ids, attention_mask=mask, labels=labels)
    m.backward()
    torch.cuda.synchronize()
    got = out.logits.float().cpu()
    for b in range(ids.shape[0]):
        n = int(mask[b].sum())
        check(f"reference checkpoint logits row {b}", got[b, :n], torch.from_numpy(g["logits"][b, :n]), 2e-2)
    assert abs(float(out.loss) - float(g["loss"])) <= 2e-2, (float(out.loss), float(g["loss"]))
    grads = dict(m.named_grads())
    for k, want in zip(g["grad_names"], g["grad_norms"]):
        k = str(k)
        if k.endswith("k_proj.bias"):  # zero in exact arithmetic (softmax is invariant to a constant key shift)
            continue
        got_n = float(grads[k].norm())
        assert abs(got_n - want) <= 3e-2 * want + 1e-7, (k, got_n, want)
    out2 = m(ids, attention_mask=mask, labels=labels, num_items_in_batch=100)
    assert abs(float(out2.loss) - float(g["loss_num_items"])) <= 2e-2
    for key, ignore in (("ll", None), ("ll_ignore", [3, 4, 5, 200])):
        ll = m.log_likelihood(ids, mean_nll=False, ignore_tokens=ignore).cpu()
        want = torch.from_numpy(g[key])
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(ll), fin), (key, ll, want)
        assert float((ll[fin] - want[fin]).abs().max()) <= 2e-2 * max(1.0, float(want[fin].abs().max()) / 100), (key, ll, want)


def test_opt_twist_init_and_raw_text_lm_match_golden():
    """TWIST initialisation from the tiny reference-side OPT text LM (640-row vocabulary cut to 502), and the same directory
    loaded as a raw OPT checkpoint through from_pretrained: both reproduce the reference's TWIST loss."""
    from slamkit_amd.model import UnitLM, UnitLMConfig
    g = _golden()
    ids, mask, labels = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels"))
    text = os.path.join(GOLDEN, "hf_opt_text_lm")
    tw = UnitLM(UnitLMConfig(base_model_name=text, vocab_size=502, twist_init=True, max_tokens=512))
    loss = float(tw(ids, attention_mask=mask, labels=labels).loss)
    assert abs(loss - float(g["twist_loss"])) <= 2e-2, (loss, float(g["twist_loss"]))
    raw = UnitLM.from_pretrained(text, vocab_size=502, max_tokens=512)
    assert float(raw(ids, attention_mask=mask, labels=labels).loss) == loss
    with pytest.raises(ValueError, match="max_position_embeddings"):
        raw.log_likelihood(torch.ones(1, 200, dtype=torch.int64), mean_nll=False)  # 200 > 128 positions
    with pytest.raises(ValueError, match="max_position_embeddings"):
        raw.sequence_logps(torch.ones(1, 200, dtype=torch.int64), torch.ones(1, 200, dtype=torch.int64))
    with pytest.raises(ValueError, match="position_ids"):
        raw(torch.ones(1, 64, dtype=torch.int64), position_ids=torch.arange(100, 164, device="cuda")[None])


def test_opt_overwrite_mode_zeroes_unused_position_rows():
    """First micro-batch of a step (grad_overwrite_next): the position table's gradient is STORED - rows the batch does not
    use come out zero even when the previous step left values there - and the whole gradient equals a fresh accumulation."""
    from slamkit_amd.model import UnitLM
    m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_opt_ckpt"), max_tokens=512)
    g = torch.Generator().manual_seed(3)
    long_ids = torch.randint(2, 502, (2, 120), generator=g)
    short_ids = torch.randint(2, 502, (2, 40), generator=g)
    row = m.engine.tensors["pos_embed"]
    m.zero_grad()
    m(long_ids, labels=long_ids)
    m.backward()
    torch.cuda.synchronize()
    pg = m.flat_grads[row.offset:row.offset + row.numel].view(row.rows, row.cols)
    assert float(pg[42:122].abs().max()) > 0  # the previous step used positions 0..119 (rows 2..121)
    m.engine.set_option("grad_overwrite_next", 1)
    m(short_ids, labels=short_ids)
    m.backward()
    torch.cuda.synchronize()
    stored = m.flat_grads.clone()
    assert float(pg[42:].abs().max()) == 0.0 and float(pg[:2].abs().max()) == 0.0
    m.zero_grad()
    m(short_ids, labels=short_ids)
    m.backward()
    torch.cuda.synchronize()
    assert torch.equal(stored, m.flat_grads)
