"""Residual dropout (OPT, engine option "dropout_thr16") on the GPU: the two kernels against the numpy restatement
(tests/dropout_ref.py) element for element, the engine-backed UnitLM against HF OPTForCausalLM in fp32 with the restated masks
injected into HF's dropout calls, eval-mode bit identity, determinism, recomputation, the weight-gradient stream and a
resumed trainer run."""
import numpy as np
import pytest
import torch

from tests import dropout_ref as R
from tests.gpu_util import cosine, dev_bf16, lib, ptr, rnd, stream, sync

pytestmark = pytest.mark.gpu
try:
    import transformers
except ImportError:
    transformers = None
needs_hf = pytest.mark.skipif(transformers is None, reason="HF transformers provides the fp32 OPT reference")

P = 0.1
THR = R.thr16(P)  # 6554


def _bits(t):
    """uint16 bits of a bf16 tensor, as numpy."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _bf16_bits_of_f32(x):
    return _bits(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16))


# ----------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("index0", [0, (1 << 35) + 8], ids=["i0", "i2p35"])
@pytest.mark.parametrize("thr", [1, 6554, 32768, 65535])
@pytest.mark.parametrize("M,H", [(64, 64), (74, 256), (300, 768), (5, 2048)])
def test_ops_match_restatement(M, H, thr, index0):
    seed, call, sid = 0x1234_5678_9ABC_DEF0, 7, 3
    keep = R.keep_mask(M, H, thr, seed, call, sid, index0)
    iseed = seed - (1 << 64) if seed >= (1 << 63) else seed
    # backward with dy = 1: exactly 0 or bf16(scale) - the mask pattern itself
    dy = torch.ones(M, H, dtype=torch.bfloat16, device="cuda")
    dm = torch.full((M, H), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib().slam_op_dropout_bwd(ptr(dy), ptr(dm), M, H, thr, iseed, call, sid, index0, stream()) == 0
    sync()
    want = np.where(keep, _bf16_bits_of_f32(np.full((M, H), R.scale(thr), dtype=np.float32)), np.uint16(0))
    got = _bits(dm)
    assert (got == want).all(), f"{int((got != want).sum())} of {M * H} mask elements differ"
    assert bool((dy == 1).all())  # dy stays intact
    # a random gradient: one rounding of dy * scale
    g = rnd(M, H, seed=3)
    gd = dev_bf16(g)
    assert lib().slam_op_dropout_bwd(ptr(gd), ptr(dm), M, H, thr, iseed, call, sid, index0, stream()) == 0
    sync()
    assert (_bits(dm) == _bf16_bits_of_f32(R.dropout_bwd_f32(g.numpy(), keep, thr))).all()
    # forward, |y| >= 0.5. resid takes y's sign: a bound in ulps of the sum says something only where the sum does not cancel
    # (a contracted multiply-add moves the fp32 sum by up to 2^-24 |y scale|, which is far below a bf16 ulp of any sum that is
    # at least as large as its terms)
    y = rnd(M, H, seed=1)
    y = torch.where(y >= 0, y + 0.5, y - 0.5).to(torch.bfloat16).float()
    resid = rnd(M, H, seed=2).abs() * torch.sign(y)
    assert float(y.abs().min()) >= 0.5
    yd, rd = dev_bf16(y), dev_bf16(resid)
    assert lib().slam_op_dropout_add(ptr(yd), ptr(rd), M, H, thr, iseed, call, sid, index0, stream()) == 0
    sync()
    out = _bits(yd)
    rb = _bits(rd)
    assert (out[~keep] == rb[~keep]).all()  # dropped: resid's own bits
    ref = _bf16_bits_of_f32(R.dropout_add_f32(y.numpy(), resid.numpy(), keep, thr))
    ulps = np.abs(out.astype(np.int32) - ref.astype(np.int32))  # same sign, no cancellation: bit distance = ulps
    print(f"[parity] dropout_add {M}x{H} thr {thr}: kept {int(keep.sum())}, max ulp {int(ulps[keep].max()) if keep.any() else 0}, "
          f"off by one {int((ulps[keep] == 1).sum())}")
    assert (ulps[keep] <= 1).all()
    assert (ulps[keep] == 0).mean() > 0.99 if keep.any() else True  # a contraction changes a rounding rarely, not routinely


# ------------------------------------------------------------------------------------------------------------------- model
def _tiny(dropout=0.0, max_tokens=2048):
    from tests.test_gpu_opt import _perturb, _unit_lm
    return _perturb(_unit_lm(max_tokens=max_tokens, dropout=dropout) if dropout else _unit_lm(max_tokens=max_tokens))


def _grads(m):
    return {k: v.detach().float().cpu().clone() for k, v in m.named_grads()}


def _step(m, batch, seed=None, call=None):
    """zero_grad, one training forward + backward; (loss, gradients)."""
    ids, mask, labels = batch
    m.set_dropout_state(seed=seed, call=call)
    m.zero_grad()
    out = m(ids, attention_mask=mask, labels=labels, return_logits=False)
    m.backward()
    torch.cuda.synchronize()
    return float(out.loss), _grads(m)


@needs_hf
def test_eval_is_untouched():
    from tests.test_gpu_opt import _batch
    m0, m1 = _tiny(), _tiny(P)
    assert m1.config.dropout == P and m1._drop_thr == THR and m0._drop_thr == 0
    ids, mask, labels, _ = _batch()
    m1.eval()
    a, b = m0(ids, attention_mask=mask, labels=labels), m1(ids, attention_mask=mask, labels=labels)
    torch.cuda.synchronize()
    assert torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss)
    for mean in (False, True):
        assert torch.equal(m0.log_likelihood(ids, mean_nll=mean), m1.log_likelihood(ids, mean_nll=mean))
    m1.train()  # scoring never drops, whatever the mode; a training forward does
    assert torch.equal(m0.log_likelihood(ids, mean_nll=False), m1.log_likelihood(ids, mean_nll=False))
    c = m1(ids, attention_mask=mask, labels=labels)
    assert not torch.equal(a.loss, c.loss)
    m1.eval()  # ... and leaves nothing behind for the next forward
    d = m1(ids, attention_mask=mask, labels=labels)
    assert torch.equal(a.logits, d.logits) and torch.equal(a.loss, d.loss)
    # a forward the engine refuses uses the arming up as well: the next, unarmed one must not inherit it
    m1.engine.arm_dropout(4)
    assert lib().slam_forward(m1.engine.h, None, None, None, None, None, 3, 128, 0.0, None, None, None) == -1
    e = m1(ids, attention_mask=mask, labels=labels)
    assert torch.equal(a.logits, e.logits) and torch.equal(a.loss, e.loss)


def _hf_grads(hf, ids, mask, labels):
    from tests.test_gpu_opt import _ref_loss
    hf.zero_grad()
    loss = _ref_loss(hf(input_ids=ids, attention_mask=mask).logits, labels)
    loss.backward()
    return float(loss), {k: p.grad.detach().clone() for k, p in hf.named_parameters() if p.grad is not None}


def _cosines(tag, got, ref):
    """Per-tensor cosine of the engine's gradients against HF's; k_proj.bias (exactly zero in exact arithmetic) by its norm."""
    out = {}
    for k, g in got.items():
        r = ref[k[3:]]
        if k.endswith("k_proj.bias"):
            qb = ref[k[3:].replace("k_proj", "q_proj")]
            assert float((g - r).norm()) <= 0.1 * float(qb.norm()), k
            continue
        out[k] = cosine(g, r)
        print(f"[parity] {tag} grad {k}: cosine {out[k]:.6f}")
    return out


@needs_hf
def test_parity_with_hf_under_injected_masks(monkeypatch):
    from tests.test_gpu_opt import _batch, _hf_from
    ids, mask, labels, _ = _batch()
    B, T = ids.shape
    Tp = -(-T // 64) * 64  # the engine pads the token axis to a multiple of 64: its rows are b * Tp + t
    seed, call = 4321, 9
    # p = 0 in the same run: what bf16 against fp32 costs without dropout
    m0 = _tiny()
    hf = _hf_from(m0)
    loss0, g0 = _step(m0, (ids, mask, labels))
    ref_loss0, ref0 = _hf_grads(hf, ids, mask, labels)
    assert abs(loss0 - ref_loss0) < 1e-2
    cos0 = _cosines("p=0", g0, ref0)
    # p = 0.1: HF in train() with the restated masks in call order (layer 0 site 0, layer 0 site 1, layer 1 site 0, ...)
    m1 = _tiny(P)
    loss1, g1 = _step(m1, (ids, mask, labels), seed=seed, call=call)
    for layer in hf.model.decoder.layers:
        layer.dropout = P
    hf.train()
    n_calls = [0]
    real_dropout = torch.nn.functional.dropout

    def injected(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return real_dropout(x, p=p, training=training, inplace=inplace)
        assert abs(p - P) < 1e-12
        sid = n_calls[0]
        n_calls[0] += 1
        H = x.shape[-1]
        keep = R.keep_mask(B * Tp, H, THR, seed, call, sid).reshape(B, Tp, H)[:, :T]
        k = torch.from_numpy(np.ascontiguousarray(keep)).to(x.dtype)
        return (x.reshape(B, T, H) * k * float(R.scale(THR))).reshape(x.shape)

    monkeypatch.setattr(torch.nn.functional, "dropout", injected)
    ref_loss1, ref1 = _hf_grads(hf, ids, mask, labels)
    monkeypatch.undo()
    assert n_calls[0] == 2 * len(hf.model.decoder.layers)
    print(f"[parity] loss p=0: engine {loss0:.5f} hf {ref_loss0:.5f}; p={P}: engine {loss1:.5f} hf {ref_loss1:.5f}")
    assert abs(ref_loss1 - ref_loss0) > 1e-3  # the masks did something on the HF side
    assert abs(loss1 - ref_loss1) < 1e-2
    cos1 = _cosines(f"p={P}", g1, ref1)
    assert set(cos1) == set(cos0)
    for k in cos1:
        print(f"[parity] {k}: cosine p=0 {cos0[k]:.6f}, p={P} {cos1[k]:.6f}")
    for k in cos1:  # the margin covers the one extra bf16 rounding of y
        assert cos1[k] >= cos0[k] - 1e-3, (k, cos0[k], cos1[k])
    # power: the same engine gradients against HF WITHOUT masks are far off - this would pass for no engine that ignores dropout
    hf.eval()
    _, ref_eval = _hf_grads(hf, ids, mask, labels)
    for k in g1:
        if k.endswith("fc2.weight"):
            c = cosine(g1[k], ref_eval[k[3:]])
            print(f"[parity] {k} against HF eval(): cosine {c:.6f}")
            assert c < 0.99, (k, c)


@needs_hf
def test_same_seed_and_call_same_bits():
    from tests.test_gpu_opt import _batch
    ids, mask, labels, _ = _batch()
    b = (ids, mask, labels)
    m = _tiny(P)
    la, ga = _step(m, b, seed=11, call=5)
    _step(m, b, seed=11, call=6)  # something else in between
    lb, gb = _step(m, b, seed=11, call=5)
    assert la == lb
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    lc, _ = _step(m, b, seed=11, call=6)
    ld, _ = _step(m, b, seed=12, call=5)
    le, _ = _step(m, b, seed=11 + (1 << 32), call=5)  # the high half of the seed is part of the key
    assert len({la, lc, ld, le}) == 4
    # forward() counts up from the call it was given
    m.set_dropout_state(seed=11, call=5)
    m.zero_grad()
    l5 = float(m(ids, attention_mask=mask, labels=labels, return_logits=False).loss)
    l6 = float(m(ids, attention_mask=mask, labels=labels, return_logits=False).loss)
    assert (l5, l6) == (la, lc)


def _opt5(dropout=P, max_tokens=1024):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from tests.test_gpu_recompute import OPT5
    m = UnitLM(UnitLMConfig(base_model_name="local-opt", base_config=dict(OPT5), vocab_size=502, max_tokens=max_tokens,
                            dropout=dropout), seed=7)
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "layer_norm" in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


def _dense5():
    from tests.test_gpu_recompute import _dense
    d = _dense(502)
    return d["input_ids"], d["attention_mask"], d["labels"]


def test_recompute_levels_same_bits():
    """Five layers over three slots: levels 1 and 2 rebuild what the forward made - level 2 draws site 0's mask again."""
    b = _dense5()
    m = _opt5()
    l0, g0 = _step(m, b, seed=3, call=2)
    plain, _ = _step(_opt5(0.0), b)
    assert l0 != plain  # dropout is on
    for level in (1, 2):
        m.gradient_checkpointing_enable(level=level)
        l, g = _step(m, b, seed=3, call=2)
        assert l == l0, (level, l, l0)
        for k in g0:
            assert torch.equal(g[k], g0[k]), (level, k)


def test_wgrad_stream_same_bits():
    """The masked gradients are read on the weight-gradient stream after the caller's stream moved on: same bits as in order."""
    b = _dense5()
    m = _opt5()
    # the same K-split plans on both paths, as the other side-stream tests set them (tests/test_gpu_opt.py): the side stream's
    # "background" plans would otherwise move the fp32 summation order of the weight gradients, dropout or not
    m.engine.set_option("gemm_tn_bal_bg_max_split", 8)
    m.engine.set_option("gemm_tn224_bg_min_m", 1 << 30)
    m.engine.set_option("gemm_nt224", 0)
    res = []
    for two in (1, 0, 1):
        m.engine.set_option("bwd_wgrad_stream", two)
        res.append(_step(m, b, seed=3, call=2))
    for l, g in res[1:]:
        assert l == res[0][0]
        for k in g:
            assert torch.equal(g[k], res[0][1][k]), k


def test_trainer_resume_repeats_the_run(tmp_path):
    """GA 2, 4 optimizer steps with dropout; 2 steps + checkpoint + resume + 2 more: the same final loss and parameters."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    g = torch.Generator().manual_seed(1)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (40,), generator=g).tolist(), "attention_mask": [1] * 41} for _ in range(32)]
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)

    def run(out, resume=None, save_steps=0, dropout=P):
        m = _tiny(dropout, max_tokens=1024)
        a = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=2, max_steps=4, warmup_steps=1,
                                  warmup_ratio=0.0, logging_steps=1, save_steps=save_steps, output_dir=str(out),
                                  num_train_epochs=4, seed=13)
        tr = SLAMTrainer(model=m, args=a, data_collator=coll, train_dataset=ds)
        tr.train(resume_from_checkpoint=resume)
        return m, tr

    m_full, tr_full = run(tmp_path / "a", save_steps=2)
    m_res, tr_res = run(tmp_path / "b", resume=str(tmp_path / "a" / "checkpoint-2"))
    assert tr_res.state.global_step == 4
    lf = [h["loss"] for h in tr_full.state.log_history if "loss" in h]
    lr = [h["loss"] for h in tr_res.state.log_history if "loss" in h]
    assert lf[-1] == lr[-1] and lf[-2:] == lr[-2:]
    a, b = m_full.state_dict(torch.float32), m_res.state_dict(torch.float32)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    m_plain, tr_plain = run(tmp_path / "c", dropout=0.0)  # and dropout was part of that run
    assert [h["loss"] for h in tr_plain.state.log_history if "loss" in h][-1] != lf[-1]
