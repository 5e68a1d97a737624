"""GPT-NeoX (Pythia) decoder family on the GPU: the engine-backed UnitLM against HF GPTNeoXForCausalLM in float64 holding the
engine's bf16 weights; the fused LayerNorm pair against the two single launches, bit for bit; recomputation; refusals, the
checkpoint round trip and TWIST initialisation."""
import ctypes as C

import pytest
import torch
import transformers

from tests.gpu_util import check, cosine
from tests.test_gpu_opt import _batch, _ref_loss

pytestmark = pytest.mark.gpu


def _hf_cfg(hidden=256, n_heads=4, pct=0.25, tied=False, layers=2, inter=1024, vocab=502):
    return transformers.GPTNeoXConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, intermediate_size=inter,
                                      num_attention_heads=n_heads, rotary_pct=pct, max_position_embeddings=256, pad_token_id=0,
                                      bos_token_id=1, eos_token_id=1, tie_word_embeddings=tied, hidden_dropout=0.0,
                                      attention_dropout=0.0)


def _unit_lm(cfg, max_tokens=512):
    """The engine model of an HF config, LayerNorm weights and all biases perturbed by 0.05 N(0, 1) (HF's init: ones and zeros)."""
    from slamkit_amd.model import UnitLM, UnitLMConfig
    m = UnitLM(UnitLMConfig(base_model_name="local-tiny-neox", base_config=cfg.to_dict(), vocab_size=502, max_tokens=max_tokens),
               seed=7)
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "layernorm" in k or "layer_norm" in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


def _hf_from(m, cfg, dtype=torch.float64):
    """HF GPTNeoXForCausalLM on the CPU with exactly the engine's bf16 weights."""
    hf = transformers.GPTNeoXForCausalLM(cfg).to(dtype).eval()
    missing, unexpected = hf.load_state_dict({k[3:]: v.to(dtype) for k, v in m.state_dict(torch.bfloat16).items()}, strict=False)
    assert set(missing) <= {"lm_head.weight"} and not unexpected
    hf.tie_weights()
    return hf


def _run(m, **batch):
    m.zero_grad()
    out = m(**batch)
    m.backward()
    torch.cuda.synchronize()
    return out.logits.clone(), out.loss.clone(), {k: g.clone() for k, g in m.named_grads()}


@pytest.mark.parametrize("n_heads,head_dim,pct,tied", [(4, 64, 0.25, False), (2, 128, 0.25, False), (4, 64, 0.5, True),
                                                       (4, 64, 1.0, False)])
def test_neox_model_matches_hf_float64(n_heads, head_dim, pct, tied):
    cfg = _hf_cfg(n_heads * head_dim, n_heads, pct, tied)
    m = _unit_lm(cfg)
    hf = _hf_from(m, cfg)
    ids, mask, labels, lens = _batch()
    logits, loss, grads = _run(m, input_ids=ids, attention_mask=mask, labels=labels)
    ref = hf(input_ids=ids, attention_mask=mask)
    ref_loss = _ref_loss(ref.logits, labels)
    got = logits.float().cpu()
    for b, n in enumerate(lens):
        check(f"logits row {b}", got[b, :n], ref.logits[b, :n].detach(), 1.5e-2, 5e-2)
    assert abs(float(loss) - float(ref_loss.detach())) < 1e-2, (float(loss), float(ref_loss.detach()))
    ref_loss.backward()
    hfp = dict(hf.named_parameters())
    assert set(grads) == {"lm." + k for k in hfp if not (tied and k == "lm_head.weight")}
    for k, g in grads.items():  # HF's names and layout: query_key_value comes back in [n_heads][3][head_dim] rows
        c = cosine(g, hfp[k[3:]].grad)
        print(f"[parity] grad {k}: cosine {c:.6f}")
        assert c >= (0.99 if g.dim() == 1 else 0.998), (k, c)
    # the same rows as one packed batch: positions restart per segment, so every real position gives the padded run's logits
    m.padding_free = True
    packed = m(ids, attention_mask=mask, labels=labels).logits.float().cpu()
    for b, n in enumerate(lens):
        check(f"packed logits row {b}", packed[b, :n], ref.logits[b, :n].detach(), 1.5e-2, 5e-2)
        check(f"packed vs padded row {b}", packed[b, :n], got[b, :n], 1.5e-2, 5e-2)


@pytest.mark.parametrize("hidden,n_heads,M", [(256, 4, 178), (2048, 16, 130), (1024, 16, 64)])
def test_dual_layernorm_is_the_split_form_bit_for_bit(hidden, n_heads, M):
    wide = hidden == 2048
    m = _unit_lm(_hf_cfg(hidden, n_heads, layers=1 if wide else 2, inter=2048 if wide else 1024))
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(2, 502, (1, M), generator=g)
    batch = dict(input_ids=ids, labels=ids)
    if M == 178:  # three packed segments: the last block of rows is ragged
        batch["position_ids"] = torch.cat([torch.arange(n) for n in (100, 61, 17)])[None]
    runs = []
    for split in (0, 1):
        m.engine.set_option("neox_split_ln", split)
        runs.append(_run(m, **batch))
    (lg0, ls0, g0), (lg1, ls1, g1) = runs
    assert torch.equal(lg0, lg1) and torch.equal(ls0, ls1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_recompute_levels_give_level_0_bits():
    m = _unit_lm(_hf_cfg())
    ids, mask, labels, _ = _batch()
    p0 = m.flat_params.clone()
    pt0 = m.flat_params_t.clone()

    def run(level):
        m.gradient_checkpointing_enable(level) if level else m.gradient_checkpointing_disable()
        m.flat_params.copy_(p0)
        m.flat_params_t.copy_(pt0)
        m.engine.set_option("grad_overwrite_next", 1)
        m(ids, attention_mask=mask, labels=labels, return_logits=False)
        loss = m._loss_buf.clone()
        m.backward()
        norm = torch.zeros(2, device="cuda")
        m.engine.grad_norm(1.0, norm)
        grads = m.flat_grads.clone()
        ea, es = (torch.zeros(m.engine.n_params, dtype=torch.bfloat16, device="cuda") for _ in range(2))
        m.engine.adamw_step_bf16(ea, es, norm, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, zero_grad=False)
        torch.cuda.synchronize()
        return loss, grads, m.flat_params.clone()

    ref = run(0)
    for level in (1, 2):
        for i, (a, b) in enumerate(zip(ref, run(level))):
            assert torch.equal(a, b), (level, i)


def test_refusals_round_trip_and_twist_init(tmp_path):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.model.unit_lm import qkv_engine_to_hf
    cfg = _hf_cfg()
    m = _unit_lm(cfg)
    ids, mask, labels, _ = _batch()
    with pytest.raises(ValueError, match="GPT-NeoX"):
        m.generate(ids[:, :8], max_new_tokens=2)
    with pytest.raises(ValueError, match="GPT-NeoX"):
        m.score_continuations(ids[:1, :8], continuations=ids[:1, 8:12])
    lens = torch.full((3,), 8, dtype=torch.int32, device="cuda")
    out = torch.zeros(3, 502, device="cuda")
    rc = m.engine.lib.slam_prefill(m.engine.h, C.c_void_p(ids.cuda().data_ptr()), C.c_void_p(lens.data_ptr()), 3, 100,
                                   C.c_void_p(out.data_ptr()), None)
    assert rc == -1 and b"GPT-NeoX" in m.engine.lib.slam_last_error(m.engine.h)
    loss = float(m(ids, attention_mask=mask, labels=labels).loss)
    m.save_pretrained(str(tmp_path / "ckpt"))
    m2 = UnitLM.from_pretrained(str(tmp_path / "ckpt"), max_tokens=512)
    assert float(m2(ids, attention_mask=mask, labels=labels).loss) == loss
    # TWIST: a local HF text LM with a larger vocabulary, cut to 502 rows; query_key_value through the permutation
    big = _hf_cfg(vocab=640)
    hf = transformers.GPTNeoXForCausalLM(big).to(torch.bfloat16)
    hf.save_pretrained(str(tmp_path / "text_lm"), safe_serialization=True)
    tw = UnitLM(UnitLMConfig(base_model_name=str(tmp_path / "text_lm"), vocab_size=502, twist_init=True, max_tokens=512))
    sd = hf.state_dict()
    w = sd["gpt_neox.layers.1.attention.query_key_value.weight"]
    t = tw.engine.tensors["layers.1.wqkv"]
    flat = tw.flat_params[t.offset:t.offset + t.rows * t.cols].view(t.rows, t.cols).cpu()
    assert torch.equal(qkv_engine_to_hf(flat, 4, 64), w)
    assert torch.equal(flat[:256].view(4, 64, 256), w.view(4, 3, 64, 256)[:, 0])  # the engine's first H rows are the q heads
    assert torch.equal(tw.state_dict()["lm.gpt_neox.embed_in.weight"], sd["gpt_neox.embed_in.weight"][:502])
