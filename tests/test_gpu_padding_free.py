"""-m gpu: padding-free execution of right-padded batches (slam_forward_unpadded, UnitLM.padding_free,
SLAMTrainingArguments.padding_free): the pack kernel bit for bit against tests/unpad_ref.py, then the model, log-likelihood,
DPO, recomputation and trainer paths at the bars tests/test_gpu_model.py and tests/test_gpu_opt.py apply to the same fixtures
on the padded path (loss abs <= 2e-2, logits rel-RMS <= 2e-2, gradient cosine >= 0.999 / 0.99)."""
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import unpad_ref as R
from tests.gpu_util import check, cosine, sync

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------ pack kernel
def _pack_case(name, golden_npz):
    g = torch.Generator().manual_seed(3)
    if name == "golden":
        ids, lab = torch.from_numpy(golden_npz["pad_ids"]), torch.from_numpy(golden_npz["pad_labels"])
        return ids, lab, golden_npz["pad_mask"].sum(1).tolist(), None
    B, T, lens, Mp = {"tail26": (3, 64, [64, 1, 37], None), "no_tail": (2, 64, [64, 64], None), "one_row": (1, 37, [37], None),
                      "long_tail": (3, 64, [64, 1, 37], 192),
                      # more rows than one 256-row scan chunk, more tokens than one block, odd T
                      "many_rows": (300, 7, torch.randint(1, 8, (300,), generator=g).tolist(), None)}[name]
    ids = torch.randint(1, 502, (B, T), generator=g)
    return ids, torch.randint(1, 502, (B, T), generator=g), lens, Mp


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("name", ["tail26", "no_tail", "one_row", "golden", "long_tail", "many_rows"])
def test_pack_kernel_equals_unpad_ref(name, with_labels, golden_npz):
    ids, lab, lens, Mp = _pack_case(name, golden_npz)
    B, T = ids.shape
    ref = R.pack(ids.numpy(), lab.numpy() if with_labels else None, lens, Mp)
    Mp = len(ref["ids"])
    assert Mp == {"tail26": 128, "no_tail": 128, "one_row": 64, "golden": 64, "long_tail": 192}.get(name, Mp)
    nbytes = E.unpadded_scratch_bytes(B, T)
    raw = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    off = (-raw.data_ptr()) % 256
    scratch = raw[off:off + nbytes]
    E.unpad_pack(ids.cuda(), lab.cuda() if with_labels else None, torch.tensor(lens, dtype=torch.int32).cuda(), B, T, Mp, 0, scratch)
    sync()
    v = {k: t.cpu().numpy() for k, t in E.unpadded_scratch_views(scratch, B, T).items()}
    for k in ("ids", "position_ids", "seg_start", "seg_end", "row"):
        assert np.array_equal(v[k][:Mp], ref[k]), k
    assert np.array_equal(v["off"], ref["off"])
    untouched = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]
    if with_labels:
        assert np.array_equal(v["labels"][:Mp], ref["labels"])
    else:
        assert (v["labels"] == untouched).all()  # without labels the array is left alone
    assert (v["ids"][Mp:] == untouched).all() and (raw[:off] == 0xA5).all() and (raw[off + nbytes:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------------ Qwen2, golden batch
@pytest.fixture(scope="module")
def tiny(golden_data, golden_npz):
    """The tiny Qwen2 model of tests/test_gpu_model.py, its golden padded batch (2 x 37, lengths 37 / 23) and the oracle's
    loss / logits / gradients for it - computed once, shared, never modified."""
    from tests.test_gpu_model import _mk
    meta = golden_data["meta"]
    cfg = O.OracleConfig(**meta["config"])
    sd = O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"])
    sd_bf = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    ids, am, lab = (torch.from_numpy(golden_npz[k]) for k in ("pad_ids", "pad_mask", "pad_labels"))
    ref = O.forward_loss_grads(cfg, sd_bf, ids, lab, attention_mask=am)
    return dict(cfg=cfg, sd_bf=sd_bf, m=_mk(cfg, sd), ids=ids, am=am, lab=lab, ref=ref)


def _grad_bars(named_grads, grads_ref, big=0.999, small_bar=0.99):
    worst = 1.0
    for k, gv in named_grads:
        ref = grads_ref[k]
        c = cosine(gv, ref)
        worst = min(worst, c)
        small = k.endswith(".bias") or k.endswith("norm.weight")
        assert c >= (small_bar if small else big), f"{k}: cosine {c:.5f}"
        assert abs(float(gv.norm()) / float(ref.norm()) - 1) <= 3e-2, k
    print("worst gradient cosine", worst)


def test_qwen2_golden_batch_padding_free(tiny, golden_npz):
    m, ids, am, lab, g = tiny["m"], tiny["ids"], tiny["am"], tiny["lab"], golden_npz
    loss_ref, logits_ref, grads_ref = tiny["ref"]
    valid = am.bool()

    def run(**kw):
        m.zero_grad()
        out = m(input_ids=ids, attention_mask=am, labels=lab, padding_free=True, **kw)
        tokens = m.engine.last_forward_tokens()
        m.backward()
        sync()
        return out.loss.detach().clone(), out.logits.clone(), m.flat_grads.clone(), tokens

    loss, logits, grads, tokens = run()
    assert tokens == 64  # 37 + 23 = 60 real tokens -> 64, where the padded path runs 2 x 64 = 128
    lg = logits.float().cpu()
    assert lg.shape == (2, 37, tiny["cfg"].vocab)
    check("logits vs reference golden (fp32 HF)", lg[valid], torch.from_numpy(g["pad_logits"])[valid], 2e-2)
    check("logits vs oracle (same bf16 weights)", lg[valid], logits_ref[valid], 2e-2)
    assert float(lg[~valid].abs().max()) == 0.0 and int((~valid).sum()) == 14  # pad positions are exactly zero
    print("loss engine / golden / oracle:", float(loss), float(g["pad_loss_mean"]), float(loss_ref))
    assert abs(float(loss) - float(g["pad_loss_mean"])) <= 2e-2
    assert abs(float(loss) - float(loss_ref)) <= 5e-3
    _grad_bars(m.named_grads(), grads_ref)
    E_ = m.flat_grads[: 512 * tiny["cfg"].hidden].view(512, tiny["cfg"].hidden)
    assert float(E_[tiny["cfg"].vocab:].abs().max()) == 0.0
    # a repeated run: the same bits
    loss2, logits2, grads2, _ = run()
    assert torch.equal(loss, loss2) and torch.equal(logits, logits2) and torch.equal(grads, grads2)
    # reduction "sum" with num_items_in_batch
    n = int(g["pad_num_items"])
    out = m(input_ids=ids, attention_mask=am, labels=lab, num_items_in_batch=n, padding_free=True, return_logits=False)
    assert out.logits is None and abs(float(out.loss.detach()) - float(g["pad_loss_sum"])) <= 2e-2
    # lengths instead of a mask, the model-wide switch instead of the argument, and the autograd surface
    m.padding_free = True
    try:
        m.zero_grad()
        out = m(input_ids=ids.cuda(), attention_mask=am.cuda(), labels=lab.cuda(), lengths=[37, 23])
        assert m.engine.last_forward_tokens() == 64
        out.loss.backward()
        sync()
        assert torch.equal(out.loss.detach(), loss) and torch.equal(out.logits, logits) and torch.equal(m.flat_grads, grads)
    finally:
        m.padding_free = False


def test_padded_path_is_kept_without_host_lengths(tiny):
    m, ids, am, lab = tiny["m"], tiny["ids"], tiny["am"], tiny["lab"]
    # off by default
    m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False)
    assert m.padding_free is False and m.engine.last_forward_tokens() == 128
    # a device mask without lengths is not read back: B x T (rounded up to 64) tokens
    m(input_ids=ids.cuda(), attention_mask=am.cuda(), labels=lab.cuda(), padding_free=True, return_logits=False)
    assert m.engine.last_forward_tokens() == 128
    # no mask and no lengths: nothing to go by
    m(input_ids=ids, labels=lab, padding_free=True, return_logits=False)
    assert m.engine.last_forward_tokens() == 128
    # a batch that carries position_ids (the flattening collator's) is untouched
    pos = torch.arange(37)[None].expand(2, 37).contiguous()
    m(input_ids=ids, attention_mask=am, position_ids=pos, labels=lab, padding_free=True, return_logits=False)
    assert m.engine.last_forward_tokens() == 74  # (dense rows with positions are not rounded up either: 2 x 37)
    # a left-padded host mask still raises, with the switch on or off
    for pf in (False, True):
        with pytest.raises(ValueError, match="right-padded"):
            m(input_ids=ids, attention_mask=am.flip(1), labels=lab, padding_free=pf)
    with pytest.raises(ValueError, match="host"):
        m(input_ids=ids, labels=lab, padding_free=True, lengths=torch.tensor([37, 23]).cuda())
    with pytest.raises(ValueError, match="row lengths"):
        m(input_ids=ids, labels=lab, padding_free=True, lengths=[38, 23])
    sync()


def test_state_errors(tiny):
    m, ids, am, lab = tiny["m"], tiny["ids"], tiny["am"], tiny["lab"]
    B, T = ids.shape
    f32 = lambda: torch.empty(B, dtype=torch.float32, device="cuda")  # noqa: E731
    m(input_ids=ids, attention_mask=am, labels=lab, padding_free=True, return_logits=False)
    held = m._hold
    with pytest.raises(E.EngineError, match="unpadded"):
        m.engine.seq_loglik(held[1], B, T, f32(), f32())
    with pytest.raises(E.EngineError, match="unpadded"):
        m.engine.seq_loglik(held[1], 1, 64, f32(), f32())  # not by the packed shape either
    with pytest.raises(E.EngineError, match="unpadded"):
        m.engine.scale_loss_rows(f32(), B, T)
    with pytest.raises(E.EngineError, match="matching"):
        m.engine.seq_loglik_unpadded(B + 1, f32(), f32())
    m.engine.seq_loglik_unpadded(B, f32(), f32())
    m.engine.scale_loss_unpadded(torch.ones(B, device="cuda"), B)
    # without labels there are no row losses to sum
    m(input_ids=ids, attention_mask=am, padding_free=True)
    with pytest.raises(E.EngineError, match="with labels"):
        m.engine.seq_loglik_unpadded(B, f32(), f32())
    # after a padded forward the unpadded calls are refused
    m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False)
    with pytest.raises(E.EngineError, match="unpadded forward"):
        m.engine.seq_loglik_unpadded(B, f32(), f32())
    with pytest.raises(E.EngineError, match="unpadded forward"):
        m.engine.scale_loss_unpadded(torch.ones(B, device="cuda"), B)
    sync()


@pytest.mark.parametrize("vocab", [504, 640])
def test_logits_in_16_byte_chunks_when_vocab_is_a_multiple_of_8(vocab):
    """vocab % 8 == 0 takes the 16-byte form of the logits kernel (502 takes the element form): 504 is the one-wave loss
    path (512 padded columns), 640 the large-vocabulary one (768). Rows of length T, 1 and in between. At the real positions
    the logits are BIT for bit those of the same tokens run as a packed [1, sum] row with position_ids (the same arrays,
    the same launches); against the padded path they meet the logits bar; pad positions are exactly zero."""
    from tests.test_gpu_model import _mk
    cfg = O.OracleConfig(n_layers=2, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, intermediate=512, vocab=vocab)
    m = _mk(cfg, O.init_weights(cfg, seed=4, bias_std=0.02, norm_jitter=0.05), max_tokens=512)
    g = torch.Generator().manual_seed(8)
    B, T, lens = 4, 48, [48, 1, 29, 8]
    ids = torch.randint(2, vocab, (B, T), generator=g)
    am = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).long()
    ids = ids * am
    lab = torch.where(am.bool(), ids, torch.full_like(ids, -100))
    out = m(input_ids=ids, attention_mask=am, labels=lab, padding_free=True)
    assert m.engine.last_forward_tokens() == 128  # 86 real tokens
    pf, pf_loss = out.logits.clone(), float(out.loss.detach())
    assert pf.shape == (B, T, vocab)
    valid = am.bool()
    assert float(pf.float().cpu()[~valid].abs().max()) == 0.0
    p = R.pack(ids.numpy(), lab.numpy(), lens)
    S = sum(lens)
    row = lambda k: torch.from_numpy(p[k][:S])[None]  # noqa: E731
    packed = m(input_ids=row("ids"), position_ids=row("position_ids"), labels=row("labels"))
    assert m.engine.last_forward_tokens() == 128
    want = torch.from_numpy(R.unpack_rows(packed.logits[0].view(torch.int16).cpu().numpy(), p["off"], B, T)).view(torch.bfloat16)
    assert torch.equal(pf.cpu(), want) and float(packed.loss.detach()) == pf_loss
    padded = m(input_ids=ids, attention_mask=am, labels=lab)
    assert m.engine.last_forward_tokens() == 192
    check(f"logits vs the padded path, vocab {vocab}", pf.float().cpu()[valid], padded.logits.float().cpu()[valid], 2e-2)
    assert abs(float(padded.loss.detach()) - pf_loss) <= 2e-2


def test_bucket_callback_padding_free(tiny):
    """The bucket callback of backward (data parallel) behind an unpadded forward: the reported ranges tile the flat
    gradient back to front and the gradients are the bits of the backward without a callback."""
    m, ids, am, lab = tiny["m"], tiny["ids"], tiny["am"], tiny["lab"]

    def run(cb):
        m.zero_grad()
        m(input_ids=ids, attention_mask=am, labels=lab, padding_free=True, return_logits=False)
        assert m.engine.last_forward_tokens() == 64
        m.backward(1.0, 1 if cb else 0, cb)
        sync()
        return m.flat_grads.clone()

    plain = run(None)
    got = []
    with_cb = run(lambda off, cnt, stream: got.append((off, cnt)))
    n = m.engine.n_params
    assert len(got) >= 2 and got[0][0] + got[0][1] == n and got[-1][0] == 0
    for (o1, c1), (o2, c2) in zip(got, got[1:]):
        assert o2 + c2 == o1 and c1 > 0 and c2 > 0
    assert torch.equal(plain, with_cb)


# ---------------------------------------------------------------------------------------------------------------- OPT
HF_OPT_KEYS = ("vocab_size", "hidden_size", "num_hidden_layers", "ffn_dim", "num_attention_heads", "max_position_embeddings",
               "word_embed_proj_dim", "pad_token_id", "bos_token_id", "eos_token_id", "dropout", "attention_dropout",
               "activation_dropout", "layerdrop", "init_std", "activation_function", "do_layer_norm_before", "enable_bias",
               "layer_norm_elementwise_affine")


try:
    import transformers
except ImportError:  # only the HF comparison needs it; everything else here has its own references
    transformers = None
needs_hf = pytest.mark.skipif(transformers is None, reason="HF transformers provides the fp32 OPT reference")


def _opt_golden_step(padding_free=True):
    """The reference-written OPT checkpoint on its golden 3 x 64 batch (lengths 64 / 41 / 17): model, output, gradients."""
    from slamkit_amd.model import UnitLM
    g = dict(np.load(os.path.join(GOLDEN, "opt_model.npz")))
    m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_opt_ckpt"), max_tokens=512)
    ids, mask, labels = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels"))
    m.padding_free = padding_free
    m.zero_grad()
    out = m(ids, attention_mask=mask, labels=labels)
    tokens = m.engine.last_forward_tokens()
    m.backward()
    sync()
    return g, m, (ids, mask, labels), out, {k: v.clone() for k, v in m.named_grads()}, tokens


def test_opt_golden_batch_padding_free():
    """tests/test_gpu_opt.py::test_opt_reference_checkpoint_matches_golden, padding-free: the reference's fp32 logits, loss,
    gradient norms and log-likelihoods of the 3 x 64 batch (lengths 64 / 41 / 17 -> 128 packed tokens); and every gradient
    tensor against the padded step from the same state at the bars of the Qwen2 golden-batch test (cosine >= 0.999 for
    matrices, >= 0.99 for bias / norm vectors, norm ratio within 3e-2)."""
    g, m, (ids, mask, labels), out, grads, tokens = _opt_golden_step()
    assert tokens == 128  # 122 real tokens, where the padded path runs 192
    got = out.logits.float().cpu()
    for b in range(3):
        n = int(mask[b].sum())
        check(f"reference checkpoint logits row {b}", got[b, :n], torch.from_numpy(g["logits"][b, :n]), 2e-2)
        assert n == 64 or float(got[b, n:].abs().max()) == 0.0
    assert abs(float(out.loss.detach()) - float(g["loss"])) <= 2e-2, (float(out.loss.detach()), float(g["loss"]))
    for k, want in zip(g["grad_names"], g["grad_norms"]):
        k = str(k)
        if k.endswith("k_proj.bias"):  # zero in exact arithmetic (softmax is invariant to a constant key shift)
            continue
        got_n = float(grads[k].norm())
        assert abs(got_n - want) <= 3e-2 * want + 1e-7, (k, got_n, want)
    out2 = m(ids, attention_mask=mask, labels=labels, num_items_in_batch=100)
    assert abs(float(out2.loss.detach()) - float(g["loss_num_items"])) <= 2e-2
    for key, ignore in (("ll", None), ("ll_ignore", [3, 4, 5, 200])):
        ll = m.log_likelihood(ids, mean_nll=False, ignore_tokens=ignore).cpu()
        assert m.engine.last_forward_tokens() == 128
        want = torch.from_numpy(g[key])
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(ll), fin), (key, ll, want)
        assert float((ll[fin] - want[fin]).abs().max()) <= 2e-2 * max(1.0, float(want[fin].abs().max()) / 100), (key, ll, want)
    # the position rows no token uses get no gradient: the packed positions are each row's own 0 .. len - 1
    assert float(grads["lm.model.decoder.embed_positions.weight"][66:].abs().max()) == 0.0
    # gradient directions: the padded step from the same state
    m.padding_free = False
    m.zero_grad()
    outp = m(ids, attention_mask=mask, labels=labels)
    assert m.engine.last_forward_tokens() == 192
    m.backward()
    sync()
    padded = {k: v.clone() for k, v in m.named_grads()}
    assert abs(float(outp.loss.detach()) - float(out.loss.detach())) <= 2e-2
    kb = [k for k in grads if k.endswith("k_proj.bias")]  # noise around zero in both runs: bounded by the q bias gradient
    for k in kb:
        qn = float(padded[k.replace("k_proj", "q_proj")].norm())
        assert float((grads[k] - padded[k]).norm()) <= 0.1 * qn, k
    _grad_bars([(k, v) for k, v in grads.items() if k not in kb], padded)


@needs_hf
def test_opt_golden_batch_padding_free_grads_vs_hf_fp32():
    """Every gradient tensor of the padding-free step against HF OPTForCausalLM in fp32 on the same bf16 weights, at the
    bars of tests/test_gpu_opt.py::test_opt_model_matches_hf_fp32 (>= 0.998 matrices, >= 0.99 vectors)."""
    import json
    g, m, (ids, mask, labels), out, grads, tokens = _opt_golden_step()
    assert tokens == 128
    with open(os.path.join(GOLDEN, "ref_opt_ckpt", "config.json")) as f:
        bc = json.load(f)["base_config"]
    hf = transformers.OPTForCausalLM(transformers.OPTConfig(**{k: bc[k] for k in HF_OPT_KEYS})).float().eval()
    missing, unexpected = hf.load_state_dict({k[3:]: v.float() for k, v in m.state_dict(torch.bfloat16).items()}, strict=False)
    assert set(missing) <= {"lm_head.weight"} and not unexpected
    hf.tie_weights()
    lg = hf(input_ids=ids, attention_mask=mask).logits
    torch.nn.functional.cross_entropy(lg[:, :-1].reshape(-1, 502).float(), labels[:, 1:].reshape(-1), ignore_index=-100).backward()
    hfp = dict(hf.named_parameters())
    for k, gv in grads.items():
        r = hfp[k[3:]].grad
        if k.endswith("k_proj.bias"):
            qb = hfp[k[3:].replace("k_proj", "q_proj")].grad
            assert float((gv.cpu() - r).norm()) <= 0.1 * float(qb.norm()), k
            continue
        c = cosine(gv, r)
        assert c >= (0.99 if gv.dim() == 1 else 0.998), (k, c)


def test_opt_dropout_is_reproducible_padding_free():
    """Two armed forwards with the same call number draw the same masks over the packed layout: forward and gradients are
    bit-identical; another call number is another mask; eval mode has none."""
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base = dict(model_type="opt", num_hidden_layers=2, hidden_size=256, num_attention_heads=4, ffn_dim=512,
                max_position_embeddings=128, init_std=0.02)
    m = UnitLM(UnitLMConfig(base_model_name="local-opt", base_config=base, vocab_size=502, max_tokens=512, dropout=0.1), seed=7)
    g = dict(np.load(os.path.join(GOLDEN, "opt_model.npz")))
    ids, mask, labels = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels"))
    m.padding_free = True

    def run(call, train=True):
        m.train(train)
        m.set_dropout_state(seed=1234, call=call)
        m.zero_grad()
        out = m(ids, attention_mask=mask, labels=labels)
        assert m.engine.last_forward_tokens() == 128
        m.backward()
        sync()
        return out.loss.detach().clone(), out.logits.clone(), m.flat_grads.clone()

    a, b, c, e = run(5), run(5), run(6), run(5, train=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[1], c[1]) and not torch.equal(a[2], c[2])
    assert not torch.equal(a[1], e[1])
    assert all(bool(torch.isfinite(t.float()).all()) for t in a)


# ------------------------------------------------------------------------------------------------------ log-likelihoods
@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_log_likelihood_padding_free(tiny, golden_npz, device):
    m, cfg, ids = tiny["m"], tiny["cfg"], tiny["ids"]
    tok = ids.to(device)
    for mean_nll, key in ((True, "ll_mean"), (False, "ll_sum")):
        ll = m.log_likelihood(tok, mean_nll, padding_free=True).cpu().numpy()
        assert m.engine.last_forward_tokens() == 64
        assert np.allclose(ll, golden_npz[key], rtol=5e-3, atol=2e-2), (key, ll, golden_npz[key])
    present = set(ids.flatten().tolist())
    ignore = [t for t in range(50, cfg.vocab) if t not in present][:200]
    got = m.log_likelihood(tok, False, ignore_tokens=ignore, padding_free=True).cpu().numpy()
    ref = O.log_likelihood(cfg, tiny["sd_bf"], ids.clone(), False, ignore_tokens=ignore).numpy()
    assert np.allclose(got, ref, rtol=5e-3, atol=0.3), (got, ref)
    bad = m.log_likelihood(tok, False, ignore_tokens=[int(ids[0, 3])], padding_free=True).cpu().numpy()
    assert np.isneginf(bad[0])
    again = m.log_likelihood(tok, False, padding_free=True).cpu().numpy()  # the mask is reset afterwards
    assert np.allclose(again, golden_npz["ll_sum"], rtol=5e-3, atol=2e-2)


def test_sequence_logps_padding_free(tiny, golden_npz):
    m, cfg, ids, lab = tiny["m"], tiny["cfg"], tiny["ids"], tiny["lab"]
    ll0, cnt0 = (t.clone() for t in m.sequence_logps(ids, lab))
    assert m.engine.last_forward_tokens() == 74  # the padded path: 2 x 37 positions
    ll, cnt = (t.clone() for t in m.sequence_logps(ids, lab, padding_free=True, lengths=[37, 23]))
    assert m.engine.last_forward_tokens() == 64
    assert torch.equal(cnt, cnt0) and cnt.tolist() == [36.0, 22.0]
    ref = O.log_likelihood(cfg, tiny["sd_bf"], ids.clone(), False).numpy()
    print("sequence_logps padding-free / padded / oracle:", ll.tolist(), ll0.tolist(), ref.tolist())
    assert np.allclose(ll.cpu().numpy(), ref, rtol=5e-3, atol=2e-2)
    assert np.allclose(ll.cpu().numpy(), golden_npz["ll_sum"], rtol=5e-3, atol=2e-2)
    # host ids without lengths: taken from pad_token_id; device ids without lengths: the padded path
    ll2, _ = m.sequence_logps(ids, lab, padding_free=True)
    assert m.engine.last_forward_tokens() == 64 and torch.equal(ll2, ll)
    m.sequence_logps(ids.cuda(), lab.cuda(), padding_free=True)
    assert m.engine.last_forward_tokens() == 74


# ---------------------------------------------------------------------------------------------------------------- DPO
def test_dpo_step_padding_free_vs_padded():
    """One SLAMDPOTrainer.optimizer_step from the same state, padded and padding-free: the same loss within 2e-2 and every
    gradient tensor (taken before the update) at the bars of the golden-batch test."""
    from slamkit_amd.tokeniser import UnitTokeniser
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer
    from tests.test_gpu_dpo import _model, _pairs
    cfg, n = O.TINY, 4
    sd_pol, sd_ref = O.init_weights(cfg, seed=11, bias_std=0.02), O.init_weights(cfg, seed=12, bias_std=0.02)
    res = {}
    for pf in (False, True):
        pol, ref = _model(sd_pol, 16 * 256, cfg), _model(sd_ref, 16 * 256, cfg)
        args = DPOConfig(per_device_train_batch_size=n, beta=0.1, logging_steps=1, max_steps=1, output_dir="/tmp/unused",
                         learning_rate=5e-5, warmup_steps=0, warmup_ratio=0.0, padding_free=pf)
        tr = SLAMDPOTrainer(model=pol, ref_model=ref, args=args, train_dataset=_pairs(n), processing_class=UnitTokeniser(None, load_fe=False))
        assert pol.padding_free is pf and ref.padding_free is pf
        mb = tr._collate_pairs(tr.train_dataset[:n])
        snap, tokens = {}, []
        update = tr._update
        tr._update = lambda lr, zero_grad: (snap.update(g={k: v.clone() for k, v in pol.named_grads()}), update(lr, zero_grad=zero_grad))
        fwd = pol.engine.forward_unpadded if pf else pol.engine.forward
        setattr(pol.engine, "forward_unpadded" if pf else "forward", lambda *a, **k: (fwd(*a, **k), tokens.append(pol.engine.last_forward_tokens())))
        pol.zero_grad()
        tr.optimizer_step([mb], 5e-5)
        sync()
        res[pf] = (float(tr._loss_acc), snap["g"], tokens, mb)
    B2, T = res[True][3]["input_ids"].shape
    packed = -(-int(res[True][3]["lengths"].sum()) // 64) * 64
    assert res[False][2] == [B2 * T] and res[True][2] == [packed] and packed < B2 * T
    print(f"DPO loss padded {res[False][0]:.6f} padding-free {res[True][0]:.6f}; tokens {B2 * T} -> {packed}")
    assert abs(res[False][0] - res[True][0]) <= 2e-2
    _grad_bars(res[True][1].items(), res[False][1])


# ------------------------------------------------------------------------------------------------------- recomputation
@pytest.mark.parametrize("body", ["qwen6_hd64", "opt5"])
def test_recompute_levels_are_bit_identical_padding_free(body):
    from tests.test_gpu_recompute import BODIES, _dense, _level, _step
    m = BODIES[body]()
    m.padding_free = True
    batch = _dense(502)  # 3 x 96, lengths 96 / 67 / 7
    outs = []
    for level in (0, 1, 2):
        _level(m, level)
        outs.append(_step(m, batch))
        assert m.engine.last_forward_tokens() == 192  # 170 real tokens, where the padded path runs 3 x 128
    for lv, o in zip((1, 2), outs[1:]):
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), f"level {lv} differs from level 0"
    assert float(outs[0][2].abs().max()) > 0 and bool(torch.isfinite(outs[0][2]).all())


# -------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_padding_free_vs_padded_and_resume(golden_data, tmp_path):
    """SLAMTrainer on the example tokens (chunked to 96 as the data pipeline chunks them: rows of 96 .. 2 tokens): every logged
    loss and the eval loss within 2e-2 of the padded run from the same seed; a save / resume in the middle repeats the
    uninterrupted padding-free run bit for bit."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.data.hf_dataset import split_into_chunks
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_gpu_train import _tiny_model
    rows = []
    for r in golden_data["G1_tokens"]:
        enc = O.unit_tokenise(r["audio_repr"])
        rows += [{"input_ids": c, "attention_mask": [1] * len(c)} for c in split_into_chunks(enc["input_ids"], 96)]
    lens = sorted(len(r["input_ids"]) for r in rows)
    assert len(rows) == 8 and lens[0] < 10 and lens[-1] == 96
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)
    sd = O.init_weights(O.TINY, seed=5, bias_std=0.02, norm_jitter=0.05)

    def run(pf, out, max_steps=6, resume=None, save_steps=0):
        m = _tiny_model(sd)
        a = SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=max_steps, num_train_epochs=4, warmup_steps=1,
                                  warmup_ratio=0.0, learning_rate=2e-3, logging_steps=1, save_steps=save_steps, seed=7,
                                  output_dir=str(out), padding_free=pf, per_device_eval_batch_size=4)
        tr = SLAMTrainer(model=m, args=a, data_collator=coll, train_dataset=ds, eval_dataset=ds)
        tokens = []
        name = "forward_unpadded" if pf else "forward"
        fwd = getattr(m.engine, name)
        setattr(m.engine, name, lambda *x, **k: (fwd(*x, **k), tokens.append(m.engine.last_forward_tokens())))
        st = tr.train(resume_from_checkpoint=resume)
        ev = tr.evaluate()["eval_loss"]
        return m, [r["loss"] for r in st.log_history if "loss" in r], ev, tokens

    m_pad, l_pad, e_pad, t_pad = run(False, tmp_path / "pad")
    m_pf, l_pf, e_pf, t_pf = run(True, tmp_path / "pf", save_steps=3)
    print("padded      ", [round(x, 4) for x in l_pad], round(e_pad, 4), t_pad)
    print("padding-free", [round(x, 4) for x in l_pf], round(e_pf, 4), t_pf)
    assert len(l_pad) == len(l_pf) == 6 and len(t_pad) == len(t_pf) == 8  # 6 steps + 2 evaluation batches
    # every batch of 4 holds a 96-token row: 384 padded positions; the evaluation batches are rows 0-3 (330 tokens) and 4-7 (290)
    assert all(a == 4 * 96 for a in t_pad) and all(b <= a and b % 64 == 0 for a, b in zip(t_pad, t_pf))
    assert t_pf[-2:] == [384, 320] and any(b < a for a, b in zip(t_pad[:6], t_pf[:6]))
    for a, b in zip(l_pad, l_pf):
        assert abs(a - b) <= 2e-2, (l_pad, l_pf)
    assert abs(e_pad - e_pf) <= 2e-2
    m_res, l_res, e_res, _ = run(True, tmp_path / "res", resume=str(tmp_path / "pf" / "checkpoint-3"))
    a, b = m_pf.state_dict(torch.float32), m_res.state_dict(torch.float32)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert e_res == e_pf and l_res[-3:] == l_pf[-3:]
