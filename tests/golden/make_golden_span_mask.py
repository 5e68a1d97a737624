"""Span-mask fixtures: what the reference computes for left- and both-side-padded rows. Run in the authoring container, on the
CPU, with the reference checkout's path in SLAMKIT_REFERENCE:
    HF_HUB_OFFLINE=1 SLAMKIT_REFERENCE=<reference checkout> python tests/golden/make_golden_span_mask.py
Writes tests/golden/span_mask.npz (data only). The batch is 3 x 40 with spans (start, length) = (0, 40), (23, 17), (9, 12):
a full row, a left-padded row and a row padded on both sides; labels are the ids with -100 outside the spans and at each
row's first real token (HF predicts that one from a pad query). Two models, both run through the imported reference UnitLM
in fp32: "qwen2" - the tiny Qwen2 of data.json (weights from oracle.init_weights); "opt" - the reference-written OPT
checkpoint tests/golden/ref_opt_ckpt. Stored per model <m>:
  <m>_logits_real  fp32 [69][502]: the logits at the real positions, rows in batch order
  <m>_loss, <m>_loss_num_items (num_items_in_batch = 100), <m>_grad_names / <m>_grad_norms (of the mean loss)
  <m>_row_alone_maxdiff [3]: each row's largest logit difference to the same row's real tokens run alone, unpadded
and ids, mask, labels, starts, lens. Asserted here: everything finite, row-alone differences <= 1e-5."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["SLAMKIT_REFERENCE"]

stub = tempfile.mkdtemp()
os.makedirs(os.path.join(stub, "omegaconf"))
with open(os.path.join(stub, "omegaconf", "__init__.py"), "w") as f:
    f.write("class DictConfig(dict): pass\nclass ListConfig(list): pass\nclass OmegaConf: pass\n")
sys.path[:0] = [stub, REF, ROOT]

from transformers import Qwen2Config  # noqa: E402
from slamkit.model.unit_lm import UnitLM, UnitLMConfig  # noqa: E402
from oracle import slam_oracle as O  # noqa: E402

UnitLMConfig.has_no_defaults_at_init = True  # see make_golden_ckpt.py

B, T, V = 3, 40, 502
SPANS = [(0, 40), (23, 17), (9, 12)]


def qwen2():
    meta = json.load(open(os.path.join(HERE, "data.json")))["meta"]
    cfg = O.OracleConfig(**meta["config"])
    base = Qwen2Config(vocab_size=151936, hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                       num_hidden_layers=cfg.n_layers, num_attention_heads=cfg.n_heads,
                       num_key_value_heads=cfg.n_kv_heads, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
                       tie_word_embeddings=True, max_position_embeddings=32768, pad_token_id=0, bos_token_id=1,
                       eos_token_id=1, attention_dropout=0.0)
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, twist_init=False))
    sd = O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("lm_head" in k for k in missing), (missing, unexpected)
    m.lm.tie_weights()
    return m.float().eval()


def opt():
    os.chdir(ROOT)  # the checkpoint names its text LM by a repository-relative path
    return UnitLM.from_pretrained(os.path.join(HERE, "ref_opt_ckpt")).float().eval()


g = torch.Generator().manual_seed(29)
ids = torch.randint(2, V, (B, T), generator=g)
mask = torch.zeros(B, T, dtype=torch.int64)
for b, (s, n) in enumerate(SPANS):
    mask[b, s:s + n] = 1
ids = ids.masked_fill(mask == 0, 0)
labels = ids.masked_fill(mask == 0, -100)
for b, (s, n) in enumerate(SPANS):
    labels[b, s] = -100
out = dict(ids=ids.numpy(), mask=mask.numpy(), labels=labels.numpy(), starts=np.array([s for s, _ in SPANS], np.int32),
           lens=np.array([n for _, n in SPANS], np.int32))

for name, make in (("qwen2", qwen2), ("opt", opt)):
    m = make()
    o = m(input_ids=ids, attention_mask=mask, labels=labels)
    if not bool(torch.isfinite(o.logits).all() and torch.isfinite(o.loss)):  # fully masked pad queries under the default kernel
        m.lm.set_attn_implementation("eager")
        o = m(input_ids=ids, attention_mask=mask, labels=labels)
        print(name, "eager attention")
    logits = o.logits.detach().float()
    real = mask.bool()
    assert bool(torch.isfinite(logits[real]).all()) and bool(torch.isfinite(o.loss))
    out[name + "_logits_real"] = logits[real].numpy()
    out[name + "_loss"] = np.float32(o.loss.detach())
    m.zero_grad()
    o.loss.backward()
    params = dict(m.named_parameters())
    names = sorted(k for k, p in params.items() if p.grad is not None)
    norms = np.array([float(params[k].grad.norm()) for k in names], dtype=np.float64)
    assert np.isfinite(norms).all()
    out[name + "_grad_names"], out[name + "_grad_norms"] = np.array(names), norms
    with torch.no_grad():
        out[name + "_loss_num_items"] = np.float32(m(input_ids=ids, attention_mask=mask, labels=labels, num_items_in_batch=100).loss)
        alone = [float((m(input_ids=ids[b:b + 1, s:s + n]).logits[0].float() - logits[b, s:s + n]).abs().max())
                 for b, (s, n) in enumerate(SPANS)]
    assert np.isfinite(out[name + "_loss_num_items"])
    out[name + "_row_alone_maxdiff"] = np.array(alone, np.float64)
    print(name, "loss", out[name + "_loss"], "num_items", out[name + "_loss_num_items"], "row alone", alone)
    assert max(alone) <= 1e-5, alone

out["transformers"] = np.array(__import__("transformers").__version__)
np.savez_compressed(os.path.join(HERE, "span_mask.npz"), **out)
print({k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "span_mask.npz")))
