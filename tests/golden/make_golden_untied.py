"""Reference-WRITTEN fixtures of an UNTIED Qwen2 body (Qwen2.5-7B unties its lm_head). Run in the authoring container:
    HF_HUB_OFFLINE=1 python tests/golden/make_golden_untied.py
Writes (data only - safetensors weights, json configs, npz inputs/outputs):
  tests/golden/hf_untied_text_lm/  <- `transformers.Qwen2ForCausalLM.save_pretrained` of a tiny untied text LM with a 640-row
                                      vocabulary (bf16 weights): ONLY what the reference's config points at as
                                      base_model_name while this script runs and in the checkpoint's config.json; no test
                                      opens it (the engine takes the dims from base_config; the TWIST test builds its own
                                      untied text LM)
  tests/golden/ref_untied_ckpt/    <- reference `UnitLM.save_pretrained` of a tiny untied Qwen2 UnitLM (hidden 128, 2 layers,
                                      bf16 weights; keys lm.model.* and lm.lm_head.weight)
  tests/golden/untied_model.npz    <- a right-padded token batch and, from the reference model reloaded with
                                      `UnitLM.from_pretrained` and run in fp32: logits, mean loss and loss with
                                      num_items_in_batch, per-tensor gradient norms of the mean loss, log_likelihood with and
                                      without ignore_tokens; and HF greedy generations of the same model (left-padded prompts,
                                      bad_words_ids, an EOS that one row emits mid-way) with the FULL processed scores of
                                      every step, so that a test can compare every decode step teacher-forced.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

stub = tempfile.mkdtemp()
os.makedirs(os.path.join(stub, "omegaconf"))
with open(os.path.join(stub, "omegaconf", "__init__.py"), "w") as f:
    f.write("class DictConfig(dict): pass\nclass ListConfig(list): pass\nclass OmegaConf: pass\n")
sys.path[:0] = [stub, REF, ROOT]

from transformers import Qwen2Config, Qwen2ForCausalLM  # noqa: E402
from slamkit.model.unit_lm import UnitLM, UnitLMConfig  # noqa: E402

UnitLMConfig.has_no_defaults_at_init = True  # see make_golden_ckpt.py

DIMS = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
            rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=False, max_position_embeddings=4096,
            attention_dropout=0.0)
V = 502
LENS = [1, 5, 37, 70]
NEW = 40
BAD = [[5], [11], [17]]


def randomise(m, seed):
    """HF init leaves biases at 0 and norms at 1: perturb them so the fixture exercises every tensor; round to bf16."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif k.endswith("norm.weight"):
                p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.1)
            p.copy_(p.bfloat16().float())
    return m


out = {}
g = torch.Generator().manual_seed(7)
B, T = 3, 64
ids = torch.randint(2, V, (B, T), generator=g)
ids[:, 0] = 1
lens = [64, 41, 17]
mask = torch.zeros(B, T, dtype=torch.int64)
for b, n in enumerate(lens):
    mask[b, :n] = 1
ids = ids.masked_fill(mask == 0, 0)
labels = ids.masked_fill(mask == 0, -100)
out["ids"], out["mask"], out["labels"] = ids.numpy(), mask.numpy(), labels.numpy()

os.chdir(ROOT)  # base_model_name below is the repository-relative path of the text LM
REL_TEXT = os.path.join("tests", "golden", "hf_untied_text_lm")
torch.manual_seed(1)
text = randomise(Qwen2ForCausalLM(Qwen2Config(vocab_size=640, pad_token_id=0, bos_token_id=1, eos_token_id=1, **DIMS)).float(), 12)
t = os.path.join(ROOT, REL_TEXT)
shutil.rmtree(t, ignore_errors=True)
text.to(torch.bfloat16).save_pretrained(t, safe_serialization=True)
text.float()

torch.manual_seed(2)
m = randomise(UnitLM(UnitLMConfig(base_model_name=REL_TEXT, vocab_size=V, twist_init=False, torch_dtype=torch.float32)).float(), 11)
assert m.config.tie_word_embeddings is False
assert m.lm.lm_head.weight.data_ptr() != m.lm.model.embed_tokens.weight.data_ptr()
d = os.path.join(HERE, "ref_untied_ckpt")
shutil.rmtree(d, ignore_errors=True)
m.to(torch.bfloat16).save_pretrained(d, safe_serialization=True)
cj = os.path.join(d, "config.json")  # the text LM's path as the repository names it, not as the authoring machine does
with open(cj) as f:
    txt = f.read().replace(t, REL_TEXT)
with open(cj, "w") as f:
    f.write(txt)
m2 = UnitLM.from_pretrained(d).float().eval()
assert not torch.equal(m2.lm.lm_head.weight, m2.lm.model.embed_tokens.weight)
o = m2(input_ids=ids, attention_mask=mask, labels=labels)
out["logits"], out["loss"] = o.logits.detach().float().numpy(), np.float32(o.loss.detach())
o.loss.backward()
names = sorted(k for k, _ in m2.named_parameters())
assert "lm.lm_head.weight" in names
out["grad_names"] = np.array(names)
out["grad_norms"] = np.array([float(dict(m2.named_parameters())[k].grad.norm()) for k in names], dtype=np.float64)
with torch.no_grad():
    out["loss_num_items"] = np.float32(m2(input_ids=ids, attention_mask=mask, labels=labels, num_items_in_batch=100).loss)
    out["ll"] = m2.log_likelihood(ids.clone(), mean_nll=False).float().numpy()  # the reference rewrites its input in place
    out["ll_ignore"] = m2.log_likelihood(ids.clone(), mean_nll=False, ignore_tokens=[3, 4, 5, 200]).float().numpy()

# ---- greedy generation of the same model through HF's generate, full processed scores kept ------------------------------
gg = torch.Generator().manual_seed(107)
Tp = max(LENS)
pids = torch.zeros(len(LENS), Tp, dtype=torch.long)
pam = torch.zeros(len(LENS), Tp, dtype=torch.long)
for b, n in enumerate(LENS):
    row = [1] + torch.randint(2, V, (n - 1,), generator=gg).tolist()
    pids[b, Tp - n:] = torch.tensor(row)
    pam[b, Tp - n:] = 1


def run(eos):
    r = m2.generate(input_ids=pids, attention_mask=pam, bad_words_ids=BAD, do_sample=False, max_new_tokens=NEW,
                    eos_token_id=eos, pad_token_id=0, output_scores=True, return_dict_in_generate=True, use_cache=True)
    return r.sequences, torch.stack([s.float() for s in r.scores], 1)  # [B, steps, V] processed scores


with torch.no_grad():
    seq0, _ = run(None)
    eos = int(seq0[2, Tp + 8])  # a token row 2 emits at step 8: that row stops early, the others run on
    assert not (seq0[:, Tp:Tp + 8] == eos).any()
    seq, sc = run(eos)
assert sc.shape == (len(LENS), NEW, V), sc.shape
top = sc.topk(2, -1).values
fin = sc[torch.isfinite(sc)]
out["gen_ids"], out["gen_mask"], out["gen_seq"] = pids.numpy(), pam.numpy(), seq.numpy()
out["gen_scores"] = sc.numpy().astype(np.float32)
out["gen_margin"] = (top[..., 0] - top[..., 1]).numpy().astype(np.float32)
out["gen_eos"], out["gen_score_rms"] = np.int64(eos), np.float32(fin.pow(2).mean().sqrt())
out["bad_words"], out["max_new_tokens"] = np.array(BAD, dtype=np.int64), np.int64(NEW)

np.savez_compressed(os.path.join(HERE, "untied_model.npz"), **out)
for p in (d, t):
    for fn in sorted(os.listdir(p)):
        print(p, fn, os.path.getsize(os.path.join(p, fn)))
print(os.path.getsize(os.path.join(HERE, "untied_model.npz")), "bytes untied_model.npz")
print({k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()})
print("eos", eos, "new tokens\n", seq[:, Tp:])
