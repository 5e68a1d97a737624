"""Reference-WRITTEN OPT fixtures (the reference's default body is OPT). Run in the authoring container:
    HF_HUB_OFFLINE=1 python tests/golden/make_golden_opt.py
Writes (data only - safetensors weights, json configs, npz inputs/outputs):
  tests/golden/hf_opt_text_lm/   <- `transformers.OPTForCausalLM.save_pretrained` of a tiny 1-layer OPT text LM with a 640-row
                                    vocabulary (bf16 weights): the TWIST source and the base-config anchor of the checkpoint
  tests/golden/ref_opt_ckpt/     <- reference `UnitLM.save_pretrained` of a tiny 1-layer OPT UnitLM (bf16 weights;
                                    config.json holds the serialised OPTConfig under base_config, keys lm.model.decoder.*)
  tests/golden/opt_model.npz     <- a right-padded token batch and, from the reference model reloaded with
                                    `UnitLM.from_pretrained` and run in fp32: logits, mean loss and loss with num_items_in_batch,
                                    per-tensor gradient norms of the mean loss, log_likelihood with and without ignore_tokens;
                                    the same loss of the reference `UnitLM(twist_init=True, base_model_name=hf_opt_text_lm)`
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

from transformers import OPTConfig, OPTForCausalLM  # noqa: E402
from slamkit.model.unit_lm import UnitLM, UnitLMConfig  # noqa: E402

UnitLMConfig.has_no_defaults_at_init = True  # see make_golden_ckpt.py

DIMS = dict(hidden_size=128, ffn_dim=256, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=128,
            word_embed_proj_dim=128, do_layer_norm_before=True, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
            layerdrop=0.0, init_std=0.02, tie_word_embeddings=True)
V = 502


def randomise(m, seed):
    """HF init leaves biases at 0 and LayerNorms at 1: perturb them so the fixture exercises every tensor; round to bf16."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif "layer_norm.weight" in k:
                p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.1)
            p.copy_(p.bfloat16().float())
    return m


out = {}
g = torch.Generator().manual_seed(7)
B, T = 3, 64
ids = torch.randint(2, V, (B, T), generator=g)
lens = [64, 41, 17]
mask = torch.zeros(B, T, dtype=torch.int64)
for b, n in enumerate(lens):
    mask[b, :n] = 1
ids = ids.masked_fill(mask == 0, 0)
labels = ids.masked_fill(mask == 0, -100)
out["ids"], out["mask"], out["labels"] = ids.numpy(), mask.numpy(), labels.numpy()

os.chdir(ROOT)  # base_model_name below is the repository-relative path of the text LM
REL_TEXT = os.path.join("tests", "golden", "hf_opt_text_lm")
torch.manual_seed(1)
text = randomise(OPTForCausalLM(OPTConfig(vocab_size=640, pad_token_id=0, bos_token_id=1, eos_token_id=1, **DIMS)).float(), 12)
t = os.path.join(ROOT, REL_TEXT)
shutil.rmtree(t, ignore_errors=True)
text.to(torch.bfloat16).save_pretrained(t, safe_serialization=True)
text.float()

torch.manual_seed(2)
m = randomise(UnitLM(UnitLMConfig(base_model_name=REL_TEXT, vocab_size=V, twist_init=False, torch_dtype=torch.float32)).float(), 11)
d = os.path.join(HERE, "ref_opt_ckpt")
shutil.rmtree(d, ignore_errors=True)
m.to(torch.bfloat16).save_pretrained(d, safe_serialization=True)
cj = os.path.join(d, "config.json")  # the text LM's path as the repository names it, not as the authoring machine does
with open(cj) as f:
    txt = f.read().replace(t, REL_TEXT)
with open(cj, "w") as f:
    f.write(txt)
m2 = UnitLM.from_pretrained(d).float().eval()
o = m2(input_ids=ids, attention_mask=mask, labels=labels)
out["logits"], out["loss"] = o.logits.detach().float().numpy(), np.float32(o.loss.detach())
o.loss.backward()
names = sorted(k for k, _ in m2.named_parameters())
out["grad_names"] = np.array(names)
out["grad_norms"] = np.array([float(dict(m2.named_parameters())[k].grad.norm()) for k in names], dtype=np.float64)
with torch.no_grad():
    out["loss_num_items"] = np.float32(m2(input_ids=ids, attention_mask=mask, labels=labels, num_items_in_batch=100).loss)
    out["ll"] = m2.log_likelihood(ids.clone(), mean_nll=False).float().numpy()  # the reference rewrites its input in place
    out["ll_ignore"] = m2.log_likelihood(ids.clone(), mean_nll=False, ignore_tokens=[3, 4, 5, 200]).float().numpy()

torch.manual_seed(5)
tw = UnitLM(UnitLMConfig(base_model_name=REL_TEXT, vocab_size=V, twist_init=True, torch_dtype=torch.float32)).float().eval()
with torch.no_grad():
    out["twist_loss"] = np.float32(tw(input_ids=ids, attention_mask=mask, labels=labels).loss)
np.savez_compressed(os.path.join(HERE, "opt_model.npz"), **out)
for p in (d, t):
    for fn in sorted(os.listdir(p)):
        print(p, fn, os.path.getsize(os.path.join(p, fn)))
print({k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()})
