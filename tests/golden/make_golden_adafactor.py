"""HF's own Adafactor on the four decoder families. Run in the authoring container (transformers installed):
    python tests/golden/make_golden_adafactor.py
Writes tests/golden/adafactor_hf_<family>.npz (data only) for the families of tests/adafactor_ref.py FAMILIES - a tied Qwen2 with
the 502-row vocabulary, an untied Qwen2, an OPT and a Qwen3, one decoder layer of the narrowest body each (float64 results per HF
name: one file per family keeps every file below 1 MiB). Per family: transformers.optimization.Adafactor with the kwargs HF's
Trainer passes for optim = "adafactor" (scale_parameter = False, relative_step = False, lr from outside; everything else at its
default) over HF's decay / no-decay parameter groups (Trainer.get_decay_parameter_names) with weight_decay = HF_WD, run for
HF_STEPS steps in float64 and again in float32, from the initial parameters and the fresh gradients of adafactor_ref.hf_inputs
(reproducible from the name list: they are not stored) times the clip coefficient HF_CS < 1.

Stored: names (HF's named_parameters order, under the reference's `lm.` prefix), shapes, decay flags, and per name i
  p64_i / p32_i          the final parameters of the float64 / float32 run
  row64_i, col64_i       the final exp_avg_sq_row / exp_avg_sq_col of a matrix (float64; row32_i, col32_i: float32)
  v64_i                  the final exp_avg_sq of a vector (v32_i)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import transformers  # noqa: E402
from transformers import OPTConfig, OPTForCausalLM, Qwen2Config, Qwen2ForCausalLM, Qwen3Config, Qwen3ForCausalLM, Trainer  # noqa: E402
from transformers.optimization import Adafactor  # noqa: E402

from tests import adafactor_ref as A  # noqa: E402


def hf_model(base, vocab):
    kind = base.get("model_type", "qwen2")
    if kind == "opt":
        c = OPTConfig(vocab_size=vocab, hidden_size=base["hidden_size"], num_hidden_layers=base["num_hidden_layers"],
                      ffn_dim=base["ffn_dim"], num_attention_heads=base["num_attention_heads"],
                      max_position_embeddings=base["max_position_embeddings"], word_embed_proj_dim=base["hidden_size"],
                      tie_word_embeddings=True, pad_token_id=0, dropout=0.0)
        return OPTForCausalLM(c)
    cls, ccls = (Qwen3ForCausalLM, Qwen3Config) if kind == "qwen3" else (Qwen2ForCausalLM, Qwen2Config)
    c = ccls(vocab_size=vocab, hidden_size=base["hidden_size"], intermediate_size=base["intermediate_size"],
             num_hidden_layers=base["num_hidden_layers"], num_attention_heads=base["num_attention_heads"],
             num_key_value_heads=base["num_key_value_heads"], head_dim=base["head_dim"],
             tie_word_embeddings=base["tie_word_embeddings"], pad_token_id=0)
    return cls(c)


def run(model, dtype, inputs, decay):
    model = model.to(dtype)
    named = list(model.named_parameters())
    with torch.no_grad():
        for n, p in named:
            p.copy_(torch.from_numpy(inputs["lm." + n][0]).to(dtype))
    groups = [{"params": [p for n, p in named if n in decay], "weight_decay": A.HF_WD},
              {"params": [p for n, p in named if n not in decay], "weight_decay": 0.0}]
    opt = Adafactor(groups, lr=A.HF_LR, scale_parameter=False, relative_step=False)  # Trainer.get_optimizer_cls_and_kwargs
    for t in range(A.HF_STEPS):
        for n, p in named:
            p.grad = (torch.from_numpy(inputs["lm." + n][1][t]).to(torch.float64) * A.HF_CS).to(dtype)
        opt.step()
    return named, opt


if __name__ == "__main__":
    for fam, (base, vocab) in A.FAMILIES.items():
        torch.manual_seed(0)
        model = hf_model(base, vocab)
        decay = set(Trainer.get_decay_parameter_names(None, model))
        names = ["lm." + n for n, _ in model.named_parameters()]
        shapes = [tuple(p.shape) for _, p in model.named_parameters()]
        inputs = A.hf_inputs(list(zip(names, shapes)))
        out = {"names": np.array(names), "decay": np.array([n[3:] in decay for n in names]),
               "transformers_version": np.array(transformers.__version__)}
        for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
            named, opt = run(model, dtype, inputs, decay)
            for i, (n, p) in enumerate(named):
                st = opt.state[p]
                assert int(st["step"]) == A.HF_STEPS and "exp_avg" not in st
                out[f"p{tag}_{i}"] = p.detach().numpy().copy()
                if p.dim() >= 2:
                    out[f"row{tag}_{i}"], out[f"col{tag}_{i}"] = st["exp_avg_sq_row"].numpy().copy(), st["exp_avg_sq_col"].numpy().copy()
                else:
                    out[f"v{tag}_{i}"] = st["exp_avg_sq"].numpy().copy()
        path = os.path.join(HERE, f"adafactor_hf_{fam}.npz")
        np.savez_compressed(path, **out)
        print(fam, len(names), "parameters,", sum(int(np.prod(s)) for s in shapes), "elements,", os.path.getsize(path), "bytes")
