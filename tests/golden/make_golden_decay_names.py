"""Which parameters HF's Trainer decays. Run in the authoring container (transformers installed):
    python tests/golden/make_golden_decay_names.py
Writes tests/golden/decay_names.json (data only - lists of names): for a tiny tied Qwen2ForCausalLM, an untied one and an
OPTForCausalLM - built from the config.json of the hf_text_lm / hf_untied_text_lm / hf_opt_text_lm fixtures, random weights -
the full parameter-name list (`named_parameters`, which lists a tied lm_head.weight once, under the embedding's name) and the
subset `transformers.Trainer.get_decay_parameter_names(None, model)` returns: the names `Trainer.create_optimizer` gives
`weight_decay` to (the method uses no trainer state, so it is called unbound). It pins UnitLM.hf_decay_flags() without
transformers at test time.
"""
import json
import os

import transformers
from transformers import AutoConfig, AutoModelForCausalLM, Trainer

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = {"qwen2_tied": "hf_text_lm", "qwen2_untied": "hf_untied_text_lm", "opt": "hf_opt_text_lm"}


def decay_names(model):
    return Trainer.get_decay_parameter_names(None, model)


if __name__ == "__main__":
    out = {"transformers_version": transformers.__version__, "models": {}}
    for key, d in MODELS.items():
        cfg = AutoConfig.from_pretrained(os.path.join(HERE, d))
        model = AutoModelForCausalLM.from_config(cfg)
        names = [n for n, _ in model.named_parameters()]
        decay = decay_names(model)
        assert set(decay) - {"lm_head.weight"} <= set(names)
        out["models"][key] = {"config": d, "parameters": names, "decay": decay}
        print(key, len(names), "parameters,", len(decay), "decayed; not decayed:", sorted(set(names) - set(decay))[:6], "...")
    with open(os.path.join(HERE, "decay_names.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
