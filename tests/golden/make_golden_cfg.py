"""Golden data for classifier-free guidance (slam_cfg_scores, UnitLM.generate(guidance_scale=)), from transformers on the CPU:
    python tests/golden/make_golden_cfg.py
(a) Op level: transformers' own UnbatchedClassifierFreeGuidanceLogitsProcessor on random fp32 rows, with a stub model that
    returns fixed unconditional logits; V in {502, 2049}, g in {1.5, 3.0, 0.5, 0.0, -1.0}.
(b) End to end: HF greedy `generate` with guidance_scale on the tiny and the wide golden Qwen2 weights (the models of
    make_golden_generate.py, bf16-rounded weights, fp32 arithmetic), LEFT-padded prompts of lengths {1, 5, 37, 70}, no EOS:
      g15      g = 1.5, the default unconditional prompt (the last prompt token)
      g30neg   g = 3.0, unpadded 6-token negative prompts
      g05neg   g = 0.5, the same kind of negative prompts
      g05bans  g = 0.5, negative prompts, bad_words_ids (one- and two-token entries) and no_repeat_ngram_size = 2: pins the
               processor order. (Under g = 1.5 the banned repeats leave HF's own top two scores so close that no prompt
               seed below 200 reaches the share asked for below on the wide model; at g = 0.5 the tolerance is a third.)
    Per case: the sequences, the top-1 / top-2 margin of the processed scores of every step and the rms of the raw logits.
A step is a near-tie when its margin is below tol = (|g| + |1 - g|) * 2 * LOGITS_TOL * rms: test_gpu_generate.py's tolerance,
scaled by how g a - (g - 1) u amplifies an error of the logits. The test compares only the steps before a row's first near-tie,
so a case is usable only if most of its steps lie there: the prompt seed of a case walks up from 0 until, by HF's margins alone,
at least 60 % of all its steps lie before their row's first near-tie (asserted), and is recorded. The bans case also needs the
pad id 0 absent from the new tokens: HF's n-gram windows run over the left padding, UnitLM's over the real tokens.
Writes tests/golden/cfg_hf.npz.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor  # noqa: E402

from oracle import slam_oracle as O  # noqa: E402
from tests.conftest import load_wide_golden  # noqa: E402
from tests.golden.make_golden_generate import LENS, hf_model  # noqa: E402

GUIDANCE = (1.5, 3.0, 0.5, 0.0, -1.0)
OP_VOCABS = (502, 2049)
NEW = 24
NEG_LEN = 6
LOGITS_TOL = 2e-2  # tests/test_gpu_generate.py
MIN_TRUSTED = 0.6
BAD = [[5], [11], [17], [23, 31], [7, 2]]
CASES = {  # name: (g, negative prompts, bans)
    "g15": (1.5, False, False),
    "g30neg": (3.0, True, False),
    "g05neg": (0.5, True, False),
    "g05bans": (0.5, True, True),
}


class _Out(dict):
    @property
    def logits(self):
        return self["logits"]


def op_golden(res):
    for V in OP_VOCABS:
        g = torch.Generator().manual_seed(V)
        x = torch.randn(3, V, generator=g) * 3.0
        y = torch.randn(3, V, generator=g) * 3.0
        res[f"op_x_{V}"], res[f"op_y_{V}"] = x.numpy(), y.numpy()
        for gs in GUIDANCE:
            proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(gs, lambda *a, **k: _Out(logits=y[:, None, :]), use_cache=False)
            out = proc(torch.ones(3, 4, dtype=torch.long), x.clone())
            res[f"op_out_{V}_{gs}"] = out.numpy().astype(np.float32)


def prompts(vocab, seed):
    g = torch.Generator().manual_seed(seed)
    T = max(LENS)
    ids = torch.zeros(len(LENS), T, dtype=torch.long)
    am = torch.zeros(len(LENS), T, dtype=torch.long)
    for b, n in enumerate(LENS):
        ids[b, T - n:] = torch.tensor([1] + torch.randint(2, vocab, (n - 1,), generator=g).tolist())
        am[b, T - n:] = 1
    neg = torch.randint(2, vocab, (len(LENS), NEG_LEN), generator=g)
    return ids, am, neg


def run(m, ids, am, neg, gs, bans):
    kw = dict(input_ids=ids, attention_mask=am, do_sample=False, max_new_tokens=NEW, eos_token_id=None, pad_token_id=0,
              guidance_scale=gs, output_scores=True, output_logits=True, return_dict_in_generate=True)
    if neg is not None:
        kw.update(negative_prompt_ids=neg, negative_prompt_attention_mask=torch.ones_like(neg))
    if bans:
        kw.update(bad_words_ids=BAD, no_repeat_ngram_size=2)
    out = m.generate(**kw)
    sc = torch.stack([s.float() for s in out.scores], 1)  # [B, steps, V] processed scores
    top = sc.topk(2, -1).values
    raw = torch.stack([s.float() for s in out.logits], 1)
    return out.sequences, top[..., 0] - top[..., 1], float(raw.pow(2).mean().sqrt())


def trusted_share(margin, tol):
    steps = margin.shape[1]
    n = 0
    for b in range(margin.shape[0]):
        low = (margin[b] < tol).nonzero()
        n += int(low[0]) if len(low) else steps
    return n / float(margin.numel())


def make(tag, cfg, seed, bias_std, jit, res):
    m = hf_model(cfg, O.init_weights(cfg, seed=seed, bias_std=bias_std, norm_jitter=jit))
    m.generation_config.eos_token_id = None
    for case, (gs, use_neg, bans) in CASES.items():
        for pseed in range(200):
            ids, am, neg = prompts(cfg.vocab, pseed)
            with torch.no_grad():
                seq, margin, rms = run(m, ids, am, neg if use_neg else None, gs, bans)
            tol = (abs(gs) + abs(1 - gs)) * 2 * LOGITS_TOL * rms
            share = trusted_share(margin, tol)
            if share >= MIN_TRUSTED and not (bans and bool((seq[:, ids.shape[1]:] == 0).any())):
                break
            print(tag, case, "prompt seed", pseed, "share", round(share, 3), "- next")
        assert share >= MIN_TRUSTED, (tag, case, share)
        k = f"{tag}_{case}"
        res[f"{k}_ids"], res[f"{k}_mask"] = ids.numpy(), am.numpy()
        if use_neg:
            res[f"{k}_neg"] = neg.numpy()
        res[f"{k}_seq"], res[f"{k}_margin"] = seq.numpy(), margin.numpy().astype(np.float32)
        res[f"{k}_rms"], res[f"{k}_seed"], res[f"{k}_g"] = np.float32(rms), np.int64(pseed), np.float32(gs)
        print(tag, case, "prompt seed", pseed, "logits rms", rms, "tol", tol, "trusted share", share)


def main():
    res = {"bad_words": np.array(json.dumps(BAD)), "max_new_tokens": np.int64(NEW), "no_repeat_ngram_size": np.int64(2)}
    op_golden(res)
    meta = json.load(open(os.path.join(HERE, "data.json")))["meta"]
    make("tiny", O.OracleConfig(**meta["config"]), meta["seed"], meta["bias_std"], meta["norm_jitter"], res)
    _, wcfg, wseed, wbias, wjit = load_wide_golden()
    make("wide", O.OracleConfig(**wcfg), wseed, wbias, wjit, res)
    np.savez_compressed(os.path.join(HERE, "cfg_hf.npz"), **res)


if __name__ == "__main__":
    main()
