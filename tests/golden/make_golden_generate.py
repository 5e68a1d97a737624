"""Golden greedy generations from HuggingFace's own `generate` (transformers Qwen2ForCausalLM, fp32, CPU) for the KV-cached
path of UnitLM.generate (tests/test_gpu_generate.py):
    python tests/golden/make_golden_generate.py
Weights: oracle.init_weights of the tiny config (tests/golden/data.json meta) and of the head_dim-128 "wide" config
(wide_model.npz meta), rounded to bf16 like the engine's parameters. Prompts of lengths {1, 5, 37, 70}, LEFT-padded with an
attention_mask, bad_words_ids and an eos_token_id that one row emits mid-way. Stores the sequences and the top-1 / top-2 margin
of the processed scores of every step, so the test can tell which steps a bf16 engine must reproduce exactly.
Writes tests/golden/generate.npz.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from transformers import Qwen2Config, Qwen2ForCausalLM  # noqa: E402

from oracle import slam_oracle as O  # noqa: E402
from tests.conftest import load_wide_golden  # noqa: E402

LENS = [1, 5, 37, 70]
NEW = 40
BAD = [[5], [11], [17]]


def hf_model(cfg, sd):
    c = Qwen2Config(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                    num_hidden_layers=cfg.n_layers, num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads,
                    head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, tie_word_embeddings=True,
                    max_position_embeddings=4096, pad_token_id=0, bos_token_id=1, eos_token_id=1, attention_dropout=0.0)
    m = Qwen2ForCausalLM(c).float().eval()
    hf = {k[len("lm."):]: v.to(torch.bfloat16).float() for k, v in sd.items()}
    missing, unexpected = m.load_state_dict(hf, strict=False)
    assert not unexpected and all("lm_head" in k for k in missing), (missing, unexpected)
    m.tie_weights()
    return m


def prompts(vocab, seed):
    g = torch.Generator().manual_seed(seed)
    T = max(LENS)
    ids = torch.zeros(len(LENS), T, dtype=torch.long)
    am = torch.zeros(len(LENS), T, dtype=torch.long)
    for b, n in enumerate(LENS):
        row = [1] + torch.randint(2, vocab, (n - 1,), generator=g).tolist()
        ids[b, T - n:] = torch.tensor(row)
        am[b, T - n:] = 1
    return ids, am


def run(m, ids, am, eos):
    out = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=BAD, do_sample=False, max_new_tokens=NEW,
                     eos_token_id=eos, pad_token_id=0, output_scores=True, return_dict_in_generate=True)
    sc = torch.stack([s.float() for s in out.scores], 1)  # [B, steps, V] processed scores
    top = sc.topk(2, -1).values
    fin = sc[torch.isfinite(sc)]
    return out.sequences, (top[..., 0] - top[..., 1]), float(fin.pow(2).mean().sqrt())


def make(tag, cfg, seed, bias_std, jit, res):
    sd = O.init_weights(cfg, seed=seed, bias_std=bias_std, norm_jitter=jit)
    m = hf_model(cfg, sd)
    ids, am = prompts(cfg.vocab, 100 + seed)
    with torch.no_grad():
        seq0, _, _ = run(m, ids, am, None)
        # EOS = a token row 2 emits at step 8 and no row emits earlier: that row stops early, the others run on
        new0 = seq0[:, ids.shape[1]:]
        eos = int(new0[2, 8])
        seq, margin, rms = run(m, ids, am, eos)
    res[f"{tag}_ids"], res[f"{tag}_mask"] = ids.numpy(), am.numpy()
    res[f"{tag}_seq"], res[f"{tag}_margin"] = seq.numpy(), margin.numpy().astype(np.float32)
    res[f"{tag}_eos"], res[f"{tag}_score_rms"] = np.int64(eos), np.float32(rms)
    res[f"{tag}_meta"] = np.array([cfg.n_layers, cfg.hidden, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.intermediate,
                                   cfg.vocab, seed], dtype=np.int64)
    res[f"{tag}_meta_f"] = np.array([cfg.rms_eps, cfg.rope_theta, bias_std, jit], dtype=np.float64)
    print(tag, "eos", eos, "shape", tuple(seq.shape), "score rms", rms)
    print(seq[:, ids.shape[1]:])
    print(margin)


def main():
    res = {"bad_words": np.array(BAD, dtype=np.int64), "max_new_tokens": np.int64(NEW)}
    meta = json.load(open(os.path.join(HERE, "data.json")))["meta"]
    make("tiny", O.OracleConfig(**meta["config"]), meta["seed"], meta["bias_std"], meta["norm_jitter"], res)
    _, wcfg, wseed, wbias, wjit = load_wide_golden()
    make("wide", O.OracleConfig(**wcfg), wseed, wbias, wjit, res)
    np.savez_compressed(os.path.join(HERE, "generate.npz"), **res)


if __name__ == "__main__":
    main()
