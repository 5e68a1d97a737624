"""Golden outputs of HuggingFace Qwen3ForCausalLM (fp32, CPU) for the Qwen3 family (tests/test_qwen3_host.py,
tests/test_gpu_qwen3.py):
    python tests/golden/make_golden_qwen3.py
Weights: tests/qwen3_ref.py `weights` of the two tiny configs A (head_dim 128, n_heads * head_dim != hidden) and B (head_dim
64, the fused-RoPE shape of the Qwen2 family), bf16-representable. Per config it stores
  * the logits of the real tokens of qwen3_ref.batch() (3 x 100, lengths 100 / 61 / 17), rows concatenated, fp32 with the
    low 8 mantissa bits rounded away (2^-16 relative: the file stays small), and the mean loss;
  * the gradient norm of every parameter and the gradients of layer 0's four norm-type vectors;
  * a greedy `generate` of 40 tokens from left-padded prompts of lengths {1, 5, 37, 70} with bad words and an EOS one row
    emits mid-way, and the top-1 / top-2 margin of every step, in the layout of make_golden_generate.py.
It refuses to write a generation whose rows have fewer than 10 steps before the first near-tie (margin below
2 x 2e-2 x score rms, the rule of test_generate_matches_hf_golden): choose another seed then.
Writes tests/golden/qwen3.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from transformers import Qwen3Config, Qwen3ForCausalLM  # noqa: E402

from tests import qwen3_ref as R  # noqa: E402
from tests.golden.make_golden_generate import BAD, NEW, prompts, run  # noqa: E402

LOGITS_TOL = 2e-2
EOS_STEP = 9  # the earliest step at which a row may stop: at least 10 new tokens on every row


def hf_model(cfg, sd):
    c = Qwen3Config(vocab_size=R.VOCAB, hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                    num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                    num_key_value_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], rms_norm_eps=cfg["rms_norm_eps"],
                    rope_theta=cfg["rope_theta"], tie_word_embeddings=True, max_position_embeddings=4096, pad_token_id=0,
                    bos_token_id=1, eos_token_id=1, attention_dropout=0.0, attention_bias=False, use_sliding_window=False)
    rp = getattr(c, "rope_parameters", None)
    theta = rp["rope_theta"] if isinstance(rp, dict) and "rope_theta" in rp else c.rope_theta
    assert float(theta) == float(cfg["rope_theta"]), theta
    m = Qwen3ForCausalLM(c).float().eval()
    missing, unexpected = m.load_state_dict({k[len("lm."):]: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("lm_head" in k for k in missing), (missing, unexpected)
    m.tie_weights()
    return m


def trim(x: torch.Tensor) -> np.ndarray:
    """fp32 with the low 8 mantissa bits rounded to nearest: 2^-17 relative error at most."""
    i = x.detach().float().contiguous().numpy().view(np.int32).astype(np.int64)
    return (((i + 0x80) >> 8) << 8).astype(np.int32).view(np.float32)


def make(tag, res):
    cfg, seed = R.CFGS[tag], R.SEED[tag]
    sd = R.weights(cfg, seed)
    m = hf_model(cfg, sd)
    ids, mask, labels, lens = R.batch()
    out = m(input_ids=ids, attention_mask=mask)
    loss = R.loss_of(out.logits, labels)
    loss.backward()
    res[f"{tag}_logits"] = trim(torch.cat([out.logits[b, :n] for b, n in enumerate(lens)]))
    res[f"{tag}_loss"] = np.float64(float(loss.detach()))
    names = [k for k, _ in R.hf_keys(cfg)]
    hp = dict(m.named_parameters())
    res[f"{tag}_grad_norms"] = np.array([float(hp[k[len("lm."):]].grad.double().norm()) for k in names], dtype=np.float64)
    for short in ("input_layernorm", "post_attention_layernorm", "self_attn.q_norm", "self_attn.k_norm"):
        res[f"{tag}_grad_{short.split('.')[-1]}"] = hp[f"model.layers.0.{short}.weight"].grad.float().numpy()
    # the restatement agrees with HF (the host test asserts the same from the file)
    ref = R.forward(cfg, sd, ids, attention_mask=mask).detach()
    for b, n in enumerate(lens):
        e = float((ref[b, :n] - out.logits[b, :n]).norm() / out.logits[b, :n].norm())
        assert e < 1e-4, (tag, b, e)
    # generation
    pids, am = prompts(R.VOCAB, 100 + seed)
    with torch.no_grad():
        seq0, _, _ = run(m, pids, am, None)
        new0 = seq0[:, pids.shape[1]:]
        eos = None
        for row in (2, 1, 3, 0):  # a token one row emits at step s >= 9 and no row emits earlier: that row stops mid-way
            for s in range(EOS_STEP, NEW):
                t = int(new0[row, s])
                if eos is None and not bool((new0[:, :s] == t).any()) and [t] not in BAD:
                    eos = t
        assert eos is not None, "no usable EOS: choose another seed"
        seq, margin, rms = run(m, pids, am, eos)
    tol = 2 * LOGITS_TOL * rms
    new = seq[:, pids.shape[1]:]
    for b in range(seq.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else margin.shape[1]
        hit = (new[b] == eos).nonzero()
        length = int(hit[0]) + 1 if len(hit) else new.shape[1]
        print(tag, "row", b, "trusted steps", trust, "length", length)
        assert min(trust, length) >= 10, (tag, b, trust, length, "choose another seed")
    res[f"{tag}_ids"], res[f"{tag}_mask"] = pids.numpy(), am.numpy()
    res[f"{tag}_seq"], res[f"{tag}_margin"] = seq.numpy(), margin.numpy().astype(np.float32)
    res[f"{tag}_eos"], res[f"{tag}_score_rms"] = np.int64(eos), np.float32(rms)
    res[f"{tag}_seed"] = np.int64(seed)
    print(tag, "loss", float(loss.detach()), "eos", eos, "score rms", rms)


def main():
    res = {"bad_words": np.array(BAD, dtype=np.int64), "max_new_tokens": np.int64(NEW)}
    for tag in ("A", "B"):
        make(tag, res)
    path = os.path.join(HERE, "qwen3.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
