"""SHA-256 digests of what a training step and the cached-generation calls compute, one line per configuration: the check
that two builds of the engine are bit-identical (a refactor of the step's host code against its parent).

Usage: [SLAM_ENGINE_LIB=/path/to/libslam_engine.so] python tools/step_digest.py [--list] [--only TAG]
Run it once per library and diff the outputs. A training line carries the loss, the logits, flat_grads, the bf16 gradient image
where one is bound, both outputs of grad_norm and the bucket callback's (offset, count, stream is None) calls; an inference line
the fp32 logits (and slam_extend_score's log-probs and argmax). --only runs one configuration (the process to put under a
tracer). The bodies are the small shapes tests/test_gpu_recompute.py justifies (the three shared slots wrap, both bucket rules
fire), hidden 256, a few hundred tokens, biases and norm weights perturbed away from their initial values.

The configurations of a body run one after the other on ONE model and engine, so what a run leaves behind (the dropout call
counter, which buffer holds the last gradients, the validity of the norm partials, the bound workspace) carries into the next
line: a full run is deterministic and two full runs compare line by line, but a --only run starts from a fresh engine and its
digests need not equal that tag's line of a full run. Compare --only runs with --only runs."""
import argparse
import hashlib
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slamkit_amd.model import UnitLM, UnitLMConfig  # noqa: E402


def _qwen(L, heads, kv, hd, vocab=502, theta=10000.0, untied=False, qwen3=False):
    base = dict(num_hidden_layers=L, hidden_size=256, num_attention_heads=heads, num_key_value_heads=kv, head_dim=hd,
                intermediate_size=512, rms_norm_eps=1e-6, rope_theta=theta, tie_word_embeddings=not untied)
    if qwen3:
        base["model_type"] = "qwen3"
    return UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=vocab, max_tokens=1024), seed=3)


def _opt(dropout=0.0):
    base = dict(model_type="opt", num_hidden_layers=5, hidden_size=256, num_attention_heads=4, ffn_dim=512,
                max_position_embeddings=256, init_std=0.02)
    kw = dict(dropout=dropout) if dropout else {}
    return UnitLM(UnitLMConfig(base_model_name="local-opt", base_config=base, vocab_size=502, max_tokens=1024, **kw), seed=7)


BODIES = {
    "q6": lambda: _qwen(6, 4, 2, 64),
    "w4": lambda: _qwen(4, 2, 1, 128, vocab=700, theta=1e6),
    "untied": lambda: _qwen(2, 4, 2, 64, untied=True),
    "opt5": _opt,
    "opt5drop": lambda: _opt(0.1),
    "q3": lambda: _qwen(5, 4, 2, 64, qwen3=True),
}
CACHED = ("q6", "w4", "q3")  # KV-cached generation exists for the Qwen families


def build(body):
    m = BODIES[body]()
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "norm" in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


def batch(kind, vocab, seed):
    """dense: 3 right-padded rows of 96; pf: the same rows run padding-free; packed: 5 segments in one row with position_ids"""
    g = torch.Generator().manual_seed(seed)
    if kind == "packed":
        ids, pos = [], []
        for n in (100, 37, 130, 5, 64):
            t = torch.randint(2, vocab, (n,), generator=g)
            t[0] = 1
            ids.append(t), pos.append(torch.arange(n))
        ids, pos = torch.cat(ids)[None], torch.cat(pos)[None]
        return dict(input_ids=ids, position_ids=pos, labels=torch.where(pos == 0, -100, ids))
    ids = torch.randint(2, vocab, (3, 96), generator=g)
    ids[:, 0] = 1
    am = torch.ones(3, 96, dtype=torch.long)
    am[1, 67:] = 0
    am[2, 7:] = 0
    ids = ids * am
    return dict(input_ids=ids, attention_mask=am, labels=torch.where(am.bool(), ids, -100), padding_free=kind == "pf")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def train_configs():
    """Every axis with every family; streams x aux_side x recompute x buckets as a full product."""
    # bk: "no" = backward without a bucket callback, else bucket_layers 0 | 1 | 2 with one (0: only the l <= 2 rule cuts buckets)
    for two, aux, rc, bk in itertools.product((1, 0), (1, 0), (0, 1, 2), ("no", 0, 1, 2)):
        yield dict(batch="packed", two=two, aux=aux, rc=rc, bk=bk)
    for kind, rc in itertools.product(("dense", "pf"), (0, 2)):
        yield dict(batch=kind, rc=rc)
    for fs, fd, two in itertools.product((1, 0), (1, 0), (1, 0)):
        yield dict(batch="dense", fuse_swiglu=fs, fuse_dswiglu=fd, two=two)
    # a storing backward (grad_overwrite_next), then one that adds to it and is final 0 | 1 | 2 with a gradient image bound
    for fin, rc, two in itertools.product((0, 1, 2), (0, 2), (1, 0)):
        yield dict(batch="packed", acc=1, fin=fin, rc=rc, two=two)


def tag_of(body, c):
    return body + "/" + ".".join(f"{k}{v}" if k != "batch" else v for k, v in c.items())


def run_train(m, c):
    e = m.engine
    for k, opt in (("two", "bwd_wgrad_stream"), ("aux", "bwd_aux_side"), ("fuse_swiglu", "fuse_swiglu"), ("fuse_dswiglu", "fuse_dswiglu")):
        e.set_option(opt, c.get(k, 1))
    if c.get("rc", 0):
        m.gradient_checkpointing_enable(level=c["rc"])
    else:
        m.gradient_checkpointing_disable()
    vocab = m.config.vocab_size
    calls = []
    bk = c.get("bk", "no")
    cb = (lambda off, cnt, stream=None: calls.append((off, cnt, stream is None))) if bk != "no" else None
    m.set_dropout_state(seed=3, call=2)
    img = None
    if c.get("acc"):
        first, last = batch("dense", vocab, 4), batch(c["batch"], vocab, 5)
        n = float(sum(int((b["labels"][:, 1:] != -100).sum()) for b in (first, last)))
        e.set_option("grad_overwrite_next", 1)
        m(**first, num_items_in_batch=n, return_logits=False)
        m.backward()
        out = m(**last, num_items_in_batch=n)
        img = m.enable_bf16_grads().zero_()
        e.set_grad_image(img)  # final 0 and 1 write it next to the fp32 values, 2 instead of them
        m.backward(1.0, final=c["fin"])
    else:
        m.zero_grad()
        out = m(**batch(c["batch"], vocab, 1))
        m.backward(1.0, 0 if cb is None else bk, cb)
    norm = torch.zeros(2, device=m.device)
    e.grad_norm(0.5, norm)
    torch.cuda.synchronize()
    parts = [f"loss {sha(out.loss)}", f"logits {sha(out.logits)}", f"grads {sha(m.flat_grads)}", f"norm {sha(norm)}"]
    if img is not None:
        parts.append(f"image {sha(img)}")
    if cb:
        parts.append(f"buckets {calls}")
    return " ".join(parts)


def run_cached(m, rc):
    """prefill, eight greedy decode steps, slam_extend at B T <= 64 and beyond (the tiled GEMM and the fused-RoPE projection take
    over there), slam_extend_score"""
    if rc:
        m.gradient_checkpointing_enable(level=rc)
    else:
        m.gradient_checkpointing_disable()
    e, dev, V = m.engine, m.device, m.config.vocab_size
    B, T, cap = 3, 32, 256
    g = torch.Generator().manual_seed(21)
    draw = lambda t: torch.randint(2, V, (B, t), generator=g).to(dev)  # noqa: E731
    cache = torch.zeros(e.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    e.bind_kv_cache(cache, B, cap)
    m(input_ids=batch("dense", V, 1)["input_ids"])  # a level switch unbinds the workspace: any forward binds it again
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    lens = torch.tensor([32, 20, 7], dtype=torch.int32, device=dev)
    e.prefill(draw(T), lens, B, T, logits)
    parts = [f"prefill {sha(logits)}"]
    steps = []
    for _ in range(8):
        e.decode_step(logits.argmax(-1).contiguous(), lens, B, logits)
        steps.append(logits.clone())
    parts.append(f"decode {sha(torch.stack(steps))}")
    for t, new in ((16, [16, 11, 0]), (40, [40, 1, 33])):
        e.extend(draw(t), torch.tensor(new, dtype=torch.int32, device=dev), lens, B, t, logits)
        parts.append(f"extend{B * t} {sha(logits)}")
    lp = torch.zeros(B, 16, dtype=torch.float32, device=dev)
    am = torch.zeros(B, 16, dtype=torch.int64, device=dev)
    e.extend_score(draw(16), torch.tensor([16, 0, 9], dtype=torch.int32, device=dev), lens, B, 16, logits, lp, am)
    torch.cuda.synchronize()
    parts.append(f"score {sha(logits)} {sha(lp)} {sha(am)} kv {sha(cache)}")
    return " ".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    for body in BODIES:
        jobs = [(tag_of(body, c), c) for c in train_configs()]
        jobs += [(f"{body}/cached.rc{rc}", rc) for rc in (0, 2)] if body in CACHED else []
        jobs = [j for j in jobs if a.only in (None, j[0])]
        if a.list:
            print("\n".join(t for t, _ in jobs))
        elif jobs:
            torch.cuda.set_device(0)
            m = build(body)
            for tag, c in jobs:
                print(tag, run_train(m, c) if isinstance(c, dict) else run_cached(m, c), flush=True)


if __name__ == "__main__":
    main()
