"""Training-step throughput of the Qwen2.5-7B body (SIMS-7B: hidden 3584, 28 / 4 heads of 128, intermediate 18944, untied
lm_head) with its 152,064-row vocabulary: tokens/s of a full optimizer step - forward, backward, clip 0.5 and AdamW on bf16
parameters with bf16 moments (the recipe's precision) - through SLAMTrainer.optimizer_step, as bench.py times Slam-358M. One
packed micro-batch of --tokens tokens in sequences of --ctx (the interleaved model's layout), seeded synthetic tokens,
random-init weights. The body runs at reduced depth (--layers, default 4); --layers 4,28 adds the full depth, which is
reported as not fitting (one JSON line with "error") when the device runs out of memory.

    python tools/wide_bench.py [--layers 4] [--tokens 16384] [--ctx 2048] [--steps 10] [--warmup 3] [--seed 0] [--recompute 0]

--recompute 1 | 2 runs the step with activation recomputation in backward (UnitLM.gradient_checkpointing_enable(level)).

Prints one JSON line per depth: tokens/s from the wall time of the timed steps (device-synchronised before and after), the
median per-step device time, the loss, the recomputation level, the bytes of the bound engine workspace and the peak device
memory torch allocated.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 152064
BASE = "Qwen/Qwen2.5-7B"


def run(layers: int, tokens: int, ctx: int, steps: int, warmup: int, seed: int, recompute: int = 0) -> dict:
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.reset_peak_memory_stats(dev)
    base = dict(KNOWN_BASE_CONFIGS[BASE], num_hidden_layers=layers)
    # with recomputation the full-size workspace is bound by the first step, in the level's layout: the constructor's own
    # (level 0) workspace stays small, so the peak below is the level's
    model = UnitLM(UnitLMConfig(base_model_name=BASE, base_config=base, vocab_size=V, max_tokens=ctx if recompute else tokens), seed=seed)
    if recompute:
        model.gradient_checkpointing_enable(level=recompute)
    args = SLAMTrainingArguments(per_device_train_batch_size=1, gradient_accumulation_steps=1, learning_rate=1e-4,
                                 max_grad_norm=0.5, logging_steps=0, optim_state_dtype="bfloat16")
    trainer = SLAMTrainer(model=model, args=args)  # drops the fp32 master: the bf16 parameters are the state
    torch.cuda.empty_cache()
    nseq = tokens // ctx
    pos = torch.arange(ctx).repeat(nseq)[None].to(dev)
    batches = []
    for i in range(4):
        g = torch.Generator().manual_seed(seed * 1000 + i)
        ids = torch.randint(2, V, (1, nseq * ctx), generator=g)
        ids[0, ::ctx] = 1
        lab = ids.clone()
        lab[0, ::ctx] = -100
        batches.append([{"input_ids": ids.to(dev), "position_ids": pos, "labels": lab.to(dev)}])
    n = float(nseq * (ctx - 1))
    ahead = {"h": trainer.post_counts(n, n)}

    def step(i):
        h, ahead["h"] = ahead["h"], trainer.post_counts(n, n)
        trainer.optimizer_step(batches[i % len(batches)], 1e-4, counts=(n, n), counts_handle=h)

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(steps):
        step(warmup + i)
        marks[i + 1].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return {"model": BASE, "layers": layers, "tokens": nseq * ctx, "ctx": ctx, "vocab": V, "steps": steps, "warmup": warmup,
            "params": model.engine.n_params, "tokens_per_s": round(nseq * ctx * steps / dt, 1),
            "ms_per_step": round(1e3 * dt / steps, 3), "ms_per_step_median": round(per[len(per) // 2], 3),
            "loss": round(float(trainer._loss_acc) / max(1, trainer._loss_n), 4),
            "recompute": recompute, "workspace_bytes": model.engine.workspace_bytes(model._ws_tokens),
            "peak_device_memory_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2),
            "device": torch.cuda.get_device_name(dev)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="4", help="comma-separated depths, e.g. 4,28")
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--recompute", type=int, default=0, choices=(0, 1, 2), help="activation recomputation level in backward")
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    for layers in (int(x) for x in a.layers.split(",")):
        try:
            res = run(layers, a.tokens, a.ctx, a.steps, a.warmup, a.seed, a.recompute)
        except torch.cuda.OutOfMemoryError as e:  # reported, not hidden: the depth does not fit this device
            res = {"model": BASE, "layers": layers, "tokens": a.tokens, "error": "out of device memory",
                   "detail": str(e).splitlines()[0][:200],
                   "peak_device_memory_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
