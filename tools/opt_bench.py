"""Training-step throughput of the OPT decoder family (engine arch 1): tokens/s of a full optimizer step - forward, backward,
clip 0.5 and AdamW on bf16 parameters with bf16 moments (the Slam recipe's precision) - through SLAMTrainer.optimizer_step,
as bench.py times Slam-358M. Shapes: OPT-125m at the reference defaults (B 8 x T 512, config/model/default.yaml context_len)
and OPT-1.3B (the TWIST-1.3B body) at B 8 x T 1024; 502-row unit vocabulary, seeded synthetic tokens, random-init weights.

    python tools/opt_bench.py [--shapes 125m,1.3b] [--steps 20] [--warmup 5] [--seed 0]

Prints one JSON line per shape: tokens/s from the wall time of the timed steps (device-synchronised before and after), the
median per-step device time, the loss.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 502
SHAPES = {"125m": ("facebook/opt-125m", 8, 512), "1.3b": ("facebook/opt-1.3b", 8, 1024)}


def run(name: str, steps: int, warmup: int, seed: int) -> dict:
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    base, B, T = SHAPES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    model = UnitLM(UnitLMConfig(base_model_name=base, vocab_size=V, max_tokens=B * T), seed=seed)
    args = SLAMTrainingArguments(per_device_train_batch_size=B, gradient_accumulation_steps=1, learning_rate=1e-4,
                                 max_grad_norm=0.5, logging_steps=0, optim_state_dtype="bfloat16")
    trainer = SLAMTrainer(model=model, args=args)
    batches = []
    for i in range(4):
        g = torch.Generator().manual_seed(seed * 1000 + i)
        ids = torch.randint(2, V, (B, T), generator=g)
        ids[:, 0] = 1
        ids = ids.to(dev)
        batches.append([{"input_ids": ids, "labels": ids}])
    n = float(B * T)
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
    return {"model": base, "batch": B, "seq_len": T, "steps": steps, "warmup": warmup, "params": model.engine.n_params,
            "tokens_per_s": round(B * T * steps / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3),
            "ms_per_step_median": round(per[len(per) // 2], 3),
            "loss": round(float(trainer._loss_acc) / max(1, trainer._loss_n), 4),
            "device": torch.cuda.get_device_name(dev)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="125m,1.3b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    for s in a.shapes.split(","):
        print(json.dumps(run(s, a.steps, a.warmup, a.seed)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
