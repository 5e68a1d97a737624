"""Training-step time of the GPT-NeoX decoder family (engine arch 4) with the fused LayerNorm pair (option "neox_split_ln" = 0) and
with the two single launches (= 1): a full optimizer step - forward, backward, clip 0.5 and AdamW on bf16 parameters with bf16
moments - through SLAMTrainer.optimizer_step, as tools/opt_bench.py times OPT. Shapes: pythia-160m at B 8 x T 1024 and
pythia-410m at B 8 x T 1024; 502-row unit vocabulary, seeded synthetic tokens, random-init weights.

    python tools/neox_bench.py [--shapes 160m,410m] [--steps 20] [--warmup 5] [--rounds 3] [--seed 0]

One process and one model per shape; the two settings alternate A / B / A / B .. for `rounds` rounds of `steps` timed steps each
(the option is read by the forward, so a switch between two steps is clean). Prints one JSON line per shape: per setting the
median device time of a step over all its rounds and the spread (min .. max) of the rounds' medians, tokens/s from the median.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 502
SHAPES = {"160m": ("EleutherAI/pythia-160m", 8, 1024), "410m": ("EleutherAI/pythia-410m", 8, 1024)}


def run(name: str, steps: int, warmup: int, rounds: int, seed: int) -> dict:
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
    count = [0]

    def step():
        h, ahead["h"] = ahead["h"], trainer.post_counts(n, n)
        trainer.optimizer_step(batches[count[0] % len(batches)], 1e-4, counts=(n, n), counts_handle=h)
        count[0] += 1

    def timed(split: int) -> float:
        torch.cuda.synchronize()
        model.engine.set_option("neox_split_ln", split)
        for _ in range(warmup):
            step()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        marks[0].record()
        for i in range(steps):
            step()
            marks[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
        return per[len(per) // 2]

    med = {0: [], 1: []}
    for _ in range(rounds):
        for split in (0, 1):
            med[split].append(timed(split))
    out = {"model": base, "batch": B, "seq_len": T, "steps": steps, "warmup": warmup, "rounds": rounds,
           "params": model.engine.n_params, "device": torch.cuda.get_device_name(dev)}
    for split, key in ((0, "dual_ln"), (1, "split_ln")):
        m = sorted(med[split])
        mid = m[len(m) // 2]
        out[key] = {"ms_per_step_median": round(mid, 3), "round_medians_ms": [round(x, 3) for x in med[split]],
                    "spread_ms": [round(m[0], 3), round(m[-1], 3)], "tokens_per_s": round(B * T / mid * 1e3, 1)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="160m,410m")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    for s in a.shapes.split(","):
        print(json.dumps(run(s, a.steps, a.warmup, a.rounds, a.seed)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
