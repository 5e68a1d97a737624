"""Training-step throughput of the OPT decoder family (engine arch 1): tokens/s of a full optimizer step - forward, backward,
clip 0.5 and AdamW on bf16 parameters with bf16 moments (the Slam recipe's precision) - through SLAMTrainer.optimizer_step,
as bench.py times Slam-358M. Shapes: OPT-125m at the reference defaults (B 8 x T 512, config/model/default.yaml context_len)
and OPT-1.3B (the TWIST-1.3B body) at B 8 x T 1024; 502-row unit vocabulary, seeded synthetic tokens, random-init weights.

    python tools/opt_bench.py [--shapes 125m,1.3b] [--steps 20] [--warmup 5] [--seed 0] [--dropout P] [--seq-len T]
    python tools/opt_bench.py --kernel-rates

--dropout P trains with residual dropout (HF OPTConfig.dropout, 0.1 by default there), --seq-len overrides the shapes'
sequence lengths. --kernel-rates times the two dropout kernels on their own at (8192, 768) and (8192, 2048) and prints their
achieved GB/s (forward: two reads and a write of M x H bf16; backward: one read and a write).

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


def kernel_rates(iters: int = 50) -> list:
    """Achieved GB/s of dropout_add / dropout_bwd alone: `iters` back-to-back launches between two events, buffers rotated
    through more memory than the last-level cache holds so that every pass streams from HBM."""
    import ctypes as C
    from slamkit_amd import engine as E
    lib, st = E.load_library(), E.current_stream_ptr()
    out = []
    for M, H in ((8192, 768), (8192, 2048)):
        nbuf = max(2, (1 << 30) // (3 * M * H * 2))  # ~1 GiB of distinct y / resid / out buffers in rotation
        bufs = [[torch.randn(M, H, device="cuda").to(torch.bfloat16) for _ in range(3)] for _ in range(nbuf)]
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        for name, nbytes, call in (
                ("dropout_add", 3 * M * H * 2, lambda b, i: lib.slam_op_dropout_add(p(b[0]), p(b[1]), M, H, 6554, 1, i, 0, 0, st)),
                ("dropout_bwd", 2 * M * H * 2, lambda b, i: lib.slam_op_dropout_bwd(p(b[0]), p(b[2]), M, H, 6554, 1, i, 0, 0, st))):
            for i in range(5):
                assert call(bufs[i % nbuf], i) == 0
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                call(bufs[i % nbuf], i)
            b.record()
            torch.cuda.synchronize()
            us = 1e3 * a.elapsed_time(b) / iters
            out.append({"kernel": name, "M": M, "H": H, "us": round(us, 2), "GB_per_s": round(nbytes / us / 1e3, 1)})
        del bufs
        torch.cuda.empty_cache()
    return out


def run(name: str, steps: int, warmup: int, seed: int, dropout: float = 0.0, seq_len: int = 0) -> dict:
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    base, B, T = SHAPES[name]
    T = seq_len or T
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = {"dropout": dropout} if dropout else {}
    model = UnitLM(UnitLMConfig(base_model_name=base, vocab_size=V, max_tokens=B * T, **kw), seed=seed)
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
            "loss": round(float(trainer._loss_acc) / max(1, trainer._loss_n), 4), "dropout": dropout,
            "device": torch.cuda.get_device_name(dev)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="125m,1.3b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=0.0, help="residual dropout probability (OPTConfig.dropout)")
    ap.add_argument("--seq-len", type=int, default=0, help="override the shapes' sequence length")
    ap.add_argument("--kernel-rates", action="store_true", help="time the two dropout kernels alone instead of the step")
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    if a.kernel_rates:
        for r in kernel_rates():
            print(json.dumps(r), flush=True)
        return
    for s in a.shapes.split(","):
        print(json.dumps(run(s, a.steps, a.warmup, a.seed, a.dropout, a.seq_len)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
