"""8-bit block-wise AdamW state (optim = "adamw_bnb_8bit") against bf16-state AdamW on one GPU: the optimizer phase, the whole
optimizer step and the peak device memory. A sibling of tools/adafactor_bench.py, whose model, batches and step timing it uses.

    python tools/adam8_bench.py [--shape slam358m | qwen7b] [--layers N] [--tokens 8192] [--ctx 1024] [--recompute 0 | 1 | 2]
                                [--steps 10] [--warmup 3] [--rounds 5] [--iters 20] [--out DIR]

Three phases in one process, each with a model of its own so that the peak is the optimizer's: SLAMTrainer under "adamw_torch",
under "adamw_bnb_8bit", and under "adamw_torch" again (A, B, A: the two A phases show the drift of the process beside the
difference), optim_state_dtype bfloat16, the same seeded packed micro-batch. Per phase: the median device time of --steps whole
optimizer steps and torch's peak allocated memory. In the last phase the engine is given 8-bit allocations of its own as well, and
windows of --iters optimizer phases (slam_grad_norm + the update on the gradients the last backward left, zero_grad off) of the
two forms alternate for --rounds rounds after 3 warm-up calls each: median, min and max per form.
One JSON line on stdout; with --out the same as adam8_bench_<shape>.json."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adafactor_bench as AB  # noqa: E402


def main(argv=None):
    ap = AB.argparse.ArgumentParser()
    ap.add_argument("--shape", default="slam358m", choices=sorted(AB.SHAPES))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--recompute", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    a.state = "bfloat16"
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"shape": a.shape, "layers": a.layers, "tokens": a.tokens, "ctx": a.ctx, "recompute": a.recompute,
           "device": torch.cuda.get_device_name(dev), "phases": []}
    for i, optim in enumerate(("adamw_torch", "adamw_bnb_8bit", "adamw_torch")):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        model, tr, vocab = AB.build(a, optim)
        bs, n = AB.batches(a, vocab, dev)
        med, lo, hi = AB.whole_steps(a, tr, bs, n, a.steps, a.warmup)
        res["phases"].append({"optim": optim, "step_ms_median": round(med, 3), "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3),
                              "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3),
                              "state_bytes": tr.optimizer.state_bytes[0]})
        res["params"] = model.engine.n_params
        if i == 2:   # the optimizer phases alone, alternating, on this model's buffers and the last backward's gradients
            eng = model.engine
            q8 = [torch.zeros(eng.adam8_state_layout(eng.n_params)[0], dtype=torch.uint8, device=dev) for _ in range(2)]
            k = {"t": tr.opt_step}

            def phase(which):
                k["t"] += 1
                eng.grad_norm(0.5, tr.norm_out)
                eng.set_option("adamw_state8", int(which == "adamw_8bit"))
                m, v = q8 if which == "adamw_8bit" else (tr.exp_avg, tr.exp_avg_sq)
                eng.adamw_step_bf16(m, v, tr.norm_out, 1e-6, 0.9, 0.999, 1e-8, 0.0, k["t"], zero_grad=False)
                eng.set_option("adamw_state8", 0)

            def window(which):
                for _ in range(3):
                    phase(which)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    phase(which)
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1) * 1e3 / a.iters   # us per optimizer phase
            win = {"adamw": [], "adamw_8bit": []}
            for _ in range(a.rounds):
                for which in win:
                    win[which].append(window(which))
            res["optimizer_phase_us"] = {w: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                         for w, v in win.items()}
            res["gradient_bytes"] = 2 if getattr(model, "_grads_in_bf16", False) else 4
            del q8
        del tr, model, bs
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"adam8_bench_{a.shape}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
