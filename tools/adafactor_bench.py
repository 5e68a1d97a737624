"""Adafactor against AdamW on one GPU: the optimizer phase, the whole optimizer step and the peak device memory.

    python tools/adafactor_bench.py [--shape slam358m | qwen7b] [--layers N] [--tokens 8192] [--ctx 1024] [--state bfloat16 | float32]
                                    [--recompute 0 | 1 | 2] [--steps 10] [--warmup 3] [--rounds 5] [--iters 20] [--out DIR]
                                    [--trace-steps N]

Two phases in one process, each with a model of its own so that the peak is the optimizer's: SLAMTrainer under optim =
"adafactor", then under "adamw_torch", the same seeded packed micro-batch (one of --tokens tokens in sequences of --ctx), the same
optim_state_dtype. Per phase: the median device time of --steps whole optimizer steps (forward, backward, clip, update) through
SLAMTrainer.optimizer_step, and torch's peak allocated memory. In the AdamW phase the engine is then given an Adafactor segment
table, state and workspace of its own as well, and windows of --iters optimizer phases (slam_grad_norm + the update, on the
gradients the last backward left, zero_grad off) of the two optimizers alternate for --rounds rounds after 3 warm-up calls each:
median, min and max per optimizer, so that the spread stands beside the difference.

Also printed: the bytes each Adafactor pass moves by design (from the shapes; the factor and partial arrays are below 1 % of a
pass and left out) beside the floor of one gradient read and one parameter read and write.

--trace-steps N: only N Adafactor optimizer phases after one real step - the run to put under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/adafactor_bench.py --trace-steps 20): the af_* kernels are the six passes.
One JSON line on stdout; with --out the same as adafactor_bench.json and a markdown table."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"slam358m": ("Qwen/Qwen2.5-0.5B", 502), "qwen7b": ("Qwen/Qwen2.5-7B", 152064)}


def build(a, optim):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    name, vocab = SHAPES[a.shape]
    base = dict(KNOWN_BASE_CONFIGS[name])
    if a.layers:
        base["num_hidden_layers"] = a.layers
    model = UnitLM(UnitLMConfig(base_model_name=name, base_config=base, vocab_size=vocab, max_tokens=a.ctx if a.recompute else a.tokens),
                   seed=a.seed)
    if a.recompute:
        model.gradient_checkpointing_enable(level=a.recompute)
    args = SLAMTrainingArguments(per_device_train_batch_size=1, gradient_accumulation_steps=1, learning_rate=1e-4, max_grad_norm=0.5,
                                 logging_steps=0, optim_state_dtype=a.state, optim=optim)
    return model, SLAMTrainer(model=model, args=args), vocab


def batches(a, vocab, dev):
    nseq = a.tokens // a.ctx
    pos = torch.arange(a.ctx).repeat(nseq)[None].to(dev)
    out = []
    for i in range(4):
        g = torch.Generator().manual_seed(a.seed * 1000 + i)
        ids = torch.randint(2, vocab, (1, nseq * a.ctx), generator=g)
        ids[0, ::a.ctx] = 1
        lab = ids.clone()
        lab[0, ::a.ctx] = -100
        out.append([{"input_ids": ids.to(dev), "position_ids": pos, "labels": lab.to(dev)}])
    return out, float(nseq * (a.ctx - 1))


def whole_steps(a, trainer, bs, n, steps, warmup):
    ahead = {"h": trainer.post_counts(n, n)}

    def step(i):
        h, ahead["h"] = ahead["h"], trainer.post_counts(n, n)
        trainer.optimizer_step(bs[i % len(bs)], 1e-4, counts=(n, n), counts_handle=h)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        step(warmup + i)
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return per[len(per) // 2], per[0], per[-1]


def pass_bytes(model, state_dtype, g_bytes):
    """bytes each pass moves by design, from the segment shapes"""
    n = sum(s.rows * s.cols for s in model.hf_param_segments())
    n_fact = sum(s.rows * s.cols for s in model.hf_param_segments() if s.factored)
    p_rw = (4 + 4 + 2) if state_dtype == "float32" else (2 + 2)   # master read + write and the bf16 copy, or the bf16 parameters both ways
    return {"elements": n, "af_sums_kernel": n_fact * g_bytes, "af_usq_kernel": n * g_bytes, "af_apply_kernel": n * (g_bytes + p_rw),
            "floor_one_g_read_p_read_write": n * (g_bytes + p_rw)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="slam358m", choices=sorted(SHAPES))
    ap.add_argument("--layers", type=int, default=0, help="override the body's depth (0: the shape's own)")
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--state", default="bfloat16", choices=("bfloat16", "float32"))
    ap.add_argument("--recompute", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"shape": a.shape, "layers": a.layers, "tokens": a.tokens, "ctx": a.ctx, "state": a.state, "recompute": a.recompute,
           "device": torch.cuda.get_device_name(dev)}
    if a.trace_steps:
        model, tr, vocab = build(a, "adafactor")
        bs, n = batches(a, vocab, dev)
        whole_steps(a, tr, bs, n, 1, 1)
        for _ in range(a.trace_steps):
            tr._clip_and_update(1e-6, zero_grad=False)
        torch.cuda.synchronize()
        res.update(traced_phases=a.trace_steps, params=model.engine.n_params,
                   pass_bytes=pass_bytes(model, a.state, 2 if a.state == "bfloat16" else 4))
        print(json.dumps(res), flush=True)
        return
    for optim in ("adafactor", "adamw_torch"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        model, tr, vocab = build(a, optim)
        bs, n = batches(a, vocab, dev)
        med, lo, hi = whole_steps(a, tr, bs, n, a.steps, a.warmup)
        res[optim] = {"step_ms_median": round(med, 3), "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3),
                      "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3)}
        res["params"] = model.engine.n_params
        if optim == "adamw_torch":   # the optimizer phases alone, alternating, on this model's buffers and the last backward's gradients
            eng = model.engine
            g_bytes = 2 if getattr(model, "_grads_in_bf16", False) else 4
            n_state, ws_bytes = eng.adafactor_set_segments([s.entry for s in model.hf_param_segments()])
            st = torch.zeros(n_state, dtype=torch.float32, device=dev)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            eng.adafactor_bind_workspace(ws)
            master = None if a.state == "bfloat16" else model.flat_master
            k = {"t": tr.opt_step}

            def phase(which):
                k["t"] += 1
                eng.grad_norm(0.5, tr.norm_out)
                if which == "adafactor":
                    eng.adafactor_step(master, st, tr.norm_out, 1e-6, k["t"], zero_grad=False)
                elif master is None:
                    eng.adamw_step_bf16(tr.exp_avg, tr.exp_avg_sq, tr.norm_out, 1e-6, 0.9, 0.999, 1e-8, 0.0, k["t"], zero_grad=False)
                else:
                    eng.adamw_step(master, tr.exp_avg, tr.exp_avg_sq, tr.norm_out, 1e-6, 0.9, 0.999, 1e-8, 0.0, k["t"], zero_grad=False)

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
            win = {"adamw": [], "adafactor": []}
            for _ in range(a.rounds):
                for which in win:
                    win[which].append(window(which))
            res["optimizer_phase_us"] = {w: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                         for w, v in win.items()}
            res["adafactor_state_floats"], res["adafactor_workspace_bytes"], res["gradient_bytes"] = n_state, ws_bytes, g_bytes
            res["pass_bytes"] = pass_bytes(model, a.state, g_bytes)
        del tr, model, bs
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"adafactor_bench_{a.shape}_{a.state}.json"), "w") as f:
            json.dump(res, f, indent=1)
        ph = res["optimizer_phase_us"]
        lines = ["| optimizer | optimizer phase us (min .. max) | whole step ms (min .. max) | peak allocated GB |", "|---|---|---|---|"]
        for o, w in (("adamw_torch", "adamw"), ("adafactor", "adafactor")):
            lines.append(f"| {o} | {ph[w]['median']} ({ph[w]['min']} .. {ph[w]['max']}) | {res[o]['step_ms_median']} "
                         f"({res[o]['step_ms_min']} .. {res[o]['step_ms_max']}) | {res[o]['peak_allocated_gb']} |")
        with open(os.path.join(a.out, f"adafactor_bench_{a.shape}_{a.state}.md"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
