"""Muon against AdamW on one GPU: the optimizer phase, the whole optimizer step, the peak device memory and the FLOP/s of the
two batched product kernels per shape class.

    python tools/muon_bench.py [--shape slam358m | qwen1p5b] [--layers N] [--tokens 8192] [--ctx 1024] [--state bfloat16 | float32]
                               [--steps 10] [--warmup 3] [--iters 10] [--out DIR]
    python tools/muon_bench.py --loss-curve 300            # a tiny model, AdamW and Muon on the same data and schedule

One process, A - B - A: a model and a trainer are built under "adamw_torch", then under "muon", then under "adamw_torch" again,
the same seeded packed micro-batch (one of --tokens tokens in sequences of --ctx), the same warm-up. Per build: the median / min /
max of --steps whole optimizer steps (forward + backward + clip + update, through SLAMTrainer.optimizer_step), the median of
--iters optimizer phases alone (SLAMTrainer._clip_and_update on the last backward's gradients, lr 1e-6) and torch's peak
allocated memory. Then, on buffers of the model's own shape classes, the two product kernels alone: A = X X^T, P = b A + c A A
(the symmetric kernel) and X <- a X + P X, each timed over --iters launches of the class's whole batch. FLOP/s are given for the
dense count (2 n n m, 2 n n n) - the symmetric kernel computes only the tiles on or below the diagonal, so its executed count is
lower; both are printed. One JSON line on stdout; with --out the same as muon_bench_<shape>_<state>.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"slam358m": ("Qwen/Qwen2.5-0.5B", 502), "qwen1p5b": ("Qwen/Qwen2.5-1.5B", 502)}


def build(a, optim):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    name, vocab = SHAPES[a.shape]
    base = dict(KNOWN_BASE_CONFIGS[name])
    if a.layers:
        base["num_hidden_layers"] = a.layers
    model = UnitLM(UnitLMConfig(base_model_name=name, base_config=base, vocab_size=vocab, max_tokens=a.tokens), seed=a.seed)
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


def whole_steps(trainer, bs, n, steps, warmup):
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


def phases(trainer, iters):
    per = []
    for i in range(iters + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        trainer._clip_and_update(1e-6, zero_grad=False)
        t1.record()
        t1.synchronize()
        if i >= 2:
            per.append(t0.elapsed_time(t1))
    return statistics.median(per), min(per), max(per)


def product_kernels(classes, iters, dev):
    """Per shape class (rows, cols, count): ms and FLOP/s of the class's batch through each product launch."""
    from slamkit_amd import engine as E
    out = []
    for rows, cols, count in classes:
        n, m = min(rows, cols), max(rows, cols)
        x = (torch.randn(count, n, m, device=dev) / m ** 0.5).to(torch.bfloat16)
        y = torch.empty_like(x)
        g = torch.empty(count, n, n, dtype=torch.bfloat16, device=dev)
        p = torch.empty_like(g)

        def timed(fn):
            for _ in range(2):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / iters
        ms_gram = timed(lambda: E.muon_syrk(x, None, g, count, n, m, n * m, 0, n * n, 1.0, 0.0))
        ms_poly = timed(lambda: E.muon_syrk(g, g, p, count, n, n, n * n, n * n, n * n, 2.0315, -4.7750))
        ms_prod = timed(lambda: E.muon_mm(p, x, x, y, count, n, m, n * n, n * m, n * m, n * m, 1.0, 3.4445))
        t = (n + 127) // 128
        tri = t * (t + 1) / 2 / (t * t)     # the fraction of output tiles the symmetric kernel computes
        dense = {"gram": 2.0 * n * n * m * count, "poly": 2.0 * n * n * n * count, "prod": 2.0 * n * n * m * count}
        out.append({"rows": rows, "cols": cols, "count": count,
                    "gram_ms": round(ms_gram, 4), "gram_dense_tflops": round(dense["gram"] / ms_gram * 1e-9, 1),
                    "gram_executed_tflops": round(dense["gram"] * tri / ms_gram * 1e-9, 1),
                    "poly_ms": round(ms_poly, 4), "poly_dense_tflops": round(dense["poly"] / ms_poly * 1e-9, 1),
                    "poly_executed_tflops": round(dense["poly"] * tri / ms_poly * 1e-9, 1),
                    "prod_ms": round(ms_prod, 4), "prod_tflops": round(dense["prod"] / ms_prod * 1e-9, 1),
                    "ns5_dense_tflop": round(5 * sum(dense.values()) * 1e-12, 3)})
    return out


def loss_curve(steps, dev):
    """A 2-layer 256-wide Qwen2 body on 64 random sequences: the logged loss of AdamW and of Muon, same data, seed and schedule."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    base = dict(num_hidden_layers=2, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, intermediate_size=512,
                rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    g = torch.Generator().manual_seed(0)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (63,), generator=g).tolist(), "attention_mask": [1] * 64} for _ in range(64)]
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)
    out = {}
    for optim in ("adamw_torch", "muon"):
        model = UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(base), vocab_size=502, max_tokens=1024), seed=1)
        args = SLAMTrainingArguments(per_device_train_batch_size=8, max_steps=steps, num_train_epochs=steps, warmup_ratio=0.05,
                                     learning_rate=1e-3, lr_scheduler_type="cosine_with_min_lr", lr_scheduler_kwargs={"min_lr": 5e-5},
                                     max_grad_norm=0.5, weight_decay=0.0, logging_steps=20, seed=7, output_dir="/tmp/unused", optim=optim)
        tr = SLAMTrainer(model=model, args=args, data_collator=coll, train_dataset=ds)
        st = tr.train()
        out[optim] = [round(r["loss"], 4) for r in st.log_history if "loss" in r]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="slam358m", choices=sorted(SHAPES))
    ap.add_argument("--layers", type=int, default=0, help="override the body's depth (0: the shape's own)")
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--state", default="bfloat16", choices=("bfloat16", "float32"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loss-curve", type=int, default=0, help="only the tiny-model loss curves over this many steps")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    dev = torch.device("cuda", torch.cuda.current_device())
    if a.loss_curve:
        print(json.dumps({"loss_every_20_steps": loss_curve(a.loss_curve, dev)}), flush=True)
        return
    res = {"shape": a.shape, "layers": a.layers, "tokens": a.tokens, "ctx": a.ctx, "state": a.state, "device": torch.cuda.get_device_name(dev),
           "runs": []}
    classes = None
    for optim in ("adamw_torch", "muon", "adamw_torch"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        model, tr, vocab = build(a, optim)
        bs, n = batches(a, vocab, dev)
        med, lo, hi = whole_steps(tr, bs, n, a.steps, a.warmup)
        pm, pl, ph = phases(tr, a.iters)
        run = {"optim": optim, "step_ms_median": round(med, 3), "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3),
               "optimizer_phase_ms_median": round(pm, 3), "optimizer_phase_ms_min": round(pl, 3), "optimizer_phase_ms_max": round(ph, 3),
               "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3)}
        if optim == "muon":
            run["state_bytes"], run["workspace_bytes"] = tr.optimizer_state_bytes
            run["adamw_ranges"] = len(tr._adamw_runs)
            classes = [(c.rows, c.cols, c.count) for c in model.engine.muon_classes()]
            run["launches_per_step"] = 2 + len(classes) * (1 + 3 * tr.args.muon_ns_steps)
        res["runs"].append(run)
        res["params"] = model.engine.n_params
        del tr, model, bs
    torch.cuda.empty_cache()
    res["product_kernels"] = product_kernels(classes, a.iters, dev)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"muon_bench_{a.shape}_{a.state}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
