"""Time the AdamW step with and without the no-decay mask (slam_set_decay_mask, weight_decay_rule = "hf") on one GPU.

    python tools/decay_rule_bench.py [--out out/decay_rule] [--rounds 7] [--iters 100]

Slam-358M shape, bf16 state (slam_adamw_step_bf16 / slam_adamw_range_bf16), with fp32 gradients and with the bf16-kept
gradients of a real backward (final = 2). Three forms: the fused walk that writes the transposed images (mask decided on the
host: the launches are the same kernels, some with wd = 0), the flat kernel followed by the transpose pass ("fuse_adamw_t" =
0), and the flat kernel alone over the whole buffer as one range (the masked kernel's own cost, nothing else in the window).
Mask off and on alternate round by round in one process; a window is `iters` steps between two device events after 3 warm-up
steps. Prints one table (median, min, max per form and the off-run spread) and writes it with the raw windows as JSON."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "decay_rule"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    from slamkit_amd.model import UnitLM, UnitLMConfig
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    m = UnitLM(UnitLMConfig(base_model_name="Qwen/Qwen2.5-0.5B", vocab_size=502, max_tokens=1024), seed=0)
    eng, n = m.engine, m.engine.n_params
    flags = m.hf_decay_flags()
    n_ranges = sum(1 for f0, f1 in zip([True] + flags, flags) if f0 and not f1)
    gen = torch.Generator(device="cuda").manual_seed(0)
    ea = (torch.randn(n, device="cuda", generator=gen) * 1e-3).bfloat16()
    eq = (torch.randn(n, device="cuda", generator=gen) * 1e-3).abs().bfloat16()
    norm = torch.tensor([1.0, 1.0], dtype=torch.float32, device="cuda")
    hyper = (norm, 1e-5, 0.9, 0.999, 1e-8, 0.1)
    state = {"step": 0}

    def one(form):
        state["step"] += 1
        if form == "range":
            eng.adamw_range(0, n, None, ea, eq, *hyper, state["step"], zero_grad=False)
        else:
            eng.adamw_step_bf16(ea, eq, *hyper, state["step"], zero_grad=False)

    def window(form):
        for _ in range(3):
            one(form)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            one(form)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.iters  # us per step

    rows = []
    for grads in ("fp32", "bf16"):
        if grads == "bf16":  # a real backward that keeps its final values in bf16 only: the optimizer then reads that buffer
            ids = torch.randint(2, 502, (1, 1024), generator=torch.Generator().manual_seed(1))
            m(input_ids=ids, labels=ids)
            m.backward(final=2)
            torch.cuda.synchronize()
        for form in ("fused", "flat+transpose", "range"):
            eng.set_option("fuse_adamw_t", 1 if form == "fused" else 0)
            win = {"off": [], "on": []}
            for _ in range(a.rounds):
                for which in ("off", "on"):
                    eng.set_decay_mask(flags if which == "on" else None)
                    win[which].append(window("range" if form == "range" else "step"))
            eng.set_decay_mask(None)
            med = {k: statistics.median(v) for k, v in win.items()}
            rows.append(dict(grads=grads, form=form, off_us=med["off"], on_us=med["on"], off_min=min(win["off"]), off_max=max(win["off"]),
                             on_min=min(win["on"]), on_max=max(win["on"]), off_spread_pct=100 * (max(win["off"]) - min(win["off"])) / med["off"],
                             delta_pct=100 * (med["on"] - med["off"]) / med["off"], windows=win))
    eng.set_option("fuse_adamw_t", 1)
    lines = [f"n_params {n}, tensors {len(flags)}, no-decay tensors {flags.count(False)}, table ranges {n_ranges}, "
             f"{a.rounds} rounds x {a.iters} steps, device {torch.cuda.get_device_name(0)}", "",
             "| gradients | form | mask off us (min .. max) | mask on us (min .. max) | off spread % | on - off % |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grads']} | {r['form']} | {r['off_us']:.1f} ({r['off_min']:.1f} .. {r['off_max']:.1f}) | "
                     f"{r['on_us']:.1f} ({r['on_min']:.1f} .. {r['on_max']:.1f}) | {r['off_spread_pct']:.2f} | {r['delta_pct']:+.2f} |")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "decay_rule_bench.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "decay_rule_bench.json"), "w") as f:
        json.dump(dict(n_params=n, rounds=a.rounds, iters=a.iters, rows=rows), f, indent=1)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
