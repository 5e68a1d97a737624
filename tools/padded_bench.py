"""Padding-free against padded execution of right-padded batches, on one GPU in one process: the same batches through the
same trainer with `padding_free` off and on, in alternating blocks of steps (device-synchronised host timing around every
block; 10 warm-up steps per mode before its first block).

    python tools/padded_bench.py [--steps 150] [--rounds 3] [--warmup 10] [--only train,dpo,ll] [--pad-side right|left|both]

  train  bench.py's `extras.padded` workload (bench.synth_padded_358m: seed 4321, [8, 1024] rows of lengths U{256..1024},
         Slam-358M, bf16 optimizer state) through SLAMTrainer.optimizer_step; one instrumented step per mode adds the
         per-family kernel times (engine option "time_families"; the dpo workload does the same for its policy engine).
  ll     UnitLM.log_likelihood on sWUGGY / sBLIMP-shaped batches: [32, 256] rows of lengths U{20..256}, the same model.
  dpo    bench.py's `--workload dpo` pairs (8 pairs = 16 sequences per step, prompt U{25..75}, completions U{50..150})
         through SLAMDPOTrainer.optimizer_step: policy forward + backward and the reference model's forward.

  span   (`--pad-side left` or `both`; replaces the three above) the `train` rows shifted to the left edge / the middle of their
         [8, 1024] batch and run as span batches (slam_forward_unpadded_spans, from the host mask), against the same rows
         right-padded under padding_free: the same launches apart from the pack and its start offsets.
  pack   (`--only pack`) the pack launch alone at 8 x 1024 and 300 x 7: slam_op_unpad_pack_spans with starts, with NULL, and
         slam_op_unpad_pack, alternating; with `--parent-lib PATH` also slam_op_unpad_pack of that build of the parent commit.

Prints one JSON line per workload - tokens/s (non-ignored labels) and ms/step of both modes from the summed blocks, the ratio
per round (its spread is the run-to-run spread), the fill (real tokens / positions) and the bound 1 / fill - then the same
as a markdown table.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises: see slamkit_amd/__init__.py

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload generators; bench.py itself is not run)

V = bench.V


def alternate(modes, steps, rounds, warmup):
    """modes: {name: step(i)}. Returns {name: [seconds of each timed block]}; blocks alternate pad, pf, pad, pf, ..."""
    out = {k: [] for k in modes}
    for r in range(rounds):
        for name, step in modes.items():
            if r == 0:
                for i in range(warmup):
                    step(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                step(i)
            torch.cuda.synchronize()
            out[name].append(time.perf_counter() - t0)
    return out


def summarise(name, secs, steps, tokens_per_step, positions_per_step, packed_per_step, what):
    pad, pf = secs["padded"], secs["padding_free"]
    ratios = [a / b for a, b in zip(pad, pf)]
    fill = tokens_per_step / positions_per_step
    row = lambda s: {"ms_per_step": round(1e3 * sum(s) / (steps * len(s)), 3),  # noqa: E731
                     "tokens_per_s": round(tokens_per_step * steps * len(s) / sum(s), 1)}
    pad_share = 1.0 - packed_per_step / positions_per_step  # positions the padding-free step does not execute
    saved = 1.0 - sum(pf) / sum(pad)
    return {"workload": name, "what": what, "steps_per_block": steps, "rounds": len(pad), "padded": row(pad), "padding_free": row(pf),
            "ratio": round(sum(pad) / sum(pf), 4), "ratio_per_round": [round(x, 4) for x in ratios],
            "ratio_spread": round(max(ratios) - min(ratios), 4), "fill": round(fill, 4), "bound_1_over_fill": round(1.0 / fill, 4),
            "positions_per_step": positions_per_step, "packed_tokens_per_step": packed_per_step,
            "pad_share_of_positions": round(pad_share, 4), "step_time_saved": round(saved, 4),
            "recovered_share_of_pads": round(saved / pad_share, 4) if pad_share > 0 else None}


def family_table(model, step):
    """{family: ms} of one instrumented step (the marks of its last forward + backward)."""
    model.engine.set_option("time_families", 1)
    step(0)
    torch.cuda.synchronize()
    fam = {}
    for nm, ms in model.engine.family_ms():
        fam[nm] = fam.get(nm, 0.0) + ms
    model.engine.set_option("time_families", 0)
    return {k: round(v, 3) for k, v in fam.items()}


def with_mode(model, on, fn):
    def step(i):
        model.padding_free = on
        fn(i, on)
    return step


def bench_train_and_ll(a, dev, res):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    B, T = bench.B, bench.T
    model = UnitLM(UnitLMConfig(base_model_name="Qwen/Qwen2.5-0.5B", rope_theta=10000.0, vocab_size=V, max_tokens=B * T), seed=0)
    args = SLAMTrainingArguments(per_device_train_batch_size=B, gradient_accumulation_steps=1, learning_rate=1e-3, max_grad_norm=0.5,
                                 logging_steps=0, optim_state_dtype="bfloat16")
    tr = SLAMTrainer(model=model, args=args)
    if "train" in a.only:
        made = [bench.synth_padded_358m(0, 400 + s, dev) for s in range(4)]
        # padded: exactly the dicts bench.py's `padded` line steps on. padding-free: the same device tensors plus the collated
        # mask ON THE HOST, which is where the trainer's collator leaves it and what gives the model its row lengths
        pad_mb = [[mb] for mb, _ in made]
        pf_mb = [[dict(mb, attention_mask=(torch.arange(T)[None] < torch.tensor(lens)[:, None]).long())] for mb, lens in made]
        counts = [float(sum(lens)) for _, lens in made]  # non-ignored labels: every real token (labels[:, 0] is never a target)
        packed = [-(-sum(lens) // 64) * 64 for _, lens in made]

        def fn(i, on):
            k = i % 4
            tr.optimizer_step((pf_mb if on else pad_mb)[k], 1e-3, counts=(counts[k],) * 2)
        modes = {"padded": with_mode(model, False, fn), "padding_free": with_mode(model, True, fn)}
        secs = alternate(modes, a.steps, a.rounds, a.warmup)
        # steps cycle through the 4 batches: per-step figures are their means (steps is a multiple of 4)
        r = summarise("train", secs, a.steps, sum(counts) / 4, B * T, sum(packed) / 4,
                      "Slam-358M optimizer step, right-padded [8, 1024] rows, lengths U{256..1024}, seed 4321 (bench.py extras.padded)")
        r["family_ms"] = {k: family_table(model, s) for k, s in modes.items()}
        res.append(r)
        print(json.dumps(r), flush=True)
    if "ll" in a.only:
        g = torch.Generator().manual_seed(4321)
        Bl, Tl = 32, 256
        batches, real = [], []
        for _ in range(4):
            ids = torch.zeros(Bl, Tl, dtype=torch.long)
            lens = torch.randint(20, Tl + 1, (Bl,), generator=g).tolist()
            for b, n in enumerate(lens):
                ids[b, :n] = torch.randint(2, V, (n,), generator=g)
            batches.append(ids.to(dev))
            real.append(lens)

        def fn(i, on):
            model.log_likelihood(batches[i % 4], True)
        modes = {"padded": with_mode(model, False, fn), "padding_free": with_mode(model, True, fn)}
        secs = alternate(modes, 2 * a.steps, a.rounds, a.warmup)
        res.append(summarise("log_likelihood", secs, 2 * a.steps, sum(sum(x) - len(x) for x in real) / 4, Bl * Tl,
                             sum(-(-sum(x) // 64) * 64 for x in real) / 4,
                             "UnitLM.log_likelihood(mean_nll=True), Slam-358M, [32, 256] rows of lengths U{20..256} on the device "
                             "(padding-free reads the lengths back once per call)"))
        print(json.dumps(res[-1]), flush=True)
    model.padding_free = False
    del tr, model
    torch.cuda.empty_cache()


def bench_span(a, dev, res):
    """The extras.padded rows at the other edge (or in the middle) of their batch, against themselves right-padded."""
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    B, T = bench.B, bench.T
    model = UnitLM(UnitLMConfig(base_model_name="Qwen/Qwen2.5-0.5B", rope_theta=10000.0, vocab_size=V, max_tokens=B * T), seed=0)
    args = SLAMTrainingArguments(per_device_train_batch_size=B, gradient_accumulation_steps=1, learning_rate=1e-3, max_grad_norm=0.5,
                                 logging_steps=0, optim_state_dtype="bfloat16")
    tr = SLAMTrainer(model=model, args=args)
    made = [bench.synth_padded_358m(0, 400 + s, dev) for s in range(4)]
    col = torch.arange(T)[None]
    right_mb, span_mb = [], []
    for mb, lens in made:
        ln = torch.tensor(lens)[:, None]
        st = (T - ln) if a.pad_side == "left" else (T - ln) // 2
        right_mb.append([dict(mb, attention_mask=(col < ln).long())])
        moved = {k: torch.stack([torch.roll(v[b], int(st[b])) for b in range(B)]) for k, v in mb.items()}
        span_mb.append([dict(moved, attention_mask=((col >= st) & (col < st + ln)).long())])
    counts = [float(sum(lens)) for _, lens in made]
    model.padding_free = True  # the right-padded rows run packed; the span rows run packed whatever that switch says
    model.span_masks = True    # host masks that are not right padding are honoured (off by default)

    def step_of(batches):
        return lambda i: tr.optimizer_step(batches[i % 4], 1e-3, counts=(counts[i % 4],) * 2)
    name = a.pad_side + "_span"
    secs = alternate({"right_padding_free": step_of(right_mb), name: step_of(span_mb)}, a.steps, a.rounds, a.warmup)
    row = lambda x: {"ms_per_step": round(1e3 * sum(x) / (a.steps * len(x)), 3),  # noqa: E731
                     "tokens_per_s": round(sum(counts) / 4 * a.steps * len(x) / sum(x), 1),
                     "ms_per_step_per_round": [round(1e3 * t / a.steps, 3) for t in x]}
    ratios = [r / s for r, s in zip(secs["right_padding_free"], secs[name])]
    r = {"workload": "span", "pad_side": a.pad_side, "steps_per_block": a.steps, "rounds": a.rounds,
         "what": f"Slam-358M optimizer step, [8, 1024] rows of lengths U{{256..1024}}, seed 4321 (bench.py extras.padded): "
                 f"padding on the {a.pad_side} side(s) as a span batch against right padding under padding_free",
         "right_padding_free": row(secs["right_padding_free"]), name: row(secs[name]),
         "ratio_right_over_span": round(sum(secs["right_padding_free"]) / sum(secs[name]), 4),
         "ratio_per_round": [round(x, 4) for x in ratios], "ratio_spread": round(max(ratios) - min(ratios), 4)}
    res.append(r)
    print(json.dumps(r), flush=True)
    model.padding_free = False
    del tr, model
    torch.cuda.empty_cache()


def bench_pack(a, dev, res):
    """Microseconds per pack launch, back to back on one stream between two events; the variants alternate, 3 rounds."""
    import ctypes as C
    from slamkit_amd import engine as E
    lib = E.load_library()
    doors = {"spans": (lib, True, "s"), "spans_null": (lib, True, None), "unpad_pack": (lib, False, None)}
    if a.parent_lib:
        old = C.CDLL(a.parent_lib)
        vp, i32 = C.c_void_p, C.c_int32
        old.slam_op_unpad_pack.restype = C.c_int
        old.slam_op_unpad_pack.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, C.c_size_t, vp]
        doors["parent_unpad_pack"] = (old, False, None)
    n = 2000
    for B, T in ((8, 1024), (300, 7)):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(1, V, (B, T), generator=g).to(dev)
        lens_h = torch.randint(1, T + 1, (B,), generator=g)
        lens = lens_h.to(torch.int32).to(dev)
        starts = (T - lens_h).to(torch.int32).to(dev)  # left padding
        Mp = -(-int(lens_h.sum()) // 64) * 64
        nbytes = E.unpadded_scratch_bytes(B, T)
        raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        o = (-raw.data_ptr()) % 256
        sp, st = raw.data_ptr() + o, E.current_stream_ptr()

        def launch(door):
            l, spans, s = doors[door]
            if spans:
                return l.slam_op_unpad_pack_spans(ids.data_ptr(), ids.data_ptr(), starts.data_ptr() if s else None, lens.data_ptr(),
                                                  B, T, Mp, 0, sp, nbytes, st)
            return l.slam_op_unpad_pack(ids.data_ptr(), ids.data_ptr(), lens.data_ptr(), B, T, Mp, 0, sp, nbytes, st)
        us = {k: [] for k in doors}
        for r in range(4):  # round 0 warms up
            for k in doors:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    assert launch(k) == 0
                e1.record()
                torch.cuda.synchronize()
                if r:
                    us[k].append(round(1e3 * e0.elapsed_time(e1) / n, 3))
        res.append({"workload": "pack", "B": B, "T": T, "M_packed": Mp, "launches_per_block": n, "us_per_launch_per_round": us})
        print(json.dumps(res[-1]), flush=True)


def bench_dpo(a, dev, res):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer
    cfg = dict(base_model_name="Qwen/Qwen2.5-0.5B", rope_theta=10000.0, vocab_size=V, max_tokens=16 * 256)
    model = UnitLM(UnitLMConfig(**cfg), seed=0)
    ref = UnitLM(UnitLMConfig(**cfg), seed=0, allocate_grads=False)

    class _Tok:  # rows below are already token ids
        bos_token_id = eos_token_id = 1

        def __call__(self, s, add_special_tokens=False):
            return {"input_ids": list(s)}
    g = torch.Generator().manual_seed(4321)

    def ids(lo, hi):
        return torch.randint(2, V, (int(torch.randint(lo, hi + 1, (1,), generator=g)),), generator=g).tolist()
    pairs = [[{"prompt": ids(25, 75), "chosen": ids(50, 150), "rejected": ids(50, 150)} for _ in range(8)] for _ in range(4)]
    args = DPOConfig(per_device_train_batch_size=8, learning_rate=5e-5, max_grad_norm=0.5, logging_steps=0, beta=0.1,
                     optim_state_dtype="bfloat16")
    tr = SLAMDPOTrainer(model=model, ref_model=ref, args=args, train_dataset=[r for b in pairs for r in b], processing_class=_Tok())
    batches = [tr._collate_pairs(tr.train_dataset[8 * i: 8 * i + 8]) for i in range(4)]

    def fn(i, on):
        ref.padding_free = on
        tr.optimizer_step([batches[i % 4]], 5e-5)
    modes = {"padded": with_mode(model, False, fn), "padding_free": with_mode(model, True, fn)}
    secs = alternate(modes, a.steps, a.rounds, a.warmup)
    r = summarise("dpo", secs, a.steps, sum(int((b["labels"] != -100).sum()) for b in batches) / 4,
                         sum(b["input_ids"].numel() for b in batches) / 4,
                         sum(-(-int(b["lengths"].sum()) // 64) * 64 for b in batches) / 4,
                         "DPO step on Slam-358M, 8 pairs = 16 right-padded sequences (bench.py --workload dpo): policy fwd + bwd, "
                         "reference fwd, clip + AdamW; tokens = completion tokens; fill = all real tokens / positions")
    r["family_ms"] = {k: family_table(model, s) for k, s in modes.items()}  # the policy engine's forward + backward
    res.append(r)
    print(json.dumps(r), flush=True)


def markdown(res):
    out = ["| workload | padded ms/step | padded tokens/s | padding-free ms/step | padding-free tokens/s | ratio | per round | fill | bound 1/fill | pads recovered |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        out.append(f"| {r['workload']} | {r['padded']['ms_per_step']} | {r['padded']['tokens_per_s']:.0f} | {r['padding_free']['ms_per_step']} | "
                   f"{r['padding_free']['tokens_per_s']:.0f} | {r['ratio']:.3f} | {' / '.join(f'{x:.3f}' for x in r['ratio_per_round'])} | "
                   f"{r['fill']:.3f} | {r['bound_1_over_fill']:.3f} | {100 * r['recovered_share_of_pads']:.0f} % |")
    for r in res:
        if "family_ms" in r:
            pad, pf = r["family_ms"]["padded"], r["family_ms"]["padding_free"]
            out += ["", f"Kernel families of one instrumented {r['workload']} step (ms, summed over the step's launches):", "",
                    "| family | padded | padding-free | ratio |", "|---|---|---|---|"]
            for k in sorted(pad, key=lambda k: -pad[k]):
                out.append(f"| {k} | {pad[k]:.3f} | {pf.get(k, 0.0):.3f} | {pad[k] / pf[k]:.2f} |" if pf.get(k) else f"| {k} | {pad[k]:.3f} | - | - |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150, help="timed steps per block (a multiple of 4: the batches cycle)")
    ap.add_argument("--rounds", type=int, default=3, help="blocks per mode")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="train,ll,dpo")
    ap.add_argument("--pad-side", choices=["right", "left", "both"], default="right",
                    help="left / both: the train rows as span batches against themselves right-padded under padding_free")
    ap.add_argument("--parent-lib", default=None, help="--only pack: a libslam_engine.so built from the parent commit")
    a = ap.parse_args()
    a.only = set(a.only.split(","))
    a.steps = max(4, a.steps // 4 * 4)
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    if "pack" in a.only:
        bench_pack(a, dev, res)
    elif a.pad_side != "right":
        bench_span(a, dev, res)
    else:
        if a.only & {"train", "ll"}:
            bench_train_and_ll(a, dev, res)
        if "dpo" in a.only:
            bench_dpo(a, dev, res)
    print(json.dumps({"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "device": torch.cuda.get_device_name(0),
                      "torch": torch.__version__, "hip": torch.version.hip}))
    if any("padded" in r for r in res):
        print(markdown(res))


if __name__ == "__main__":
    main()
