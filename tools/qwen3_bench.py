"""Measurements of the Qwen3 family (profiles/qwen3.md): one JSON line per section.

    python tools/qwen3_bench.py [--sections step,kernels,decode] [--layers 28] [--tokens 8192] [--ctx 1024] [--steps 10]
                                [--warmup 3] [--seed 0]

step     tokens/s of a full optimizer step of the Qwen3-0.6B-shaped body (hidden 1024, 16 / 8 heads of 128, SwiGLU 3072, tied,
         vocabulary 502) - forward, backward, clip 0.5 and AdamW on bf16 parameters with bf16 moments - through
         SLAMTrainer.optimizer_step, as tools/wide_bench.py times the 7B body: one packed micro-batch of --tokens tokens in
         sequences of --ctx, seeded synthetic tokens, random-init weights.
kernels  slam_op_qknorm_rope_fwd and slam_op_qknorm_bwd alone at M = --tokens, 16 / 8 heads of 128: device-event time per call
         over 200 calls, the bytes the algorithm moves, and the time those bytes take at the rates the project has measured
         for its RMSNorm kernels (4.80 TB/s forward, 5.21 TB/s backward: DESIGN.md section 4). The forward call builds its RoPE
         tables first (one more launch) and the backward call includes its two finish launches: the time of each kernel alone
         is read from a kernel trace of this section (rocprofv3 --kernel-trace --stats -- python tools/qwen3_bench.py
         --sections kernels).
decode   slam_decode_step time at B 8 behind a 64-token prefill, Qwen3 against the Qwen2 engine of the same dims (arch 0: a
         q|k|v bias instead of the two norm weights); the difference is the extra qknorm_rows_f32 launch per layer.
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
BASE = "Qwen/Qwen3-0.6B"
FWD_RATE, BWD_RATE = 4.80e12, 5.21e12  # bytes/s of rmsnorm_fwd / rmsnorm_bwd alone


def step_section(layers, tokens, ctx, steps, warmup, seed):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    dev = torch.device("cuda", torch.cuda.current_device())
    base = dict(KNOWN_BASE_CONFIGS[BASE], num_hidden_layers=layers, rope_theta=10000.0)
    model = UnitLM(UnitLMConfig(base_model_name=BASE, base_config=base, vocab_size=V, max_tokens=tokens), seed=seed)
    args = SLAMTrainingArguments(per_device_train_batch_size=1, gradient_accumulation_steps=1, learning_rate=1e-4,
                                 max_grad_norm=0.5, logging_steps=0, optim_state_dtype="bfloat16")
    trainer = SLAMTrainer(model=model, args=args)
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
    return {"section": "step", "model": BASE, "layers": layers, "tokens": nseq * ctx, "ctx": ctx, "vocab": V, "steps": steps,
            "params": model.engine.n_params, "tokens_per_s": round(nseq * ctx * steps / dt, 1),
            "ms_per_step": round(1e3 * dt / steps, 3), "ms_per_step_median": round(per[len(per) // 2], 3),
            "loss": round(float(trainer._loss_acc) / max(1, trainer._loss_n), 4),
            "workspace_bytes": model.engine.workspace_bytes(model._ws_tokens)}


def _time(fn, iters=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def kernels_section(M, seed):
    from slamkit_amd import engine as E
    lib = E.load_library()
    nH, nKV, hd = 16, 8, 128
    nQK, QKV = nH + nKV, (nH + 2 * nKV) * hd
    g = torch.Generator(device="cuda").manual_seed(seed)
    st = E.current_stream_ptr()
    p = lambda t: None if t is None else int(t.data_ptr())  # noqa: E731
    x0 = torch.randn(M, QKV, device="cuda", generator=g).to(torch.bfloat16)
    x = x0.clone()
    wq = (1 + 0.1 * torch.randn(hd, device="cuda", generator=g)).to(torch.bfloat16)
    wk = (1 + 0.1 * torch.randn(hd, device="cuda", generator=g)).to(torch.bfloat16)
    raw = torch.empty(M, nQK * hd, dtype=torch.bfloat16, device="cuda")
    rstd = torch.empty(M, nQK, dtype=torch.float32, device="cuda")
    tab = torch.empty(4 * M * (hd // 2), dtype=torch.float32, device="cuda")
    ctx = 1024

    def fwd(save=True):
        rc = lib.slam_op_qknorm_rope_fwd(p(x), p(wq), p(wk), None, 1e4, 1e-6, M, ctx, nH, nKV, hd, p(raw) if save else None,
                                         p(rstd) if save else None, p(tab), st)
        assert rc == 0, rc

    fwd_us = _time(fwd)
    fwd_nosave_us = _time(lambda: fwd(False))
    x.copy_(x0)
    fwd()
    dq = torch.randn(M, QKV, device="cuda", generator=g).to(torch.bfloat16)
    nws = lib.slam_op_qknorm_bwd_workspace(M, nH, nKV, hd)
    ws = torch.empty(nws // 4, dtype=torch.float32, device="cuda")
    dwq = torch.empty(hd, dtype=torch.float32, device="cuda")
    dwk = torch.empty(hd, dtype=torch.float32, device="cuda")

    def bwd():
        rc = lib.slam_op_qknorm_bwd(p(dq), p(raw), p(rstd), p(wq), p(wk), p(dwq), p(dwk), p(ws), M, nH, nKV, hd, st)
        assert rc == 0, rc

    bwd_us = _time(bwd)
    e = M * nQK * hd
    fwd_bytes = e * 2 * 3 + M * nQK * 4 + 2 * M * (hd // 2) * 4 * 2  # q|k read, written twice; rstd; cos / sin, plain + scaled
    bwd_bytes = e * 2 * 3 + M * nQK * 4                              # dy and raw read, dx written; rstd
    return {"section": "kernels", "M": M, "heads": [nH, nKV, hd],
            "table_plus_qknorm_rope_fwd_us": round(fwd_us, 2), "table_plus_qknorm_rope_fwd_nosave_us": round(fwd_nosave_us, 2),
            "fwd_bytes": fwd_bytes, "fwd_bound_us": round(fwd_bytes / FWD_RATE * 1e6, 2),
            "qknorm_bwd_us_with_finish": round(bwd_us, 2), "bwd_bytes": bwd_bytes, "bwd_bound_us": round(bwd_bytes / BWD_RATE * 1e6, 2),
            "bwd_blocks": lib.slam_op_qknorm_bwd_workspace(M, nH, nKV, hd) // (2 * hd * 4)}


def decode_section(layers, seed, B=8, prompt=64, steps=64):
    from slamkit_amd import engine as E
    from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS
    b = KNOWN_BASE_CONFIGS[BASE]
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"section": "decode", "layers": layers, "B": B, "prompt": prompt, "steps": steps}
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, V, (B, prompt), generator=g).to(dev)
    for name, arch in (("qwen2_same_dims", 0), ("qwen3", 3)):
        desc = E.SlamModelDesc(layers, b["hidden_size"], b["num_attention_heads"], b["num_key_value_heads"], b["head_dim"],
                               b["intermediate_size"], V, 0, 1e-6, 10000.0)
        eng = E.Engine(desc, arch=arch)
        params = (torch.randn(eng.n_params, generator=torch.Generator().manual_seed(seed + 1)) * 0.02).to(torch.bfloat16).to(dev)
        for tname, t in eng.tensors.items():
            if tname.endswith(("ln1", "ln2", "norm", "q_norm", "k_norm")):
                params[t.offset:t.offset + t.numel] = 1.0
        eng.bind_params(params, None)
        tokens = max(B * prompt, 2 * B)
        ws = torch.empty(eng.workspace_bytes(tokens) + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        eng.bind_workspace(ws[off:off + eng.workspace_bytes(tokens)], tokens)
        cap = 256
        kv = torch.empty(eng.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
        eng.bind_kv_cache(kv, B, cap)
        logits = torch.empty(B, V, dtype=torch.float32, device=dev)
        tok = torch.ones(B, dtype=torch.int64, device=dev)
        best = None
        for rep in range(3):
            lens = torch.full((B,), prompt, dtype=torch.int32, device=dev)
            eng.prefill(ids, lens, B, prompt, logits)
            for _ in range(8):
                eng.decode_step(tok, lens, B, logits)
            torch.cuda.synchronize()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                eng.decode_step(tok, lens, B, logits)
            z.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(z) * 1e3 / steps
            best = us if best is None else min(best, us)
        out[name + "_us_per_step"] = round(best, 1)
        assert bool(torch.isfinite(logits).all())
        eng.close()
    out["extra_us_per_layer"] = round((out["qwen3_us_per_step"] - out["qwen2_same_dims_us_per_step"]) / layers, 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="step,kernels,decode")
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    for s in a.sections.split(","):
        if s == "step":
            res = step_section(a.layers, a.tokens, a.ctx, a.steps, a.warmup, a.seed)
        elif s == "kernels":
            res = kernels_section(a.tokens, a.seed)
        elif s == "decode":
            res = decode_section(a.layers, a.seed)
        else:
            raise SystemExit(f"unknown section {s!r}")
        res["device"] = torch.cuda.get_device_name()
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
