"""KV-cached generation benchmark (slam_prefill / slam_decode_step / UnitLM.generate) at the reference's evaluation setting:
B = 8, prompt 256, 150 new tokens (config/metric/generate.yaml), on a randomly initialised model.

Usage: python tools/decode_bench.py [--models slam,cfg3] [--steps 150] [--reps 2] [--no-reforward]
       python tools/decode_bench.py --trace-summary DIR   (per-launch table of the decode kernels from a
                                                            `rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_bench.py`)
Prints one JSON line per measurement:
  prefill_ms          one slam_prefill of the batch (median of 5, device events)
  step_ms             median of device-event-timed decode steps after 10 warm-up steps
  floor_ms / floor_share   weight bytes / 6.3 TB/s (every weight is read once per step) and floor / step
  generate_s, reforward_s, speedup   end-to-end greedy generate vs a re-forward loop built here from `forward` (one full
                      forward over the whole sequence per new token), alternated within this call
A second Slam-358M run at B = 96 (above the 64-row limit of the weight-streaming kernel: its bf16 projections take the tiled
GEMM) gives the decode step on the other side of the kernel selection.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 6.3e12
MODELS = {
    "slam": ("Qwen/Qwen2.5-0.5B", 502),
    "cfg3": ("Qwen/Qwen2.5-1.5B", 152576),
}


def ev_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def build(name, max_tokens):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base, vocab = MODELS[name]
    return UnitLM(UnitLMConfig(base_model_name=base, vocab_size=vocab, max_tokens=max_tokens), allocate_grads=False, seed=0)


def step_bench(m, B, P, steps, tag):
    import torch
    dev = m.device
    V = m.config.vocab_size
    g = torch.Generator(device=dev).manual_seed(0)
    ids = torch.randint(2, V, (B, P), device=dev, generator=g)
    lens = torch.full((B,), P, dtype=torch.int32, device=dev)
    cap = -(-(P + steps) // 64) * 64
    m._ensure_workspace(max(B * P, 2 * B))
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    pre = []
    for _ in range(5):
        lens.fill_(P)
        pre.append(ev_ms(lambda: m.engine.prefill(ids, lens, B, P, logits)))
    tok = torch.ones(B, dtype=torch.int64, device=dev)
    st = []
    for k in range(steps - 1):
        t = ev_ms(lambda: m.engine.decode_step(tok, lens, B, logits))
        if k >= 10:
            st.append(t)
    wbytes = 2 * m.engine.n_params
    step = statistics.median(st)
    floor = wbytes / HBM_BPS * 1e3
    r = dict(bench="decode", model=tag, B=B, prompt=P, prefill_ms=round(statistics.median(pre), 3), step_ms=round(step, 4),
             floor_ms=round(floor, 4), floor_share=round(floor / step, 3), weight_MB=round(wbytes / 1e6, 1), steps_timed=len(st))
    print(json.dumps(r), flush=True)
    return r


def e2e(m, B, P, new, reps, tag, reforward=True):
    import torch
    dev = m.device
    V = m.config.vocab_size
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, V, (B, P), device=dev, generator=g)

    def gen():
        return m.generate(input_ids=ids, max_new_tokens=new, eos_token_id=[])

    def loop():
        seq = ids
        for _ in range(new):
            nxt = m(input_ids=seq).logits[:, -1].float().argmax(-1)
            seq = torch.cat([seq, nxt[:, None]], 1)
        return seq

    m._ensure_workspace(B * (-(-(P + new) // 64) * 64))
    gen()  # warm-up (allocations, first launches)
    tg, tr = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen()
        torch.cuda.synchronize()
        tg.append(time.perf_counter() - t0)
        if reforward:
            t0 = time.perf_counter()
            loop()
            torch.cuda.synchronize()
            tr.append(time.perf_counter() - t0)
    r = dict(bench="generate_e2e", model=tag, B=B, prompt=P, new_tokens=new, generate_s=round(statistics.median(tg), 4))
    if tr:
        r.update(reforward_s=round(statistics.median(tr), 4), speedup=round(statistics.median(tr) / statistics.median(tg), 2))
    print(json.dumps(r), flush=True)


def trace_summary(d):
    """Per-launch table of the decode kernels from a rocprofv3 kernel trace (the SQLite database it writes, or
    *kernel_trace.csv files): (kernel, grid in blocks) -> launches, median duration."""
    import sqlite3
    rows = {}

    def add(name, gx, gy, gz, us):
        if not any(k in name for k in ("gemm_skinny", "skinny_reduce", "attn_decode", "rmsnorm_fwd", "swiglu_fwd")):
            return
        short = name.split("(")[0].replace("void ", "").replace("(anonymous namespace)::", "")
        rows.setdefault((short, gx, gy, gz), []).append(us)

    for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        c = sqlite3.connect(f)
        for n, gx, gy, gz, wx, us in c.execute("select name, grid_x, grid_y, grid_z, workgroup_x, duration / 1e3 from kernels"):
            add(n.replace("(anonymous namespace)::", ""), gx // max(wx, 1), gy, gz, us)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            add(r.get("Kernel_Name", ""), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]),
                int(r["Grid_Size_Z"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
        print(json.dumps(dict(kernel=k[0], grid=list(k[1:]), launches=len(v), median_us=round(statistics.median(v), 2),
                              total_ms=round(sum(v) / 1e3, 2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="slam,cfg3")
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-reforward", action="store_true")
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        trace_summary(a.trace_summary)
        return
    import torch
    assert torch.cuda.is_available()
    for name in a.models.split(","):
        m = build(name, 4096)
        step_bench(m, 8, 256, a.steps, name)
        if name == "slam":
            step_bench(m, 96, 64, min(a.steps, 60), name)
        e2e(m, 8, 256, a.steps, a.reps, name, reforward=(name == "slam" and not a.no_reforward))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
