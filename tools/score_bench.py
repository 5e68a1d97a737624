"""Scoring benchmark: UnitLM.score_continuations (one prefill, slam_kv_repeat, slam_extend_score) against the route it
replaces - sequence_logps over the [B n, T + T_c] concatenated batch - and the fused head + row statistics kernel
(slam_op_score_rows) against the tiled bf16 head GEMM of the same shape, on randomly initialised models.

Usage: python tools/score_bench.py [--models slam,cfg3] [--reps 5] [--score-chunk 128]
       python tools/score_bench.py --kernel [--reps 7]
Prints one JSON line per measurement. The compared runs alternate rep by rep in this process behind a warm-up of each; times
are medians, with every repetition listed beside them.
  end to end (B = 8 prompts of 256 tokens, n = 8 continuations of 128 tokens each): one line per way, `way` =
      "score_continuations" | "sequence_logps", with `seconds`, `seconds_all`, `workspace_tokens` / `workspace_MB` (host
      arithmetic of slam_workspace_bytes for what the way binds) and, on the first, `speedup` and `sum_abs_diff_max` (the
      largest difference between the two ways' per-row sums).
  --kernel (M, V, K) = (8192, 502, 896) and (4096, 152167, 1536): `score_ms` = one slam_op_score_rows (both launches),
      `gemm_nt_ms` = slam_op_gemm_nt writing bf16 [M, V padded to 256], device events, with the achieved TFLOP/s of each
      (2 M V K flop) and `rate_share` = the score kernel's rate over gemm_nt's."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def end_to_end(tag, B, n, P, Tc, reps, score_chunk):
    import torch
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base, vocab = MODELS[tag]
    m = UnitLM(UnitLMConfig(base_model_name=base, vocab_size=vocab, max_tokens=max(P + Tc, 2048)), allocate_grads=False, seed=0)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, vocab, (B, P), device=dev, generator=g)
    cont = torch.randint(2, vocab, (B * n, Tc), device=dev, generator=g)
    full = torch.cat([ids.repeat_interleave(n, 0), cont], 1)
    lab = torch.full_like(full, -100)
    lab[:, P:] = cont
    C = Tc if score_chunk is None else min(score_chunk, Tc)
    ws_tokens = {"score_continuations": max(B * P, B * n * C, 2 * B * n), "sequence_logps": B * n * (P + Tc)}

    def new():
        return m.score_continuations(ids, continuations=cont, num_per_prompt=n, score_chunk=score_chunk).sum(1)

    def old():
        return m.sequence_logps(full, lab, padding_free=False)[0]

    ways = {"score_continuations": new, "sequence_logps": old}
    res = {}
    for k, f in ways.items():  # warm-up: workspace growth, kernel selection
        res[k] = wall(f)[1].double().cpu()
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, f in ways.items():
            times[k].append(wall(f)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in ways:
        r = dict(bench="score_e2e", model=tag, B=B, n=n, prompt=P, continuation=Tc, score_chunk=score_chunk, way=k,
                 seconds=round(med[k], 5), seconds_all=[round(t, 5) for t in times[k]], workspace_tokens=ws_tokens[k],
                 workspace_MB=round(m.engine.workspace_bytes(ws_tokens[k]) / 1e6, 1))
        if k == "score_continuations":
            r["speedup"] = round(med["sequence_logps"] / med[k], 3)
            r["sum_abs_diff_max"] = round(float((res["score_continuations"] - res["sequence_logps"]).abs().max()), 4)
        print(json.dumps(r), flush=True)


def kernel(M, V, K, reps):
    import torch
    from slamkit_amd import engine as E
    lib = E.load_library()
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    VP = -(-V // 256) * 256
    W = (torch.randn(VP, K, device="cuda", generator=g) * 0.03).to(torch.bfloat16)
    t = torch.randint(0, V, (M,), device="cuda", generator=g)
    lp = torch.empty(M, dtype=torch.float32, device="cuda")
    am = torch.empty(M, dtype=torch.int64, device="cuda")
    ws = torch.empty(E.score_rows_workspace_bytes(M, V), dtype=torch.uint8, device="cuda")
    Y = torch.empty(M, VP, dtype=torch.bfloat16, device="cuda")
    st = E.current_stream_ptr()

    def score():
        E.score_rows(X, W[:V], t, lp, am, None, ws)

    def gemm():
        rc = lib.slam_op_gemm_nt(X.data_ptr(), W.data_ptr(), Y.data_ptr(), None, None, M, VP, K, 1, st)
        assert rc == 0, rc

    ways = {"score": score, "gemm_nt": gemm}
    for f in ways.values():
        f()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, f in ways.items():
            times[k].append(ev_ms(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    flop = 2.0 * M * V * K
    print(json.dumps(dict(bench="score_kernel", M=M, V=V, K=K, score_ms=round(med["score"], 4), gemm_nt_ms=round(med["gemm_nt"], 4),
                          score_ms_all=[round(x, 4) for x in times["score"]], gemm_nt_ms_all=[round(x, 4) for x in times["gemm_nt"]],
                          score_tflops=round(flop / med["score"] / 1e9, 1), gemm_nt_tflops=round(flop / med["gemm_nt"] / 1e9, 1),
                          rate_share=round(med["gemm_nt"] / med["score"], 3), partial_MB=round(ws.numel() / 1e6, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="slam,cfg3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--score-chunk", type=int, default=None)
    ap.add_argument("--kernel", action="store_true")
    a = ap.parse_args()
    if a.kernel:
        kernel(8192, 502, 896, a.reps)
        kernel(4096, 152167, 1536, a.reps)
        return
    for tag in a.models.split(","):
        end_to_end(tag, 8, 8, 256, 128, a.reps, a.score_chunk)


if __name__ == "__main__":
    main()
