"""KV-cached generation benchmark (slam_prefill / slam_decode_step / UnitLM.generate) at the reference's evaluation setting:
B = 8, prompt 256, 150 new tokens (config/metric/generate.yaml), on a randomly initialised model.

Usage: python tools/decode_bench.py [--models slam,cfg3] [--steps 150] [--reps 2] [--no-reforward]
       python tools/decode_bench.py --cfg --models slam,cfg3,7b [--batches 1,8,32] [--blocks 3]
       python tools/decode_bench.py --num-return-sequences 8 [--models slam,cfg3] [--reps 3]
       python tools/decode_bench.py --prefill-chunk 512 [--models slam,cfg3]
       python tools/decode_bench.py --decode-weights fp8 --include-head --models slam,cfg3,7b
       python tools/decode_bench.py --trace-summary DIR   (per-launch table of the decode kernels from a
                                                            `rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_bench.py`)
Prints one JSON line per measurement:
  prefill_ms          one slam_prefill of the batch (median of 5, device events)
  step_ms             median of device-event-timed decode steps after 10 warm-up steps
  floor_ms / floor_share   weight bytes / 6.3 TB/s (every weight is read once per step) and floor / step
  generate_s, reforward_s, speedup   end-to-end greedy generate vs a re-forward loop built here from `forward` (one full
                      forward over the whole sequence per new token), alternated within this call
With --sampler torch,engine (and --do-sample: temperature 0.8, top_k 25, the reference's evaluation setting) only the end-to-end
generate is measured, once per sampler and rep, alternating the samplers within this call: one line per sampler with
`sampler`, `do_sample`, `generate_s` (median) and `generate_s_all`. --sample-op times the token choice alone at (B, V) =
(8, 502), (8, 152167), (64, 152167), (1, 152167): `engine_us` = one slam_sample_tokens, `torch_us` = the torch sampler's
per-step ops (bad words, warp, softmax, multinomial, pad, EOS bookkeeping), device events around 200 back-to-back calls.
With --num-return-sequences n: end-to-end sampled generate (sampler="engine") of B prompts x n continuations from ONE prefill
(`way` = "one_prefill": slam_prefill of B rows, slam_kv_repeat, B n rows decoded) against the same call on the prompts repeated
n times (`way` = "repeated_batch"), alternated rep by rep in this process: one line per way with `generate_s` (median),
`generate_s_all`, `workspace_tokens` / `workspace_MB` (what generate binds: max(B T, 2 B n) against B n T tokens; host
arithmetic of slam_workspace_bytes) and `peak_alloc_MB` (torch's peak over the way's first call, weights and cache included).
Then `kv_repeat_ms` (the fan-out alone behind a prefill, device events, median of 5) and one `logprob_op` line per
(B n, V) = (64, 502), (64, 152167): `logprobs_us` = one slam_token_logprobs, device events around 200 back-to-back calls.
With --prefill-chunk C: the prefill of B = 8 x T = 2048 prompts in one slam_prefill (`way` = "one_shot") against slam_prefill
over the first C columns + slam_extend over every further block of C (`way` = "chunked"), alternated rep by rep in this
process after a warm-up of each way, device events, median of 5: one line per way with `prefill_ms`, `prefill_ms_all`,
`workspace_tokens` / `workspace_MB` (what generate binds for that way with n = 1: host arithmetic of slam_workspace_bytes),
and on the chunked line `ratio` = chunked / one-shot and `logits_rel_rms` (the chunked last-token logits against the one-shot
ones). --trace-summary also lists the attn_extend / kv_extend_scatter / attn_fwd launches, for the kernel's share from a
`rocprofv3 --kernel-trace --stats` run of their own.
--constrain-op times slam_constrain_scores alone at (B, V) = (8, 502), (8, 152167), (64, 152167): a history of 256 prompt + 150
new tokens per row, no_repeat_ngram 3, device events around 200 back-to-back calls, five rounds alternating `inplace_us`
(scores is logits: only the bans are written) and `copy_us` (scores in a buffer of its own), with `copy_floor_us` =
2 B V 4 bytes / 6.3 TB/s. With --sampler S --no-repeat-ngram n: end-to-end greedy generate with sampler S, without and with
no_repeat_ngram_size = n, alternated rep by rep: one line per setting with `no_repeat_ngram_size`, `generate_s`, `generate_s_all`.
--sample-op --warp times slam_sample_tokens_warped beside slam_sample_tokens at (B, V) = (8, 502), (8, 152167), (64, 152167)
and top_k 25 and 256: `plain_us`, `warped_all_us` (min_p 0.05, typical_p 0.95, epsilon 1e-3, eta 2e-3) and `warped_typical_us`
(typical_p 0.9 alone), device events around 200 back-to-back calls, five alternating rounds, median and [min, max]. With
--sampler engine --warp: end-to-end sampled generate (temperature 0.8, top_k 25) without (`way` = "plain") and with those four
warpers (`way` = "warped"), alternated rep by rep.
--decode-weights fp8 [--include-head] [--models slam,cfg3,7b] [--batches 1,8,64] [--blocks 3]: the decode step from bf16
weights (codes dropped) and from FP8 codes (UnitLM.quantize_decode_weights), in alternating blocks within this process, prompt
256, device events, 10 warm-up steps per block: one `decode_w8` line per (model, B) with `bf16_step_ms` / `fp8_step_ms` (median
over the blocks, `_all` the blocks), `bf16_over_fp8` (median of the per-block ratios, `_minmax`), the bytes a step streams
(`bf16_MB`, `fp8_MB`) and their 6.3 TB/s floors, and `w8_launches_per_step`. --decode-weights bf16 runs the bf16 blocks alone
through calls every earlier revision has: the same file, copied into a parent checkout, measures it for an A-B-A comparison.
`7b` is the Qwen2.5-7B body with the unit vocabulary.
--cfg [--models slam,cfg3,7b] [--batches 1,8,32] [--blocks 3]: the guided decode step of classifier-free guidance - one
slam_cfg_scores over the 2 B logits rows, one slam_cfg_mirror_tokens, one slam_decode_step over 2 B rows - against the plain
step at B (slam_decode_step alone: launches this option does not touch), as plain - guided - plain blocks within this process,
prompt 256, device events per step, 10 warm-up steps per block: one `cfg_step` line per (model, B, neg_len) with
`plain_step_ms` (median over all plain blocks, `_all` the blocks), `guided_step_ms` and `guided_over_plain` (median of the
per-block ratios against the mean of the two plain blocks around it, `_minmax`). neg_len is the length of the unconditional
rows' prompts: 1 (generate's default, the last prompt token) and 256 (a negative prompt as long as the prompt). Then one
`cfg_op` line per (B, V) in {8, 32} x {502, 152576}: `cfg_scores_us` = one slam_cfg_scores (device events around 200
back-to-back calls, five rounds), `bytes_MB` = what it moves (2 B rows read, B written; rows above one chunk are read twice) and
`GBps`, `floor_us` = bytes / 6.3 TB/s; and `mirror_us` = one slam_cfg_mirror_tokens.
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
    "7b": ("Qwen/Qwen2.5-7B", 502),  # the SIMS-7B body with the unit vocabulary, as in tools/spec_bench.py
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


def w8_bench(name, batches, P, steps, blocks, fp8, include_head):
    """The decode step from bf16 weights (codes dropped) and from FP8 codes (UnitLM.quantize_decode_weights), in alternating
    blocks within this process. With fp8 false only the bf16 blocks run, through calls every earlier revision has - the same
    file measures a parent checkout for the A-B-A comparison."""
    import torch
    m = build(name, 4096)
    info = None
    if fp8:  # quantise once up front: every block then runs the same model
        info = m.quantize_decode_weights(include_head=include_head)
        m.drop_decode_weights()
    for B in batches:
        t = {"bf16": [], "fp8": []}
        last = {}
        for _ in range(blocks):
            last["bf16"] = step_bench(m, B, P, steps, name, quiet=True)
            t["bf16"].append(last["bf16"]["step_ms"])
            if fp8:
                m.quantize_decode_weights(include_head=include_head)
                n0 = m.engine.decode_w8_launches()
                last["fp8"] = step_bench(m, B, P, steps, name, quiet=True, saved=info["bf16_bytes"] - info["fp8_bytes"])
                last["fp8"]["w8_launches_per_step"] = (m.engine.decode_w8_launches() - n0) / (steps - 1)
                t["fp8"].append(last["fp8"]["step_ms"])
                m.drop_decode_weights()
        r = dict(bench="decode_w8", model=name, B=B, prompt=P, steps_timed=last["bf16"]["steps_timed"], blocks=blocks,
                 bf16_step_ms=round(statistics.median(t["bf16"]), 4), bf16_step_ms_all=t["bf16"],
                 bf16_MB=last["bf16"]["weight_MB"], bf16_floor_ms=last["bf16"]["floor_ms"])
        if fp8:
            ratios = [b / f for b, f in zip(t["bf16"], t["fp8"])]
            r.update(fp8_step_ms=round(statistics.median(t["fp8"]), 4), fp8_step_ms_all=t["fp8"], fp8_MB=last["fp8"]["weight_MB"],
                     fp8_floor_ms=last["fp8"]["floor_ms"], include_head=bool(include_head),
                     w8_launches_per_step=last["fp8"]["w8_launches_per_step"],
                     bf16_over_fp8=round(statistics.median(ratios), 3),
                     bf16_over_fp8_minmax=[round(min(ratios), 3), round(max(ratios), 3)])
        print(json.dumps(r), flush=True)
    del m
    torch.cuda.empty_cache()


def cfg_step_bench(name, batches, P, steps, blocks, scale=1.5):
    """The guided step (slam_cfg_scores + slam_cfg_mirror_tokens + slam_decode_step over 2 B rows) between two plain steps at B."""
    import torch
    from slamkit_amd import engine as E
    m = build(name, 4096)
    dev = m.device
    V = m.config.vocab_size
    cap = -(-(P + steps) // 64) * 64  # every block prefills again

    def block(rows, lens0, guided):
        g = torch.Generator(device=dev).manual_seed(0)
        ids = torch.randint(2, V, (rows, P), device=dev, generator=g)
        lens = lens0.clone()
        logits = torch.empty(rows, V, dtype=torch.float32, device=dev)
        m.engine.prefill(ids, lens, rows, P, logits)
        tok = torch.ones(rows, dtype=torch.int64, device=dev)
        if guided:
            scores = torch.empty(rows // 2, V, dtype=torch.float32, device=dev)
            ws = torch.empty(E.cfg_workspace_bytes(rows // 2, V), dtype=torch.uint8, device=dev)

        def step():
            if guided:
                E.cfg_scores(logits, scale, scores, ws)
                E.cfg_mirror_tokens(tok)
            m.engine.decode_step(tok, lens, rows, logits)

        st = [ev_ms(step) for _ in range(steps)]
        return statistics.median(st[10:])

    for B in batches:
        m._ensure_workspace(max(2 * B * P, 4 * B))
        cache = torch.empty(m.engine.kv_cache_bytes(2 * B, cap), dtype=torch.uint8, device=dev)
        m.engine.bind_kv_cache(cache, 2 * B, cap)
        full = torch.full((B,), P, dtype=torch.int32, device=dev)
        for neg_len in (1, P):
            both = torch.cat([full, torch.full((B,), neg_len, dtype=torch.int32, device=dev)])
            plain, guided, ratios = [block(B, full, False)], [], []
            for _ in range(blocks):
                guided.append(block(2 * B, both, True))
                plain.append(block(B, full, False))
                ratios.append(guided[-1] / (0.5 * (plain[-2] + plain[-1])))
            print(json.dumps(dict(bench="cfg_step", model=name, B=B, prompt=P, neg_len=neg_len, steps_timed=steps - 10, blocks=blocks,
                                  plain_step_ms=round(statistics.median(plain), 4), plain_step_ms_all=[round(t, 4) for t in plain],
                                  guided_step_ms=round(statistics.median(guided), 4),
                                  guided_step_ms_all=[round(t, 4) for t in guided],
                                  guided_over_plain=round(statistics.median(ratios), 3),
                                  guided_over_plain_minmax=[round(min(ratios), 3), round(max(ratios), 3)])), flush=True)
        del cache
    del m
    torch.cuda.empty_cache()


def cfg_op_bench(calls=200, rounds=5):
    """Device-event time of slam_cfg_scores and of slam_cfg_mirror_tokens alone."""
    import torch
    from slamkit_amd import engine as E
    dev = torch.device("cuda")
    for B, V in ((8, 502), (32, 502), (8, 152576), (32, 152576)):
        g = torch.Generator(device=dev).manual_seed(V + B)
        logits = torch.randn(2 * B, V, device=dev, generator=g) * 3.0
        scores = torch.empty(B, V, dtype=torch.float32, device=dev)
        ws = torch.empty(E.cfg_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
        nxt = torch.ones(2 * B, dtype=torch.int64, device=dev)

        def run_scores():
            for _ in range(calls):
                E.cfg_scores(logits, 1.5, scores, ws)

        def run_mirror():
            for _ in range(calls):
                E.cfg_mirror_tokens(nxt)

        run_scores()
        run_mirror()
        torch.cuda.synchronize()
        ts, tm = [], []
        for _ in range(rounds):  # alternated
            ts.append(ev_ms(run_scores) / calls * 1e3)
            tm.append(ev_ms(run_mirror) / calls * 1e3)
        nbytes = (3 if V <= 2048 else 5) * B * V * 4  # rows above one chunk: the statistics' launch reads both rows first
        us = statistics.median(ts)
        print(json.dumps(dict(bench="cfg_op", B=B, vocab=V, cfg_scores_us=round(us, 2),
                              cfg_scores_us_minmax=[round(min(ts), 2), round(max(ts), 2)], bytes_MB=round(nbytes / 1e6, 3),
                              GBps=round(nbytes / us / 1e3, 1), floor_us=round(nbytes / HBM_BPS * 1e6, 3),
                              mirror_us=round(statistics.median(tm), 2))), flush=True)


def step_bench(m, B, P, steps, tag, quiet=False, saved=0):
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
    wbytes = 2 * m.engine.n_params - saved  # saved: what the FP8 codes take off the stream
    step = statistics.median(st)
    floor = wbytes / HBM_BPS * 1e3
    r = dict(bench="decode", model=tag, B=B, prompt=P, prefill_ms=round(statistics.median(pre), 3), step_ms=round(step, 4),
             floor_ms=round(floor, 4), floor_share=round(floor / step, 3), weight_MB=round(wbytes / 1e6, 1), steps_timed=len(st))
    if not quiet:
        print(json.dumps(r), flush=True)
    return r


def e2e_samplers(m, B, P, new, reps, tag, samplers, do_sample):
    """generate_s of each sampler, alternated rep by rep."""
    import torch
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, m.config.vocab_size, (B, P), device=dev, generator=g)
    kw = dict(input_ids=ids, max_new_tokens=new, eos_token_id=[])
    if do_sample:
        kw.update(do_sample=True, temperature=0.8, top_k=25, seed=11)
    m._ensure_workspace(B * (-(-(P + new) // 64) * 64))
    times = {s: [] for s in samplers}
    for s in samplers:
        m.generate(sampler=s, **kw)  # warm-up
    for _ in range(reps):
        for s in samplers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(sampler=s, **kw)
            torch.cuda.synchronize()
            times[s].append(time.perf_counter() - t0)
    for s in samplers:
        print(json.dumps(dict(bench="generate_e2e", model=tag, B=B, prompt=P, new_tokens=new, sampler=s, do_sample=bool(do_sample),
                              generate_s=round(statistics.median(times[s]), 4),
                              generate_s_all=[round(t, 4) for t in times[s]])), flush=True)


def e2e_no_repeat(m, B, P, new, reps, tag, sampler, n):
    """generate_s without and with no_repeat_ngram_size = n, alternated rep by rep."""
    import torch
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, m.config.vocab_size, (B, P), device=dev, generator=g)
    kw = dict(input_ids=ids, max_new_tokens=new, eos_token_id=[], sampler=sampler)
    m._ensure_workspace(B * (-(-(P + new) // 64) * 64))
    times = {k: [] for k in (0, n)}
    for k in times:
        m.generate(no_repeat_ngram_size=k, **kw)  # warm-up
    for _ in range(reps):
        for k in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(no_repeat_ngram_size=k, **kw)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    for k in times:
        print(json.dumps(dict(bench="generate_e2e", model=tag, B=B, prompt=P, new_tokens=new, sampler=sampler, no_repeat_ngram_size=k,
                              generate_s=round(statistics.median(times[k]), 4),
                              generate_s_all=[round(t, 4) for t in times[k]])), flush=True)


def constrain_op_bench(calls=200, rounds=5, prompt=256, new_tokens=150, n=3):
    """Device-event time of slam_constrain_scores alone, in place and into a buffer of its own."""
    import torch
    from slamkit_amd import engine as E
    dev = torch.device("cuda")
    for B, V in ((8, 502), (8, 152167), (64, 152167)):
        g = torch.Generator(device=dev).manual_seed(V + B)
        logits = torch.randn(B, V, device=dev, generator=g) * 3.0
        scores = torch.empty_like(logits)
        ids = torch.randint(2, V, (B, prompt), device=dev, generator=g)
        plen = torch.full((B,), prompt, dtype=torch.int32, device=dev)
        new = torch.randint(2, V, (B, new_tokens), device=dev, generator=g)
        done = torch.zeros(B, dtype=torch.uint8, device=dev)
        desc = E.SlamConstrainDesc(step=new_tokens, no_repeat_ngram=n, n_per_prompt=1, prompt_stride=0, ban_eos=0, n_eos=0,
                                   n_begin=0, n_seqs=0, n_seq_tokens=0)

        def run(out):
            for _ in range(calls):
                E.constrain_scores(logits, out, desc, ids, plen, new, done)

        for out in (logits, scores):
            run(out)
        torch.cuda.synchronize()
        ti, tc = [], []
        for _ in range(rounds):  # alternated
            ti.append(ev_ms(lambda: run(logits)) / calls * 1e3)
            tc.append(ev_ms(lambda: run(scores)) / calls * 1e3)
        print(json.dumps(dict(bench="constrain_op", B=B, vocab=V, history=prompt + new_tokens, no_repeat_ngram=n,
                              inplace_us=round(statistics.median(ti), 2), inplace_us_minmax=[round(min(ti), 2), round(max(ti), 2)],
                              copy_us=round(statistics.median(tc), 2), copy_us_minmax=[round(min(tc), 2), round(max(tc), 2)],
                              copy_floor_us=round(2 * B * V * 4 / HBM_BPS * 1e6, 2))), flush=True)


def sample_op_bench(calls=200, rounds=5):
    """Device-event time of the token choice alone: slam_sample_tokens against the torch sampler's per-step ops."""
    import torch
    from slamkit_amd import engine as E
    from slamkit_amd.model.unit_lm import _warp
    dev = torch.device("cuda")
    for B, V in ((8, 502), (8, 152167), (64, 152167), (1, 152167)):
        g = torch.Generator(device=dev).manual_seed(V + B)
        logits = torch.randn(B, V, device=dev, generator=g) * 3.0
        bad = torch.tensor([3, 4, 5], dtype=torch.long, device=dev)
        banned = torch.zeros(V, dtype=torch.uint8, device=dev)
        banned[bad] = 1
        eos_t = torch.tensor([1], dtype=torch.long, device=dev)
        eos_i = eos_t.to(torch.int32)
        new = torch.empty(B, calls, dtype=torch.int64, device=dev)
        nxt = torch.empty(B, dtype=torch.int64, device=dev)
        res = dict(bench="sample_op", B=B, vocab=V)
        for do_sample in (0, 1):
            desc = E.SlamSampleDesc(do_sample=do_sample, top_k=25, temperature=0.8, top_p=1.0, seed=11, step=0, pad_id=0, n_eos=1)
            ws = torch.empty(E.sample_workspace_bytes(B, V, 25), dtype=torch.uint8, device=dev)
            gen = torch.Generator(device=dev).manual_seed(11)

            def engine_calls():
                done = torch.zeros(B, dtype=torch.uint8, device=dev)
                for k in range(calls):
                    desc.step = k
                    E.sample_tokens(logits, desc, nxt, ws, banned, None, eos_i, done, new)

            def torch_calls():
                done = torch.zeros(B, dtype=torch.bool, device=dev)
                for k in range(calls):
                    scores = logits.index_fill(1, bad, float("-inf"))
                    if do_sample:
                        scores = _warp(scores, 0.8, 25, 1.0)
                        t = torch.multinomial(torch.softmax(scores, -1), 1, generator=gen)[:, 0]
                    else:
                        t = scores.argmax(-1)
                    t = torch.where(done, torch.full_like(t, 0), t)
                    new[:, k] = t
                    done |= torch.isin(t, eos_t)

            for name, fn in (("engine", engine_calls), ("torch", torch_calls)):
                fn()
                torch.cuda.synchronize()
            te, tt = [], []
            for _ in range(rounds):  # alternated
                te.append(ev_ms(engine_calls) / calls * 1e3)
                tt.append(ev_ms(torch_calls) / calls * 1e3)
            tag = "sample" if do_sample else "greedy"
            res[f"{tag}_engine_us"] = round(statistics.median(te), 2)
            res[f"{tag}_torch_us"] = round(statistics.median(tt), 2)
            res[f"{tag}_engine_us_minmax"] = [round(min(te), 2), round(max(te), 2)]
            res[f"{tag}_torch_us_minmax"] = [round(min(tt), 2), round(max(tt), 2)]
        print(json.dumps(res), flush=True)


WARP_ALL = dict(min_p=0.05, typical_p=0.95, epsilon_cutoff=1e-3, eta_cutoff=2e-3)


def warp_op_bench(calls=200, rounds=5):
    """Device-event time of slam_sample_tokens_warped (all four warpers on, and typical_p alone) beside slam_sample_tokens."""
    import torch
    from slamkit_amd import engine as E
    dev = torch.device("cuda")
    for B, V in ((8, 502), (8, 152167), (64, 152167)):
        g = torch.Generator(device=dev).manual_seed(V + B)
        logits = torch.randn(B, V, device=dev, generator=g) * 3.0
        banned = torch.zeros(V, dtype=torch.uint8, device=dev)
        banned[torch.tensor([3, 4, 5], device=dev)] = 1
        eos_i = torch.tensor([1], dtype=torch.int32, device=dev)
        new = torch.empty(B, calls, dtype=torch.int64, device=dev)
        nxt = torch.empty(B, dtype=torch.int64, device=dev)
        for top_k in (25, 256):
            desc = E.SlamSampleDesc(do_sample=1, top_k=top_k, temperature=0.8, top_p=1.0, seed=11, step=0, pad_id=0, n_eos=1)
            ws = torch.empty(E.sample_workspace_bytes(B, V, top_k), dtype=torch.uint8, device=dev)

            def run(warp):
                def fn():
                    done = torch.zeros(B, dtype=torch.uint8, device=dev)
                    for k in range(calls):
                        desc.step = k
                        if warp is None:
                            E.sample_tokens(logits, desc, nxt, ws, banned, None, eos_i, done, new)
                        else:
                            E.sample_tokens_warped(logits, desc, nxt, ws, warp, None, 1, None, banned, None, eos_i, done, new)
                return fn

            ways = {"plain": run(None), "warped_all": run(E.SlamWarpDesc(**WARP_ALL)),
                    "warped_typical": run(E.SlamWarpDesc(typical_p=0.9))}
            for fn in ways.values():
                fn()
            torch.cuda.synchronize()
            t = {w: [] for w in ways}
            for _ in range(rounds):  # alternated
                for w, fn in ways.items():
                    t[w].append(ev_ms(fn) / calls * 1e3)
            res = dict(bench="warp_op", B=B, vocab=V, top_k=top_k)
            for w in ways:
                res[f"{w}_us"] = round(statistics.median(t[w]), 2)
                res[f"{w}_us_minmax"] = [round(min(t[w]), 2), round(max(t[w]), 2)]
            print(json.dumps(res), flush=True)


def e2e_warp(m, B, P, new, reps, tag):
    """generate_s of the engine sampler (temperature 0.8, top_k 25) without and with the four warpers, alternated rep by rep."""
    import torch
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, m.config.vocab_size, (B, P), device=dev, generator=g)
    kw = dict(input_ids=ids, max_new_tokens=new, eos_token_id=[], do_sample=True, temperature=0.8, top_k=25, seed=11,
              sampler="engine")
    m._ensure_workspace(B * (-(-(P + new) // 64) * 64))
    ways = {"plain": {}, "warped": WARP_ALL}
    times = {w: [] for w in ways}
    for extra in ways.values():
        m.generate(**kw, **extra)  # warm-up
    for _ in range(reps):
        for w, extra in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(**kw, **extra)
            torch.cuda.synchronize()
            times[w].append(time.perf_counter() - t0)
    for w in ways:
        print(json.dumps(dict(bench="generate_e2e_warp", model=tag, B=B, prompt=P, new_tokens=new, way=w,
                              generate_s=round(statistics.median(times[w]), 4),
                              generate_s_all=[round(t, 4) for t in times[w]])), flush=True)


def nbest_bench(name, B, P, new, reps, n):
    """n continuations per prompt from one prefill against the repeated batch; kv_repeat alone."""
    import torch
    m = build(name, -(-(P + new) // 64) * 64)  # the workspace starts small: each way binds what it needs
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, m.config.vocab_size, (B, P), device=dev, generator=g)
    rep_ids = ids.repeat_interleave(n, 0)
    kw = dict(max_new_tokens=new, eos_token_id=[], do_sample=True, temperature=0.8, top_k=25, seed=11, sampler="engine")
    ways = {"one_prefill": lambda: m.generate(input_ids=ids, num_return_sequences=n, **kw),
            "repeated_batch": lambda: m.generate(input_ids=rep_ids, **kw)}
    info, outs = {}, {}
    for w, fn in ways.items():  # warm-up; one_prefill first: the workspace only grows
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        outs[w] = fn()
        torch.cuda.synchronize()
        info[w] = dict(workspace_tokens=m._ws_tokens, workspace_MB=round(m.engine.workspace_bytes(m._ws_tokens) / 1e6, 1),
                       peak_alloc_MB=round(torch.cuda.max_memory_allocated() / 1e6, 1))
    same = bool(torch.equal(outs["one_prefill"], outs["repeated_batch"]))
    times = {w: [] for w in ways}
    for _ in range(reps):
        for w, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[w].append(time.perf_counter() - t0)
    for w in ways:
        print(json.dumps(dict(bench="nbest_e2e", model=name, B=B, n=n, prompt=P, new_tokens=new, way=w, same_tokens=same,
                              generate_s=round(statistics.median(times[w]), 4),
                              generate_s_all=[round(t, 4) for t in times[w]], **info[w])), flush=True)
    cap = -(-(P + new) // 64) * 64
    cache = torch.empty(m.engine.kv_cache_bytes(B * n, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B * n, cap)
    lens = torch.zeros(B * n, dtype=torch.int32, device=dev)
    logits = torch.empty(B * n, m.config.vocab_size, dtype=torch.float32, device=dev)
    t = []
    for _ in range(6):
        lens[:B] = P
        m.engine.prefill(ids, lens, B, P, logits)
        t.append(ev_ms(lambda: m.engine.kv_repeat(n, lens, logits)))
    print(json.dumps(dict(bench="kv_repeat", model=name, B=B, n=n, prompt=P, kv_repeat_ms=round(statistics.median(t[1:]), 4),
                          cache_MB_copied=round(m.engine.kv_cache_bytes(B * (n - 1), P) / 1e6, 1))), flush=True)
    del m, cache
    torch.cuda.empty_cache()


def chunked_prefill_bench(name, B, T, C, reps=5):
    """One slam_prefill of [B, T] against slam_prefill + slam_extend in chunks of C columns."""
    import torch
    m = build(name, B * T)
    dev = m.device
    V = m.config.vocab_size
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, V, (B, T), device=dev, generator=g)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    cap = -(-(T + 64) // 64) * 64
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    m._ensure_workspace(B * T)  # one workspace for both ways: the timed launches are the same whatever is bound
    logits = {w: torch.empty(B, V, dtype=torch.float32, device=dev) for w in ("one_shot", "chunked")}
    chunks = [(c0, min(C, T - c0)) for c0 in range(0, T, C)]
    parts = [(ids[:, c0:c0 + w].contiguous(), (full - c0).clamp(min=0, max=w).contiguous(), w) for c0, w in chunks]
    cur = torch.empty_like(full)

    def one_shot():
        m.engine.prefill(ids, full, B, T, logits["one_shot"])

    def chunked():
        cur.copy_(parts[0][1])
        m.engine.prefill(parts[0][0], cur, B, parts[0][2], logits["chunked"])
        for x, nl, w in parts[1:]:
            m.engine.extend(x, nl, cur, B, w, logits["chunked"])

    ways = {"one_shot": one_shot, "chunked": chunked}
    for fn in ways.values():  # warm-up of each way
        fn()
    torch.cuda.synchronize()
    assert cur.tolist() == [T] * B
    times = {w: [] for w in ways}
    for _ in range(reps):
        for w, fn in ways.items():
            times[w].append(ev_ms(fn))
    a, b = logits["chunked"].double(), logits["one_shot"].double()
    rel = float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    tok = {"one_shot": max(B * T, 2 * B), "chunked": max(B * min(T, C), 2 * B)}
    med = {w: statistics.median(times[w]) for w in ways}
    for w in ways:
        r = dict(bench="chunked_prefill", model=name, B=B, T=T, chunk=C, way=w, prefill_ms=round(med[w], 3),
                 prefill_ms_all=[round(t, 3) for t in times[w]], workspace_tokens=tok[w],
                 workspace_MB=round(m.engine.workspace_bytes(tok[w]) / 1e6, 1))
        if w == "chunked":
            r.update(ratio=round(med["chunked"] / med["one_shot"], 3), logits_rel_rms=float(f"{rel:.3e}"))
        print(json.dumps(r), flush=True)
    del m, cache
    torch.cuda.empty_cache()


def logprob_op_bench(calls=200, rounds=5):
    """Device-event time of slam_token_logprobs alone."""
    import torch
    from slamkit_amd import engine as E
    dev = torch.device("cuda")
    for B, V in ((64, 502), (64, 152167)):
        g = torch.Generator(device=dev).manual_seed(V + B)
        logits = torch.randn(B, V, device=dev, generator=g) * 3.0
        tok = torch.randint(0, V, (B,), device=dev, generator=g)
        out = torch.empty(B, calls, dtype=torch.float32, device=dev)
        ws = torch.empty(E.token_logprobs_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
        done = torch.zeros(B, dtype=torch.uint8, device=dev)
        fin = torch.zeros(B, dtype=torch.uint8, device=dev)

        def run():
            for k in range(calls):
                E.token_logprobs(logits, tok, out, k, ws, done, fin)

        run()
        torch.cuda.synchronize()
        t = [ev_ms(run) / calls * 1e3 for _ in range(rounds)]
        print(json.dumps(dict(bench="logprob_op", B=B, vocab=V, logprobs_us=round(statistics.median(t), 2),
                              logprobs_us_minmax=[round(min(t), 2), round(max(t), 2)],
                              logits_MB=round(B * V * 4 / 1e6, 2))), flush=True)


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
        if not any(k in name for k in ("gemm_skinny", "skinny_reduce", "attn_decode", "rmsnorm_fwd", "swiglu_fwd", "attn_extend", "kv_extend_scatter",
                                       "attn_fwd")):
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
    ap.add_argument("--sampler", default=None, help="torch,engine: end-to-end generate per sampler, alternated")
    ap.add_argument("--do-sample", action="store_true", help="with --sampler: temperature 0.8, top_k 25 instead of greedy")
    ap.add_argument("--sample-op", action="store_true", help="time the token choice alone (engine vs torch ops)")
    ap.add_argument("--warp", action="store_true",
                    help="with --sample-op: slam_sample_tokens_warped beside slam_sample_tokens; with --sampler engine: "
                         "sampled generate without and with min_p / typical_p / epsilon_cutoff / eta_cutoff")
    ap.add_argument("--constrain-op", action="store_true", help="time slam_constrain_scores alone (in place and copying)")
    ap.add_argument("--no-repeat-ngram", type=int, default=0,
                    help="n, with --sampler S: end-to-end greedy generate without and with no_repeat_ngram_size=n, alternated")
    ap.add_argument("--num-return-sequences", type=int, default=0,
                    help="n: generate of 8 prompts x n from one prefill vs the repeated batch, kv_repeat and token_logprobs alone")
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="C: prefill of 8 x 2048 prompts in one slam_prefill vs slam_prefill + slam_extend in chunks of C")
    ap.add_argument("--decode-weights", default=None, choices=["bf16", "fp8"],
                    help="decode step per model and batch: fp8 alternates blocks from bf16 weights and from FP8 codes; bf16 runs "
                         "the bf16 blocks alone")
    ap.add_argument("--cfg", action="store_true",
                    help="classifier-free guidance: the guided step (2 B rows + slam_cfg_scores + the mirror) between plain steps "
                         "at B (--batches, default 1,8,32), then slam_cfg_scores and slam_cfg_mirror_tokens alone")
    ap.add_argument("--batches", default=None, help="with --decode-weights (default 1,8,64) or --cfg (default 1,8,32)")
    ap.add_argument("--blocks", type=int, default=3, help="with --decode-weights: alternations per (model, batch)")
    ap.add_argument("--include-head", action="store_true", help="with --decode-weights fp8: FP8 codes for the LM head too")
    a = ap.parse_args()
    if a.trace_summary:
        trace_summary(a.trace_summary)
        return
    import torch
    assert torch.cuda.is_available()
    if a.cfg:
        for name in a.models.split(","):
            cfg_step_bench(name, [int(b) for b in (a.batches or "1,8,32").split(",")], 256, min(a.steps, 60), a.blocks)
        cfg_op_bench()
        return
    if a.decode_weights:
        for name in a.models.split(","):
            w8_bench(name, [int(b) for b in (a.batches or "1,8,64").split(",")], 256, a.steps, a.blocks, a.decode_weights == "fp8", a.include_head)
        return
    if a.sample_op:
        if a.warp:
            warp_op_bench()
        else:
            sample_op_bench()
        return
    if a.constrain_op:
        constrain_op_bench()
        return
    if a.prefill_chunk > 0:
        for name in a.models.split(","):
            chunked_prefill_bench(name, 8, 2048, a.prefill_chunk)
        return
    if a.num_return_sequences > 1:
        for name in a.models.split(","):
            nbest_bench(name, 8, 256, a.steps, a.reps, a.num_return_sequences)
        logprob_op_bench()
        return
    for name in a.models.split(","):
        m = build(name, 4096)
        if a.sampler:
            if a.warp:
                e2e_warp(m, 8, 256, a.steps, a.reps, name)
            elif a.no_repeat_ngram > 0:
                for smp in a.sampler.split(","):
                    e2e_no_repeat(m, 8, 256, a.steps, a.reps, name, smp, a.no_repeat_ngram)
            else:
                e2e_samplers(m, 8, 256, a.steps, a.reps, name, a.sampler.split(","), a.do_sample)
            del m
            torch.cuda.empty_cache()
            continue
        step_bench(m, 8, 256, a.steps, name)
        if name == "slam":
            step_bench(m, 96, 64, min(a.steps, 60), name)
        e2e(m, 8, 256, a.steps, a.reps, name, reforward=(name == "slam" and not a.no_reforward))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
