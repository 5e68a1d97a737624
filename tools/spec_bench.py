"""What one round of assisted generation (generate(assistant_model=), draft-model speculative decoding) costs against plain
decoding, on randomly initialised models: a Slam-358M-shaped draft under a Qwen2.5-1.5B-shaped and a Qwen2.5-7B-shaped target,
one unit vocabulary of 502, a prompt of 256 tokens in both caches, B in {1, 8}, K in {2, 4, 8}.

Usage: python tools/spec_bench.py [--targets cfg3,7b] [--batches 1,8] [--ks 2,4,8] [--reps 20] [--prompt 256] [--lookup]

Per (target, B, K) one JSON line with wall-clock medians in ms, the host synchronised before and behind every timed part (the
launch cost of a part is inside its figure, as it is in the loop):
  draft_ms      the draft's part of a round: slam_extend of the catch-up block (T = 2), K slam_sample_tokens_at, K - 1
                slam_decode_step
  verify_ms     the target's part: slam_extend_logits over [B, K + 1], one slam_sample_tokens_at over B (K + 1) rows
  accept_ms     slam_spec_accept, the read-back of its five counters, the two slam_kv_rewind
  round_ms      the three parts back to back with the round's one synchronisation (the read-back)
  plain_ms      K + 1 plain steps of the target: slam_decode_step + slam_sample_tokens each, one synchronisation behind them
  plain_step_ms plain_ms / (K + 1)
  break_even_tokens_per_round   round_ms / plain_step_ms: the mean number of tokens a round has to emit (1 .. K + 1) for assisted
                generation to match plain decoding; above K + 1 no acceptance rate can reach it
Rounds and plain steps are alternated rep by rep in one process; every rep starts from the same cache lengths (the rollback
restores them). Random weights accept nothing, so this tool measures COST only: the speed-up at a real acceptance rate needs a
trained draft / target pair and is not claimed from these figures.

--lookup adds prompt-lookup decoding (generate(prompt_lookup_num_tokens=)) to the same reps - lookup parts, lookup round, draft
parts, draft round and plain steps alternated rep by rep in the one process - and prints a second line per (target, B, K):
  propose_ms    slam_ngram_propose (max_ngram 2) on the 256-token prompt plus one new token, its two statistics included
  verify_ms     as above (the same launches)
  accept_ms     slam_spec_accept, the read-back of the seven counters, the target's slam_kv_rewind
  round_ms      the three parts back to back with the one synchronisation
  break_even_tokens_per_round   round_ms / plain_step_ms, and draft_break_even_tokens_per_round of the same reps beside it
and, before the targets, one line per (B, history length) of the proposal kernel alone (no model; 50 calls back to back per
timed window, the figure is the window / 50): random ids over the 502 units at max_ngram 2 and 16, and the worst case of a
constant history, where every window matches max_ngram = 16 tokens back."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = 502
MODELS = {"slam": "Qwen/Qwen2.5-0.5B", "cfg3": "Qwen/Qwen2.5-1.5B", "7b": "Qwen/Qwen2.5-7B"}


def build(name, max_tokens):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    return UnitLM(UnitLMConfig(base_model_name=MODELS[name], vocab_size=VOCAB, max_tokens=max_tokens), allocate_grads=False, seed=0)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench_propose(dev, B, Lh, K, reps):
    """slam_ngram_propose alone on histories of Lh tokens (all but one in the prompt), wall clock with the launch inside."""
    import torch
    from slamkit_amd import engine as E
    g = torch.Generator(device=dev).manual_seed(B + Lh)
    chunk = torch.ones(B, K + 1, dtype=torch.int64, device=dev)
    n_prop = torch.zeros(B, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    plen = torch.full((B,), Lh - 1, dtype=torch.int32, device=dev)
    n_new = torch.ones(B, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    out = {}
    for name, mx in (("random", 2), ("random16", 16), ("constant16", 16)):
        prompt = torch.randint(2, VOCAB, (B, Lh - 1), device=dev, generator=g)
        if name == "constant16":
            prompt.fill_(7)
        new = prompt[:, :8].clone()

        def many():  # 50 back to back per timed window: one call is a few microseconds of kernel behind its launches
            for _ in range(50):
                E.ngram_propose(chunk, n_prop, mx, 0, prompt, plen, new, n_new, done, None, stats)

        t = [wall_ms(many) / 50 for _ in range(reps + 2)][2:]
        out[name + "_ms"] = round(statistics.median(t), 4)
        out[name + "_proposed"] = int(stats[1])
    print(json.dumps(dict(bench="ngram_propose", B=B, history=Lh, K=K, **out, reps=reps)), flush=True)


def bench(target, draft, tag, B, K, P, reps, lookup=False):
    import torch
    from slamkit_amd import engine as E
    dev, V, K1 = target.device, VOCAB, K + 1
    cap = -(-(P + 2 * K1 + 2) // 64) * 64
    g = torch.Generator(device=dev).manual_seed(B * 16 + K)
    ids = torch.randint(2, V, (B, P), device=dev, generator=g)
    base = torch.full((B,), P, dtype=torch.int32, device=dev)
    target._ensure_workspace(max(B * P, B * K1, 2 * B))
    draft._ensure_workspace(max(B * P, 2 * B))
    caches = []
    logits, logits_d = (torch.empty(B, V, dtype=torch.float32, device=dev) for _ in range(2))
    for m, lg in ((target, logits), (draft, logits_d)):
        caches.append(torch.empty(m.engine.kv_cache_bytes(B, cap) + 256, dtype=torch.uint8, device=dev))
        off = (-caches[-1].data_ptr()) % 256
        m.engine.bind_kv_cache(caches[-1][off:], B, cap)
        m.engine.prefill(ids, base.clone(), B, P, lg)
    desc = E.SlamSampleDesc(do_sample=1, top_k=25, temperature=0.8, top_p=1.0, seed=11, step=0, pad_id=0, n_eos=0)
    ws = torch.empty(E.sample_workspace_bytes(B * K1, V, 25), dtype=torch.uint8, device=dev)
    lens_t, lens_d, prompt_len = base.clone(), base.clone(), base.clone()
    n_new = torch.ones(B, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    nxt = torch.ones(B, dtype=torch.int64, device=dev)
    chunk = torch.ones(B, K1, dtype=torch.int64, device=dev)
    tgt = torch.ones(B, K1, dtype=torch.int64, device=dev)
    new = torch.zeros(B, 4096, dtype=torch.int64, device=dev)
    draft_ids = torch.ones(B, 2, dtype=torch.int64, device=dev)
    draft_new_lens = torch.ones(B, dtype=torch.int32, device=dev)
    tgt_new_lens = torch.full((B,), K1, dtype=torch.int32, device=dev)
    logits_all = torch.zeros(B, K1, V, dtype=torch.float32, device=dev)
    stats = torch.zeros(7, dtype=torch.int32, device=dev)  # slam_spec_accept's five, slam_ngram_propose's two
    n_prop = torch.zeros(B, dtype=torch.int32, device=dev)
    scratch = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 2, dtype=torch.int64, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))  # the draft side of slam_spec_accept under lookup: read by nothing

    def reset():
        for t in (lens_t, lens_d):
            t.copy_(base)
        n_new.fill_(1)
        done.zero_()
        draft_new_lens.fill_(1)
        tgt_new_lens.fill_(K1)
        target.engine.kv_rewind(P)
        draft.engine.kv_rewind(P)

    def draft_part():
        draft.engine.extend(draft_ids, draft_new_lens, lens_d, B, 2, logits_d)
        for j in range(1, K1):
            desc.step = j - 1
            E.sample_tokens_at(logits_d, desc, nxt, ws, n_new, 1, j, out=chunk)
            if j < K:
                draft.engine.decode_step(nxt, lens_d, B, logits_d)

    def verify_part():
        target.engine.extend_logits(chunk, tgt_new_lens, lens_t, B, K1, logits_all)
        desc.step = 0
        E.sample_tokens_at(logits_all.view(B * K1, V), desc, tgt.view(-1), ws, n_new, K1, 0)

    def accept_part():
        E.spec_accept(chunk, tgt, K, new.shape[1], 0, None, prompt_len, n_new, done, new, lens_t, lens_d, draft_ids,
                      draft_new_lens, tgt_new_lens, stats)
        st = stats.tolist()
        target.engine.kv_rewind(max(1, st[1]))
        draft.engine.kv_rewind(max(1, st[2]))
        return st

    def one_round():
        draft_part()
        verify_part()
        accept_part()

    def propose_part():
        E.ngram_propose(chunk, n_prop, 2, 0, ids, prompt_len, new, n_new, done, None, stats[5:])

    def lookup_accept_part():
        E.spec_accept(chunk, tgt, K, new.shape[1], 0, None, prompt_len, n_new, done, new, lens_t, scratch[0], scratch[1],
                      scratch[2], tgt_new_lens, stats)
        st = stats.tolist()
        target.engine.kv_rewind(max(1, st[1]))
        return st

    def lookup_round():
        propose_part()
        verify_part()
        lookup_accept_part()

    def plain():
        for s in range(K1):
            desc.step = s
            E.sample_tokens(logits, desc, nxt, ws, out=new)
            target.engine.decode_step(nxt, lens_t, B, logits)

    t = {k: [] for k in ("draft", "verify", "accept", "round", "plain")}
    tl = {k: [] for k in ("propose", "verify", "accept", "round")}
    emitted = 0
    for rep in range(reps + 2):  # two warm-up reps
        if lookup:
            reset()
            la = wall_ms(propose_part)
            lb = wall_ms(verify_part)
            lc = wall_ms(lookup_accept_part)
            reset()
            lr = wall_ms(lookup_round)
            if rep >= 2:
                for k, v in zip(tl, (la, lb, lc, lr)):
                    tl[k].append(v)
        reset()
        a = wall_ms(draft_part)
        b = wall_ms(verify_part)
        c = wall_ms(accept_part)
        emitted = int(stats[3])
        reset()
        r = wall_ms(one_round)
        reset()
        p = wall_ms(plain)
        if rep >= 2:
            for k, v in zip(t, (a, b, c, r, p)):
                t[k].append(v)
    med = {k: statistics.median(v) for k, v in t.items()}
    step = med["plain"] / K1
    print(json.dumps(dict(bench="spec_round", target=tag, draft="slam", B=B, K=K, prompt=P, vocab=V,
                          **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          round_ms_minmax=[round(min(t["round"]), 4), round(max(t["round"]), 4)],
                          plain_step_ms=round(step, 4), break_even_tokens_per_round=round(med["round"] / step, 3),
                          max_tokens_per_round=K1, emitted_last_round=emitted, reps=reps)), flush=True)
    if lookup:
        ml = {k: statistics.median(v) for k, v in tl.items()}
        print(json.dumps(dict(bench="lookup_round", target=tag, B=B, K=K, prompt=P, vocab=V, max_ngram=2,
                              **{f"{k}_ms": round(v, 4) for k, v in ml.items()},
                              round_ms_minmax=[round(min(tl["round"]), 4), round(max(tl["round"]), 4)],
                              plain_step_ms=round(step, 4), break_even_tokens_per_round=round(ml["round"] / step, 3),
                              draft_break_even_tokens_per_round=round(med["round"] / step, 3), max_tokens_per_round=K1,
                              proposed_last_round=int(stats[6]), reps=reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="cfg3,7b")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prompt", type=int, default=256)
    ap.add_argument("--lookup", action="store_true", help="also time prompt-lookup rounds, and the proposal kernel alone")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    if a.lookup:
        for B in (1, 8, 64):
            for Lh in (257, 2048, 8192):
                bench_propose(torch.device("cuda"), B, Lh, 4, a.reps)
    draft = build("slam", 4096)
    for name in a.targets.split(","):
        target = build(name, 4096)
        for B in (int(x) for x in a.batches.split(",")):
            for K in (int(x) for x in a.ks.split(",")):
                bench(target, draft, name, B, K, a.prompt, a.reps, a.lookup)
        del target
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
