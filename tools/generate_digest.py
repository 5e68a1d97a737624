"""Digests of what UnitLM.generate and UnitLM.score_continuations compute AND of the engine calls they make, one line per
configuration: the check that a refactor of the generation host code leaves both as its parent has them.

Usage: [SLAM_ENGINE_LIB=/path/to/libslam_engine.so] python tools/generate_digest.py [--tree PATH] [--list] [--only TAG] [--host]
--tree PATH puts PATH in front of sys.path, so this one file runs against an unpacked `git archive` of another commit; with one
built library in SLAM_ENGINE_LIB for both trees (csrc unchanged), run it once per tree and diff the outputs: they must be equal.

--host needs no GPU: the refused calls, on a model object that has a config and a device and nothing else (every one of them
is refused before the engine is touched). One line per call: the exception's type and message, or what came back. The matrix
is what tests/test_{cfg,spec,lookup,warp,constrain,score}_host.py exercise, values that only `generation_config` carries, and
pairs of simultaneous errors, which pin the precedence.

The default mode needs a GPU. A line carries the tag, the SHA-256 of the returned sequences (and log-probs / argmax),
`last_assist_stats` where the call set it, and the SHA-256 of the call log: every call of the slamkit_amd.engine functions and
Engine methods named in LOGGED, with its arguments bound to the parameter names - a tensor as (dtype, shape, contiguous), a
ctypes structure as its field values at call time, an Engine as its number in order of appearance. Bodies: q6, w4, q3 of
tools/step_digest.py with a 2-layer draft; 3 left-padded prompts of 5, 37 and 64 real tokens (".T130": 5, 37, 130), 24 new
tokens. A configuration that sets EOS ids takes them from a run of itself without any: the token row 0 emits at step 7 and the
one row 1 emits at step 15, less what the last row emits, so that some row ends early and the last one runs to the end; this is
asserted. As in step_digest.py the configurations of a body run on one model: compare full runs with full runs, --only with
--only."""
import argparse
import ctypes
import hashlib
import inspect
import math
import os
import sys
import types

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--list", action="store_true")
ap.add_argument("--only", default=None)
ap.add_argument("--host", action="store_true")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from slamkit_amd import engine as E  # noqa: E402
from slamkit_amd.model.unit_lm import UnitLM, UnitLMConfig  # noqa: E402

LOGGED = (["sample_tokens", "sample_tokens_at", "sample_tokens_warped", "spec_accept", "ngram_propose", "constrain_scores",
           "token_logprobs", "cfg_scores", "cfg_mirror_tokens"],
          ["bind_workspace", "bind_kv_cache", "prefill", "extend", "extend_logits", "extend_score", "decode_step", "kv_repeat",
           "kv_rewind", "set_logit_mask"])
LOG, ENGINES = [], {}


def _show(v):
    if isinstance(v, torch.Tensor):
        return (str(v.dtype), tuple(v.shape), v.is_contiguous())
    if isinstance(v, ctypes.Structure):
        return tuple((f[0], getattr(v, f[0])) for f in v._fields_)
    if isinstance(v, E.Engine):
        return ENGINES.setdefault(id(v), (len(ENGINES), v))[0]  # holds v: no other Engine gets its id while the body runs
    return v


def _logged(name, fn):
    sig = inspect.signature(fn)

    def wrapper(*a, **kw):
        b = sig.bind(*a, **kw)
        b.apply_defaults()
        LOG.append((name,) + tuple((k, _show(v)) for k, v in b.arguments.items()))
        return fn(*a, **kw)
    return wrapper


def wrap_engine():
    for n in LOGGED[0]:
        setattr(E, n, _logged(n, getattr(E, n)))
    for n in LOGGED[1]:
        setattr(E.Engine, n, _logged(n, getattr(E.Engine, n)))


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


# ---- --host ---------------------------------------------------------------------------------------------------------------------
def host_model(vocab=502, opt=False, max_tokens=8192):
    """tests/test_spec_host.py::_host_model"""
    base = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=2, num_key_value_heads=2, head_dim=64 if opt else 32,
                intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    if opt:
        base = dict(model_type="opt", num_hidden_layers=2, hidden_size=128, num_attention_heads=2, ffn_dim=256,
                    max_position_embeddings=128)
    m = UnitLM.__new__(UnitLM)
    m.config = UnitLMConfig(base_model_name="facebook/opt-125m" if opt else "local", base_config=base, vocab_size=vocab,
                            max_tokens=max_tokens)
    m.device = torch.device("cpu")
    return m


def host_calls():
    """(tag, model, method name, kwargs) of every refused call"""
    NS = types.SimpleNamespace
    m, d, opt, small = host_model(), host_model(), host_model(opt=True), host_model(max_tokens=64)
    meta = host_model()
    meta.device = torch.device("meta")
    ids = torch.ones(2, 4, dtype=torch.long)
    neg = torch.full((2, 6), 3, dtype=torch.long)
    am0 = torch.ones_like(neg)
    am0[1] = 0
    nan = math.nan
    eng = dict(do_sample=True, top_k=5, sampler="engine")
    hist = dict(ngram=dict(no_repeat_ngram_size=2), seq=dict(bad_words_ids=[[3, 4]]), minnew=dict(min_new_tokens=2, eos_token_id=5),
                minlen=dict(min_length=7, eos_token_id=5), begin=dict(begin_suppress_tokens=[3]))
    gen = []

    def g(tag, model=m, **kw):
        kw.setdefault("input_ids", ids)
        kw.setdefault("max_new_tokens", 4)
        gen.append((tag, model, "generate", kw))

    # test_spec_host
    g("assist.type", assistant_model=object())
    g("assist.self", assistant_model=m)
    g("assist.vocab", assistant_model=host_model(vocab=300))
    g("assist.device", assistant_model=meta)
    for bad in (0, 16, -1, 2.0, "4", True):
        g(f"assist.k.{bad!r}", assistant_model=d, num_assistant_tokens=bad)
    g("assist.k.nodraft", num_assistant_tokens=4)
    g("assist.nret", assistant_model=d, num_return_sequences=2, **eng)
    g("assist.logprobs", assistant_model=d, return_logprobs=True)
    for k, c in hist.items():
        g(f"assist.hist.{k}", assistant_model=d, **c)
    g("assist.sample.none", assistant_model=d, do_sample=True, top_k=5)
    g("assist.sample.torch", assistant_model=d, do_sample=True, top_k=5, sampler="torch")
    g("assist.topk", assistant_model=d, do_sample=True, top_k=300, sampler="engine")
    g("assist.optdraft", assistant_model=opt)
    g("assist.opttarget", model=opt, assistant_model=d)
    g("assist.draft_max_tokens", assistant_model=small, input_ids=torch.ones(2, 61, dtype=torch.long))
    g("assist.rows", assistant_model=d, input_ids=torch.ones(1025, 4, dtype=torch.long))
    # test_lookup_host
    g("lookup.with_draft", assistant_model=d, prompt_lookup_num_tokens=4)
    g("lookup.n.alone", max_matching_ngram_size=2)
    for bad in (0, 16, -1, 2.0, "4", True):
        g(f"lookup.k.{bad!r}", prompt_lookup_num_tokens=bad)
    for bad in (0, 17, -1, 2.0, "2", True):
        g(f"lookup.n.{bad!r}", prompt_lookup_num_tokens=4, max_matching_ngram_size=bad)
    g("lookup.nret", prompt_lookup_num_tokens=4, num_return_sequences=2, **eng)
    g("lookup.logprobs", prompt_lookup_num_tokens=4, return_logprobs=True)
    for k, c in hist.items():
        g(f"lookup.hist.{k}", prompt_lookup_num_tokens=4, **c)
    g("lookup.sample.none", prompt_lookup_num_tokens=4, do_sample=True, top_k=5)
    g("lookup.sample.torch", prompt_lookup_num_tokens=4, do_sample=True, top_k=5, sampler="torch")
    g("lookup.topk", prompt_lookup_num_tokens=4, do_sample=True, top_k=300, sampler="engine")
    g("lookup.opt", model=opt, prompt_lookup_num_tokens=4)
    g("lookup.rows", prompt_lookup_num_tokens=4, input_ids=torch.ones(1025, 4, dtype=torch.long))
    g("lookup.gc.k", generation_config=NS(prompt_lookup_num_tokens=99))
    g("lookup.gc.n", generation_config=NS(prompt_lookup_num_tokens=4, max_matching_ngram_size=99))
    g("lookup.gc.n.alone", generation_config=NS(max_matching_ngram_size=3))
    g("lookup.gc.override", generation_config=NS(prompt_lookup_num_tokens=4, max_matching_ngram_size=3), max_matching_ngram_size=0)
    # test_warp_host
    for name, bad in (("min_p", (-0.1, 1.5, nan)), ("typical_p", (0.0, -0.2, 1.5, nan)), ("epsilon_cutoff", (-1e-3, 1.0, 2.0, nan)),
                      ("eta_cutoff", (-1e-3, 1.0, 2.0, nan))):
        for v in bad:
            for s in (None, "engine"):
                g(f"warp.{name}.{v}.{s}", do_sample=True, top_k=25, sampler=s, **{name: v})
            g(f"warp.{name}.{v}.gc", do_sample=True, top_k=25, generation_config=NS(**{name: v}))
        g(f"warp.{name}.override", do_sample=True, top_k=25, generation_config=NS(**{name: 0.5}), **{name: bad[0]})
    for typo in ("min_pp", "typical", "epsilon_cutof", "eta_cut_off", "top_h"):
        g(f"warp.typo.{typo}", do_sample=True, top_k=25, **{typo: 0.1})
    g("warp.topk0.engine", do_sample=True, top_k=0, min_p=0.1, sampler="engine")
    # test_cfg_host (max_tokens 64 there)
    for bad in (math.nan, math.inf, -math.inf):
        g(f"cfg.scale.{bad}", model=small, guidance_scale=bad)
    for s in (None, 1.0, 1):
        g(f"cfg.off.neg.{s!r}", model=small, guidance_scale=s, negative_prompt_ids=neg)
        g(f"cfg.off.mask.{s!r}", model=small, guidance_scale=s, negative_prompt_attention_mask=torch.ones_like(neg))
    g("cfg.mask.alone", model=small, guidance_scale=2.0, negative_prompt_attention_mask=torch.ones_like(neg))
    g("cfg.neg.rows", model=small, guidance_scale=2.0, negative_prompt_ids=neg[:1])
    g("cfg.neg.dim", model=small, guidance_scale=2.0, negative_prompt_ids=neg[0])
    g("cfg.neg.mask.shape", model=small, guidance_scale=2.0, negative_prompt_ids=neg, negative_prompt_attention_mask=am0[:, :3])
    g("cfg.neg.empty_row", model=small, guidance_scale=2.0, negative_prompt_ids=neg, negative_prompt_attention_mask=am0)
    g("cfg.max_tokens", model=small, guidance_scale=2.0, negative_prompt_ids=torch.full((2, 61), 3, dtype=torch.long))
    g("cfg.assist", model=small, guidance_scale=2.0, assistant_model=d)
    g("cfg.lookup", model=small, guidance_scale=2.0, prompt_lookup_num_tokens=3)
    g("cfg.gc.scale", model=small, generation_config=NS(guidance_scale=nan))
    g("cfg.num_beams", model=small, guidance_scale=2.0, num_beams=2)
    g("cfg.repetition_penalty", model=small, guidance_scale=2.0, repetition_penalty=1.2)
    # test_constrain_host: _constraint_plan's refusals, through generate
    for k, c in dict(ngram=dict(no_repeat_ngram_size=-1), ngram_f=dict(no_repeat_ngram_size=2.0), ngram_b=dict(no_repeat_ngram_size=True),
                     minnew=dict(min_new_tokens=-1), minlen=dict(min_length="3"), begin=dict(begin_suppress_tokens=list(range(257))),
                     empty=dict(bad_words_ids=[[]]), long=dict(bad_words_ids=[list(range(17))]),
                     many=dict(bad_words_ids=[[i, i + 1] for i in range(257)]),
                     eos17=dict(min_new_tokens=1, eos_token_id=list(range(17)))).items():
        g(f"plan.{k}", **c)
    # the rest of generate's own refusals, and values that only generation_config carries
    for bad in (0, -1, 2.0, "4", True):
        g(f"prefill_chunk.{bad!r}", prefill_chunk=bad)
    g("opt", model=opt)
    g("no_inputs", input_ids=None)
    g("inputs.dim", input_ids=ids[0])
    g("nret.0", num_return_sequences=0)
    g("nret.greedy", num_return_sequences=2)
    g("sampler.bad", sampler="hip")
    g("engine.topk", do_sample=True, top_k=0, sampler="engine")
    g("engine.temperature", do_sample=True, top_k=5, temperature=0.0, sampler="engine")
    g("engine.top_p", do_sample=True, top_k=5, top_p=0.0, sampler="engine")
    g("engine.eos17", eos_token_id=list(range(17)), sampler="engine")
    g("torch.sample_ids", sample_ids=torch.arange(2))
    g("max_tokens", model=small, input_ids=torch.ones(2, 61, dtype=torch.long))
    g("empty_row", attention_mask=torch.tensor([[1, 1, 1, 1], [0, 0, 0, 0]]))
    g("gc.num_beams", generation_config=NS(num_beams=4))
    g("gc.repetition_penalty", generation_config=NS(repetition_penalty=1.3))
    g("gc.min_p", generation_config=NS(min_p=2.0, do_sample=True, top_k=5))
    g("gc.nret.greedy", generation_config=NS(num_return_sequences=3))
    g("gc.topk.engine", generation_config=NS(do_sample=True, top_k=999), sampler="engine")
    g("gc.ngram", generation_config=NS(no_repeat_ngram_size=-2))
    g("gc.assist.hist", generation_config=NS(begin_suppress_tokens=[3]), assistant_model=d)
    g("gc.eos17.engine", generation_config=NS(eos_token_id=list(range(17))), sampler="engine")
    # two errors at once: which one wins
    g("pair.min_p+sampler", min_p=2.0, sampler="hip")
    g("pair.cfg+assist.k", guidance_scale=2.0, assistant_model=d, num_assistant_tokens=99)
    g("pair.max_new0+kwarg", max_new_tokens=0, frobnicate=1)
    g("pair.max_new0+kwarg.lp.nret", max_new_tokens=0, frobnicate=1, return_logprobs=True, num_return_sequences=2, do_sample=True)
    g("pair.max_new0+sampler", max_new_tokens=0, sampler="hip")
    g("pair.max_new0+nret.greedy", max_new_tokens=0, num_return_sequences=2)
    g("pair.opt+prefill_chunk", model=opt, prefill_chunk=0)
    g("pair.opt+num_beams", model=opt, num_beams=2)
    g("pair.num_beams+repetition_penalty", num_beams=2, repetition_penalty=1.2)
    g("pair.kwarg+sampler", frobnicate=1, sampler="hip")
    g("pair.kwarg+nret.greedy", frobnicate=1, num_return_sequences=2)
    g("pair.plan+no_inputs", no_repeat_ngram_size=-1, input_ids=None)
    g("pair.typical_p+plan", typical_p=0.0, min_new_tokens=-1)
    g("pair.sampler+cfg.scale", sampler="hip", guidance_scale=nan)
    g("pair.cfg.off.neg+lookup.k", negative_prompt_ids=neg, prompt_lookup_num_tokens=99)
    g("pair.lookup.k+assist", prompt_lookup_num_tokens=99, assistant_model=d)
    g("pair.lookup.n.alone+assist.type", max_matching_ngram_size=2, assistant_model=object())
    g("pair.lookup.k+engine.topk", prompt_lookup_num_tokens=99, do_sample=True, top_k=0, sampler="engine")
    g("pair.lookup.sample+engine.topk", prompt_lookup_num_tokens=4, do_sample=True, top_k=0)
    g("pair.assist.k+assist.nret", assistant_model=d, num_assistant_tokens=0, num_return_sequences=2, **eng)
    g("pair.assist.vocab+assist.k", assistant_model=host_model(vocab=300), num_assistant_tokens=0)
    g("pair.assist.nret+logprobs", assistant_model=d, num_return_sequences=2, return_logprobs=True, **eng)
    g("pair.engine.topk+sample_ids.shape", do_sample=True, top_k=0, sampler="engine", sample_ids=torch.arange(5))
    g("pair.torch.sample_ids+empty_row", sample_ids=torch.arange(2), attention_mask=torch.zeros(2, 4, dtype=torch.long))
    g("pair.empty_row+max_tokens", model=small, input_ids=torch.ones(2, 61, dtype=torch.long),
      attention_mask=torch.cat([torch.ones(1, 61), torch.zeros(1, 61)]).long())
    g("pair.cfg.neg.rows+max_tokens", model=small, guidance_scale=2.0, input_ids=torch.ones(2, 61, dtype=torch.long),
      negative_prompt_ids=neg[:1])
    g("pair.max_tokens+lookup.rows", model=small, prompt_lookup_num_tokens=4, input_ids=torch.ones(1025, 61, dtype=torch.long))
    g("pair.assist.rows+draft_max_tokens", assistant_model=small, input_ids=torch.ones(1025, 61, dtype=torch.long))
    # test_score_host
    bare = UnitLM.__new__(UnitLM)
    optish = UnitLM.__new__(UnitLM)
    optish.config = NS(is_opt=True)
    sc = dict(input_ids=torch.zeros(2, 4, dtype=torch.long), continuations=torch.zeros(4, 5, dtype=torch.long), num_per_prompt=2)
    score = [("score.opt", optish, dict(input_ids=sc["input_ids"], continuations=torch.zeros(2, 5, dtype=torch.long)))]
    for i, kw in enumerate((dict(num_per_prompt=0), dict(num_per_prompt=-2), dict(num_per_prompt=1.0), dict(num_per_prompt=True),
                            dict(score_chunk=0), dict(score_chunk=2.0), dict(score_chunk="4"), dict(score_chunk=True),
                            dict(prefill_chunk=0), dict(prefill_chunk=-1), dict(num_per_prompt=3), dict(continuations=None),
                            dict(continuation_lengths=torch.zeros(3, dtype=torch.int32)), dict(input_ids=None),
                            dict(continuations=torch.zeros(4, dtype=torch.long)),
                            dict(num_per_prompt=0, score_chunk=0), dict(score_chunk=0, prefill_chunk=0),
                            dict(prefill_chunk=0, input_ids=None), dict(num_per_prompt=3, continuation_lengths=torch.zeros(3)))):
        score.append((f"score.{i}." + "+".join(kw), bare, dict(sc, **kw)))
    m2 = host_model(max_tokens=64)
    score.append(("score.lengths.range", m2, dict(sc, continuation_lengths=torch.tensor([0, 6, 1, 1]))))
    score.append(("score.empty_row", m2, dict(sc, attention_mask=torch.tensor([[1, 1, 1, 1], [0, 0, 0, 0]]))))
    score.append(("score.max_tokens", m2, dict(sc, input_ids=torch.zeros(2, 60, dtype=torch.long))))
    score.append(("score.Tc0", m2, dict(sc, continuations=torch.zeros(4, 0, dtype=torch.long), return_argmax=True)))
    return gen + [(t, mm, "score_continuations", kw) for t, mm, kw in score]


def run_host():
    for tag, model, method, kw in host_calls():
        if ARGS.only not in (None, tag):
            continue
        if ARGS.list:
            print(tag)
            continue
        try:
            out = getattr(model, method)(**kw)
            out = out if isinstance(out, tuple) else (out,)
            res = "returned " + " ".join(f"{tuple(t.shape)} {t.dtype} {sha(t)}" for t in out)
        except Exception as e:  # noqa: BLE001 - the type is part of the line
            res = f"{type(e).__name__}: {e}"
        print(tag, res, flush=True)


# ---- the default mode -----------------------------------------------------------------------------------------------------------
def _qwen(L, heads, kv, hd, vocab=502, theta=10000.0, qwen3=False, seed=3):
    base = dict(num_hidden_layers=L, hidden_size=256, num_attention_heads=heads, num_key_value_heads=kv, head_dim=hd,
                intermediate_size=512, rms_norm_eps=1e-6, rope_theta=theta, tie_word_embeddings=True)
    if qwen3:
        base["model_type"] = "qwen3"
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=vocab, max_tokens=1024), seed=seed)
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "norm" in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


BODIES = {  # tools/step_digest.py's bodies that have a cache, each with its 2-layer draft
    "q6": lambda: (_qwen(6, 4, 2, 64), _qwen(2, 4, 2, 64, seed=5)),
    "w4": lambda: (_qwen(4, 2, 1, 128, vocab=700, theta=1e6), _qwen(2, 2, 1, 128, vocab=700, theta=1e6, seed=5)),
    "q3": lambda: (_qwen(5, 4, 2, 64, qwen3=True), _qwen(2, 4, 2, 64, qwen3=True, seed=5)),
}
NEW = 24


def prompts(vocab, longest=64, repeats=False):
    """3 left-padded prompts of 5, 37 and `longest` real tokens; repeats: each a short pattern over and over (bigrams recur)"""
    g = torch.Generator().manual_seed(17)
    ids = torch.zeros(3, longest, dtype=torch.long)
    am = torch.zeros(3, longest, dtype=torch.long)
    for b, n in enumerate((5, 37, longest)):
        row = torch.randint(2, vocab, (n,), generator=g)
        if repeats:
            row = row[:3 + b].repeat(n)[:n]
        ids[b, longest - n:], am[b, longest - n:] = row, 1
    return dict(input_ids=ids, attention_mask=am)


def generate_configs(vocab):
    """(tag, kwargs, sets EOS) of every generate call of a body"""
    S = dict(do_sample=True, top_k=25, temperature=0.8, top_p=0.9, seed=5)
    G = dict(do_sample=False)
    warp = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    bans = dict(no_repeat_ngram_size=2, bad_words_ids=[[11, 12, 13]], min_new_tokens=6, begin_suppress_tokens=[5, 6, 7],
                suppress_tokens=[8, 9])
    P, PL, PR = prompts(vocab), prompts(vocab, 130), prompts(vocab, repeats=True)
    neg = torch.randint(2, vocab, (3, 80), generator=torch.Generator().manual_seed(23))
    nam = torch.ones(3, 80, dtype=torch.long)
    nam[0, :9], nam[1, 70:] = 0, 0
    out = []

    def add(tag, base, eos=True, samplers=(None, "engine"), **kw):
        for s in samplers:
            out.append((f"{tag}.{s or 'torch'}", dict(base, max_new_tokens=NEW, sampler=s, **kw), eos))

    for name, mode in (("greedy", G), ("sampled", S)):
        add(name, P, **mode)
        add(name + ".T130", PL, **mode)
    add("sampled.ids", P, samplers=("engine",), sample_ids=torch.tensor([7, 1 << 33, 3]), **S)
    add("nbest3", P, num_return_sequences=3, **S)
    add("nbest3.lp", P, num_return_sequences=3, return_logprobs=True, **S)
    add("chunk48", P, prefill_chunk=48, **S)
    add("chunk48.T130", PL, prefill_chunk=48, **G)
    add("bans", P, **bans, **S)
    add("bans.lp", P, return_logprobs=True, **bans, **S)
    add("warp", P, **warp, **S)
    add("cfg.g15", P, guidance_scale=1.5, **S)
    add("cfg.g3.neg", P, guidance_scale=3.0, negative_prompt_ids=neg, negative_prompt_attention_mask=nam, **G)
    add("cfg.g05.n2.bans.lp", P, guidance_scale=0.5, num_return_sequences=2, return_logprobs=True, **bans, **S)
    E_ = ("engine",)
    for K in (1, 4):
        add(f"assist.K{K}.greedy", P, samplers=(None,), assistant_model="draft", num_assistant_tokens=K, **G)
        add(f"assist.K{K}.sampled", P, samplers=E_, assistant_model="draft", num_assistant_tokens=K, **S)
        add(f"assist.K{K}.sampled.warp", P, samplers=E_, assistant_model="draft", num_assistant_tokens=K, **warp, **S)
    add("assist.greedy.warp", P, samplers=E_, assistant_model="draft", **warp, **G)
    add("assist.bad1", P, samplers=E_, assistant_model="draft", bad_words_ids=[[21], [22]], suppress_tokens=[23], **S)
    add("assist.chunk48.T130", PL, samplers=E_, assistant_model="draft", prefill_chunk=48, **S)
    out.append(("assist.new1.engine", dict(P, max_new_tokens=1, assistant_model="draft", sampler="engine", eos_token_id=[], **S), False))
    for K, n in ((3, 2), (15, 1)):
        add(f"lookup.K{K}n{n}.greedy", PR, samplers=(None,), prompt_lookup_num_tokens=K, max_matching_ngram_size=n, **G)
        add(f"lookup.K{K}n{n}.sampled", PR, samplers=E_, prompt_lookup_num_tokens=K, max_matching_ngram_size=n, **S)
    out.append(("lookup.new1.torch", dict(PR, max_new_tokens=1, prompt_lookup_num_tokens=3, eos_token_id=[], **G), False))
    for tag, kw in (("new0", {}), ("new0.lp", dict(return_logprobs=True)),
                    ("new0.n3.lp", dict(return_logprobs=True, num_return_sequences=3, do_sample=True))):
        out.append((tag, dict(P, max_new_tokens=0, **kw), False))
    return out


def score_configs(vocab):
    g = torch.Generator().manual_seed(29)
    P = prompts(vocab)
    c1, c3 = torch.randint(2, vocab, (3, 20), generator=g), torch.randint(2, vocab, (9, 20), generator=g)
    l3 = torch.tensor([20, 0, 7, 20, 13, 1, 0, 20, 5], dtype=torch.int32)
    return [("score.n1", dict(P, continuations=c1)),
            ("score.n1.chunks.argmax", dict(P, continuations=c1, score_chunk=8, prefill_chunk=48, return_argmax=True)),
            ("score.n3.lens", dict(P, continuations=c3, continuation_lengths=l3, num_per_prompt=3, score_chunk=6)),
            ("score.n3.lens.argmax.ignore", dict(P, continuations=c3, continuation_lengths=l3, num_per_prompt=3, return_argmax=True,
                                                 ignore_tokens=[0, 1, 30])),
            ("score.Tc0", dict(P, continuations=c3[:, :0], num_per_prompt=3, return_argmax=True))]


def eos_for(model, kw, tag):
    """The EOS ids of a configuration, from a run of itself without any (see the module's documentation)."""
    out = model.generate(**dict(kw, eos_token_id=[]))
    new = (out.sequences if hasattr(out, "sequences") else out)[:, kw["input_ids"].shape[1]:].cpu()
    assert new.shape[1] == NEW, (tag, new.shape)
    last = set(new[-1].tolist())
    eos = [t for t in (int(new[0, 7]), int(new[1, 15])) if t not in last]
    assert eos, f"{tag}: the last row emits both EOS candidates"
    return sorted(set(eos))


def run_gpu():
    if not ARGS.list:
        torch.cuda.set_device(0)
        wrap_engine()
    for body, make in BODIES.items():
        vocab = 700 if body == "w4" else 502
        jobs = [(f"{body}/{t}", "generate", kw, e) for t, kw, e in generate_configs(vocab)]
        jobs += [(f"{body}/{t}", "score_continuations", kw, False) for t, kw in score_configs(vocab)]
        jobs = [j for j in jobs if ARGS.only in (None, j[0])]
        if ARGS.list:
            print("\n".join(j[0] for j in jobs))
            continue
        if not jobs:
            continue
        ENGINES.clear()
        model, draft = make()
        for tag, method, kw, sets_eos in jobs:
            kw = {k: (draft if isinstance(v, str) and v == "draft" else v) for k, v in kw.items()}
            parts = []
            if sets_eos:
                kw["eos_token_id"] = eos_for(model, kw, tag)
                parts.append(f"eos {kw['eos_token_id']}")
            del LOG[:]
            model.last_assist_stats = None
            out = getattr(model, method)(**kw)
            torch.cuda.synchronize()
            out = tuple(out) if isinstance(out, tuple) else (out,)
            if sets_eos:  # some row ends early, some row runs to the end
                new = out[0][:, kw["input_ids"].shape[1]:].cpu()
                hit = torch.isin(new, torch.tensor(kw["eos_token_id"]))
                early, full = hit[:, :-1].any(1), ~hit[:, :-1].any(1) & (new.shape[1] == NEW)
                assert bool(early.any()) and bool(full.any()), f"{tag}: EOS {kw['eos_token_id']} early {early.tolist()} full {full.tolist()}"
            parts += [f"{tuple(t.shape)} {sha(t)}" for t in out]
            if model.last_assist_stats is not None:
                parts.append(f"stats {model.last_assist_stats}")
            parts.append(f"calls {len(LOG)} {hashlib.sha256(repr(LOG).encode()).hexdigest()[:16]}")
            print(tag, " ".join(parts), flush=True)


if __name__ == "__main__":
    run_host() if ARGS.host else run_gpu()
