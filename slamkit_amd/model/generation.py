"""KV-cached generation for UnitLM: the bodies of `UnitLM.generate` and `UnitLM.score_continuations`, and their contracts: one
paragraph per option. An option that is off adds no launch.

generate
--------
HF `generate` on the engine's KV cache (the reference calls `generate(input_ids=, attention_mask=, bad_words_ids=[[t], ...],
temperature=, top_k=, max_new_tokens=)` with left-padded prompts). Prompts of either padding side are compacted to per-row
lengths (positions start at each row's first real token, HF's cumsum(mask) - 1), prefilled once, then decoded one token per
step (slam_decode_step). Logits are fp32; bad words get -inf, then temperature, top_k and top_p (sampling only). Finished rows
are padded with pad_token_id; generation stops when every row has emitted eos_token_id. Explicit arguments override
`generation_config`. Returns [B, T_in + n_new] int64: the prompt as passed, padding included, then the new tokens. num_beams !=
1 and repetition_penalty != 1 are refused; OPT models have no KV-cached decode.

`sampler` selects who picks the token. None / "torch": torch ops (torch.multinomial with one generator for the batch: a row's
continuation depends on the batch around it). "engine": slam_sample_tokens picks it on the device and writes it where the next
decode step reads it - no torch op between two engine calls - with a stateless Philox draw keyed on (seed, row id, step): a
row's continuation depends on its prompt, the seed and its row id alone, whatever the batch. `sample_ids` (int64 [B], default 0
.. B-1) are those row ids: a sharded evaluation passes the examples' global indices. The engine sampler needs 1 <= top_k <= 256
and temperature > 0 when sampling, top_p in (0, 1] and at most 16 EOS ids (ValueError otherwise); a tie at the k-th score goes
to the lower id where HF keeps all ties. seed=None draws a 62-bit seed from torch's default CPU generator.

`num_return_sequences` = n (sampling only; HF refuses greedy n-best too) returns [B n, T_in + n_new], row b n + i the i-th
sample of prompt b (HF's order), the prompt part repeated as passed. The B prompts are prefilled ONCE, the cache rows fanned
out to B n rows (slam_kv_repeat) and B n rows decoded: the workspace is max(B T, 2 B n) tokens, not B n T. With
sampler="engine" `sample_ids` has shape [B n] (default 0 .. B n - 1): row b n + i draws what row b n + i of a call on the
prompts repeated n times draws; the torch sampler draws one multinomial over B n rows. The tokens of the two calls are equal
whenever their logits are equal bit for bit, which holds when the longest prompt (the row stride of the prefill) is a multiple
of 128 tokens; at another length the prefill's attention tiles fall differently on the rows of the two batches, the logits
differ by rounding (within the model tolerance) and a draw that lands on a boundary may differ.

`return_logprobs=True` returns GenerateOutput(sequences, logprobs): logprobs fp32 [B n, n_new], the model's own log-softmax
(raw fp32 logits: no banned mask, temperature or truncation) of every new token, its EOS included, 0.0 behind a row's EOS;
trimmed with the sequences. Both samplers get it from slam_token_logprobs.

`prefill_chunk` = C (an int >= 1; None = the one-shot prefill) prefills the prompts C columns at a time: columns [0, min(T, C))
by slam_prefill, every further block of C columns (the last one as wide as what is left) appended to the cache by slam_extend,
rows that have already ended taking no part. The workspace is max(B min(T, C), 2 B n) tokens instead of max(B T, 2 B n): the
chunk, not the prompt length, sets the activation memory. The chunks' attention runs in another kernel than the one-shot
prefill's, so the logits differ from it by rounding (within the model tolerance); a token chosen at a near-tie may differ.

Bans that depend on a row's own history, as HF's logits processors compute them, applied to the fp32 logits before everything
else by one HIP launch per step (slam_constrain_scores) under both samplers: `no_repeat_ngram_size` = n (no n-gram of a row
occurs twice; 0 = off), `bad_words_ids` entries of any length >= 1 (a multi-token entry bans its last token behind its prefix;
at most 256 such entries of at most 16 tokens, ValueError above), `min_new_tokens` and `min_length` (no EOS id while fewer than
min_new_tokens new tokens exist, or while the prompt width as passed plus the new tokens is below min_length),
`begin_suppress_tokens` (banned for the first new token, at most 256 ids) and `suppress_tokens` (banned at every step, merged
with the single-token bad words). A row's history is its REAL tokens: the prompt without its padding, then its new tokens. HF's
windows run over input_ids as passed, left-pad ids included; the two agree unless a window contains a pad id. `return_logprobs`
still returns the raw-logit log-probs: the bans then go into a scores buffer of their own, which only the token choice reads.

`assistant_model` = a smaller UnitLM over the same unit vocabulary (HF's assisted generation, draft-model speculative
decoding). Per round the draft proposes `num_assistant_tokens` = K tokens per row (an int 1 .. 15, default 4; constant: HF's
heuristic schedule is not implemented), the target scores the pending token and the K proposals in one chunk
(slam_extend_logits) and samples its own token at every chunk position, and slam_spec_accept keeps the target's tokens up to
and including the first one the draft did not propose - 1 .. K + 1 tokens per row and round for one stream of the target's
weights. Both models draw with the engine sampler's draw of (seed, row id, step), so token s of row r is sample(the target's
logits after the prefix; seed, r, s) whatever the draft proposed: the output does not depend on the draft, on K or on whether a
draft was used, up to the rounding between the chunk attention and the decode-step attention (the caveat of `prefill_chunk`).
An assistant implies the engine sampler: greedy works under sampler=None too, do_sample=True needs sampler="engine". Rejected
tokens are undone by lowering the rows' cached lengths (slam_kv_rewind). One host synchronisation per round (reading back five
counters), none per token; `model.last_assist_stats` = {"rounds", "proposed", "accepted", "tokens"}. Refused (ValueError): a
draft that is not a UnitLM, is OPT, is this model, is on another device or has another vocab_size; num_return_sequences > 1;
return_logprobs; the history-dependent bans (no_repeat_ngram_size, multi-token bad words, min_new_tokens / min_length,
begin_suppress_tokens) - single-token bad words and suppress_tokens work; more than 1024 rows.

`prompt_lookup_num_tokens` = K (an int 1 .. 15; HF's prompt-lookup decoding, PromptLookupCandidateGenerator) is assisted
generation without a second model: per round one integer kernel (slam_ngram_propose) looks up the row's own last n-gram - n =
`max_matching_ngram_size` (an int 1 .. 16, default 2) down to 1, the longest n with an earlier occurrence, the earliest
occurrence of that n - and proposes up to K of the tokens that followed it, cut in front of an EOS id. The target then verifies
all K + 1 chunk columns of every live row, columns without a proposal holding pad_token_id, and slam_spec_accept keeps its
tokens as above: every emitted token is the target's own draw, so the output does not depend on K, on n or on whether lookup is
used (same rounding caveat), and sampling yields the target's distribution. Up to 1024 rows; both arguments are also read from
`generation_config`. `model.last_assist_stats["proposed"]` counts the tokens actually proposed (not rows x K). Refused
(ValueError): together with assistant_model; max_matching_ngram_size without prompt_lookup_num_tokens; K or n out of range; and
the assistant's list (num_return_sequences > 1, return_logprobs, history-dependent bans, do_sample without sampler="engine").

`min_p`, `typical_p`, `epsilon_cutoff`, `eta_cutoff` (sampling only; also read from `generation_config`) are the second half of
HF's warper chain, applied in HF's order behind temperature, top_k and top_p: min_p in [0, 1] (0 off) drops tokens below min_p
times the top probability; typical_p in (0, 1] (1 off) keeps the tokens whose -log p is closest to the entropy up to that mass;
epsilon_cutoff in [0, 1) (0 off) drops probabilities below it; eta_cutoff in [0, 1) (0 off) drops those below min(eps,
sqrt(eps) exp(-entropy)); ValueError outside these ranges. Each warper renormalises what the ones before it kept and keeps at
least one token. The torch sampler applies HF's definitions to the full row, so top_k=0 works there. The engine sampler applies
them to the ranked top-k candidates inside the sampling kernel (slam_sample_tokens_warped: no further launch, no further random
word, still no torch op between two engine calls), which is HF's chain exactly when 1 <= top_k <= 256 is part of the request -
it has to be under this sampler. Two deviations from HF: a tie at the k-th score goes to the lower id (HF keeps every tie), and
tokens with equal |-log p - entropy| are ordered by rank, (score descending, id ascending), where torch.sort leaves their order
open. Assisted and prompt-lookup decoding verify with the same chain (the draft proposes with it too), so their tokens stay the
target's own draws. Greedy decoding ignores the four, as HF does.

`guidance_scale` = g (a finite float; also read from `generation_config`) other than 1 turns on classifier-free guidance, HF's
UnbatchedClassifierFreeGuidanceLogitsProcessor: the scores become g (a - u) + u, a the log-softmax of the row's logits and u
that of an unconditional twin that reads `negative_prompt_ids` [B, T_neg] (with `negative_prompt_attention_mask`, any padding
side, compacted like the prompts) or, without them, the row's last real prompt token, followed by the same new tokens. HF runs
the twin as a second forward per step; here it rides in the same decode batch. One prefill covers 2 B rows, the B prompts and
then the B unconditional prompts, right-padded to max(T, T_neg); `num_return_sequences` = n fans all of them out, rows [0, B n)
conditional in HF's order and rows [B n, 2 B n) their twins; the cache holds 2 B n rows of roundup(max(T, T_neg) +
max_new_tokens, 64) and the workspace max(2 B min(max(T, T_neg), prefill_chunk), 4 B n) tokens. Per step, in HF's processor
order (guidance first): slam_cfg_scores from the 2 B n logits rows into B n rows of scores, the history bans in place on those,
the single-token mask and the token choice over the B n rows (`sample_ids` keeps B n entries), slam_token_logprobs on the raw
conditional rows for `return_logprobs` (the model's own log-softmax, as above), slam_cfg_mirror_tokens, and the decode step
over 2 B n rows. Both samplers; the engine sampler still has no torch op between two engine calls. Deviations from HF: a
right-padded prompt's default unconditional token is its last REAL token (HF takes the last column, a pad); every branch's real
tokens start at position 0 (HF runs the unconditional branch without position_ids, so a padded negative prompt counts its pads
as positions; unpadded ones agree); where HF would produce NaN (a -inf on either side) the header's rules apply. ValueError: a
non-finite guidance_scale; negative prompts (or their mask) while guidance is off - HF ignores them silently -, with another
batch size than B or with an empty row; max(T, T_neg) + max_new_tokens above max_tokens; guidance together with assistant_model
or prompt_lookup_num_tokens (the verify pass would need guided chunk scores).

score_continuations
-------------------
This model's log-probs of given continuations of the prompts, through the KV cache: the scoring half of
generate(num_return_sequences=n, return_logprobs=True). input_ids [B, T_in] (+ attention_mask, any padding side); continuations
int64 [B n, T_c], right-padded, rows b n .. b n + n - 1 continuing prompt b (generate's order: `out[:, T_in:]` feeds straight
in); continuation_lengths [B n] (0 .. T_c real tokens per row; default T_c; 0 is legal). Returns fp32 [B n, T_c]: the
log-softmax (fp32 scores, never rounded to bf16) of every continuation token given the prompt and the tokens before it, 0.0 at
pads. return_argmax=True returns (logprobs, argmax): argmax int64 [B n, T_c], the model's greedy choice FOR continuation
position t (position t is accepted by a verifier iff it equals argmax[:, t]), -1 at pads.

The prompts are compacted and prefilled ONCE (in chunks of `prefill_chunk` columns if given), the cache fanned out to B n rows
(slam_kv_repeat), and the continuations appended `score_chunk` columns at a time by slam_extend_score (None = one block): a
block's first column is slam_token_logprobs on the logits the rows held before it (the prefill's, then the previous block's
last-token logits), every other column comes from the fused head. The workspace is max(B min(T, prefill_chunk), B n
score_chunk, 2 B n) tokens, and no [B n, T + T_c] batch is formed. Inside the loop the engine calls follow each other with no
torch op between them (every block's operands are built before it). `ignore_tokens` sets the logit mask (those columns count as
-inf) for the call and clears it afterwards. Known exception to the no-torch-op rule: with `ignore_tokens`, one in-place fill
of those columns of the last-token logits follows each block, because slam_token_logprobs reads raw logits and takes no mask.
"""
import math
import types
from typing import List, NamedTuple, Optional

import torch

from .. import engine as E


class GenerateOutput(NamedTuple):
    """generate(return_logprobs=True): the sequences as without it, and the log-probability of every new token."""
    sequences: torch.Tensor
    logprobs: torch.Tensor


def _warp(scores: torch.Tensor, temperature: float, top_k: int, top_p: float, min_p: float = 0.0, typical_p: float = 1.0,
          epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0) -> torch.Tensor:
    """HF's sampling warpers in HF's order: temperature, top-k, top-p, min_p, typical_p, epsilon_cutoff, eta_cutoff (at least
    one token kept; each is HF's own definition on the full row, on what the warpers before it left finite)."""
    if temperature != 1.0:
        scores = scores / temperature
    if top_k > 0:
        kth = torch.topk(scores, min(top_k, scores.shape[-1])).values[:, -1:]
        scores = scores.masked_fill(scores < kth, float("-inf"))
    if top_p < 1.0:
        srt, idx = torch.sort(scores, descending=False)
        cum = srt.softmax(-1).cumsum(-1)
        drop = cum <= (1 - top_p)
        drop[:, -1] = False
        scores = scores.masked_fill(drop.scatter(1, idx, drop), float("-inf"))
    if min_p > 0.0:  # MinPLogitsWarper: probs < min_p * max prob
        probs = scores.softmax(-1)
        scores = scores.masked_fill(probs < min_p * probs.amax(-1, keepdim=True), float("-inf"))
    if typical_p < 1.0:  # TypicalLogitsWarper: the tokens whose -log p is closest to the entropy, up to the mass
        logp = scores.log_softmax(-1)
        ent = -(logp * logp.exp()).nansum(-1, keepdim=True)
        srt, idx = torch.sort((-logp - ent).abs(), descending=False)
        cum = scores.gather(-1, idx).softmax(-1).cumsum(-1)
        last = (cum < typical_p).sum(-1, keepdim=True).clamp_(max=scores.shape[-1] - 1)
        drop = srt > srt.gather(1, last)
        drop[:, 0] = False
        scores = scores.masked_fill(drop.scatter(1, idx, drop), float("-inf"))
    if epsilon_cutoff > 0.0:  # EpsilonLogitsWarper: probs < epsilon, every top-1 score exempt
        drop = (scores.softmax(-1) < epsilon_cutoff) & (scores < scores.amax(-1, keepdim=True))
        scores = scores.masked_fill(drop, float("-inf"))
    if eta_cutoff > 0.0:  # EtaLogitsWarper: probs < min(epsilon, sqrt(epsilon) exp(-entropy))
        logp = scores.log_softmax(-1)
        probs = logp.exp()
        ent = -(logp * probs).nansum(-1, keepdim=True)
        eps = torch.tensor(eta_cutoff, dtype=scores.dtype, device=scores.device)
        eta = torch.min(eps, torch.sqrt(eps) * torch.exp(-ent))
        drop = (scores.softmax(-1) < eta) & (scores < scores.amax(-1, keepdim=True))
        scores = scores.masked_fill(drop, float("-inf"))
    return scores


class _ConstraintPlan(NamedTuple):
    """generate's history-dependent bans, validated on the host (no device): what slam_constrain_scores will be asked for."""
    ngram: int
    min_new: int
    min_length: int
    begin: List[int]
    seqs: List[List[int]]   # bad word sequences of two tokens and more
    single: List[int]       # single-token bad words + suppress_tokens: the vocabulary-wide mask
    eos: List[int]
    active: bool            # some step needs the constrain kernel


def _constraint_plan(no_repeat_ngram_size, min_new_tokens, min_length, begin_suppress, suppress, bad, eos) -> _ConstraintPlan:
    def count(v, name):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be an int >= 0 (got {v!r})")
        return v

    ngram = count(no_repeat_ngram_size, "no_repeat_ngram_size")
    min_new = count(min_new_tokens, "min_new_tokens")
    min_len = count(min_length, "min_length")
    begin = [int(t) for t in begin_suppress]
    if len(begin) > E.CONSTRAIN_MAX_BEGIN:
        raise ValueError(f"begin_suppress_tokens: at most {E.CONSTRAIN_MAX_BEGIN} ids (got {len(begin)})")
    single = [int(t) for t in suppress]
    seqs = []
    for w in bad:
        w = [int(t) for t in w]
        if len(w) < 1:
            raise ValueError("bad_words_ids: an entry needs at least one token")
        if len(w) > E.CONSTRAIN_MAX_SEQ_LEN:
            raise ValueError(f"bad_words_ids: an entry has at most {E.CONSTRAIN_MAX_SEQ_LEN} tokens (got {len(w)})")
        if len(w) == 1:
            single.append(w[0])
        else:
            seqs.append(w)
    if len(seqs) > E.CONSTRAIN_MAX_SEQS:
        raise ValueError(f"bad_words_ids: at most {E.CONSTRAIN_MAX_SEQS} multi-token entries (got {len(seqs)})")
    eos = [int(t) for t in eos]
    if (min_new > 0 or min_len > 0) and len(eos) > 16:
        raise ValueError(f"min_new_tokens / min_length take at most 16 EOS ids (got {len(eos)})")
    active = ngram > 0 or bool(seqs) or bool(begin) or (bool(eos) and (min_new > 0 or min_len > 0))
    return _ConstraintPlan(ngram, min_new, min_len, begin, seqs, single, eos, active)


class _Constrainer:
    """The device side of a _ConstraintPlan for one generate call: the lists, the prompts and the scores buffer. apply() is one
    slam_constrain_scores launch, or none when the step has nothing to ban."""

    def __init__(self, plan: _ConstraintPlan, ids, prompt_len, t_in: int, nret: int, new, keep_logits: bool, dev):
        def i32(v):
            return torch.tensor(v, dtype=torch.int32, device=dev) if len(v) else None

        self.plan, self.ids, self.prompt_len, self.t_in, self.new = plan, ids, prompt_len, t_in, new
        self.eos, self.begin = i32(plan.eos), i32(plan.begin)
        self.seq_tokens = i32([t for w in plan.seqs for t in w])
        off = [0]
        for w in plan.seqs:
            off.append(off[-1] + len(w))
        self.seq_offsets = i32(off) if plan.seqs else None
        self.desc = E.SlamConstrainDesc(step=0, no_repeat_ngram=plan.ngram, n_per_prompt=nret, prompt_stride=0, ban_eos=0,
                                        n_eos=len(plan.eos), n_begin=len(plan.begin), n_seqs=len(plan.seqs),
                                        n_seq_tokens=off[-1])
        self.keep_logits = keep_logits  # slam_token_logprobs reads the raw logits: the bans go into a buffer of their own
        self.scores = None

    def apply(self, logits, step: int, done):
        p = self.plan
        ban_eos = bool(p.eos) and (step < p.min_new or self.t_in + step < p.min_length)
        if not (p.ngram > 0 or p.seqs or ban_eos or (step == 0 and p.begin)):
            return logits
        if self.keep_logits and self.scores is None:
            self.scores = torch.empty_like(logits)
        out = self.scores if self.keep_logits else logits
        self.desc.step = step
        self.desc.ban_eos = int(ban_eos)
        E.constrain_scores(logits, out, self.desc, self.ids, self.prompt_len, self.new, done, self.eos, self.begin,
                           self.seq_tokens, self.seq_offsets)
        return out


def _compact_rows(seq: torch.Tensor, attention_mask, pad: int, what: str):
    """Every row's real tokens moved to the left (stable: their order is kept), pad behind them: (ids [B, T] int64 contiguous,
    lens int32 [B], T = the longest row). seq is on the device already; attention_mask None = every token is real."""
    dev = seq.device
    mask = (attention_mask.to(dev) != 0) if attention_mask is not None else torch.ones_like(seq, dtype=torch.bool)
    order = torch.sort((~mask).to(torch.int8), dim=1, stable=True).indices
    lens = mask.sum(1).to(torch.int32)
    T = int(lens.max())
    if int(lens.min()) < 1:
        raise ValueError(f"every {what} row needs at least one unmasked token")
    ids = seq.gather(1, order)[:, :T]
    ids = torch.where(torch.arange(T, device=dev)[None] < lens[:, None], ids, torch.full_like(ids, pad)).contiguous()
    return ids, lens, T


class _Guidance:
    """Classifier-free guidance of one generate call. The logits hold n conditional rows, then their n unconditional twins;
    apply() is slam_cfg_scores into a scores buffer of n rows, mirror() copies the n chosen tokens behind themselves so that
    the decode step feeds both branches the same token."""

    def __init__(self, scale: float, n: int, vocab: int, dev):
        self.scale, self.n = float(scale), n
        self.scores = torch.empty(n, vocab, dtype=torch.float32, device=dev)
        self.ws = torch.empty(E.cfg_workspace_bytes(n, vocab), dtype=torch.uint8, device=dev)
        self.next = torch.empty(2 * n, dtype=torch.int64, device=dev)
        self.slot = self.next[:n]  # where the token choice is written

    def apply(self, logits):
        E.cfg_scores(logits, self.scale, self.scores, self.ws)
        return self.scores

    def mirror(self):
        E.cfg_mirror_tokens(self.next)
        return self.next


def _bind_cache(model, rows: int, cap: int):
    """A KV cache of `rows` x `cap` positions bound to the model's engine, 256-byte aligned inside the raw buffer returned."""
    nbytes = model.engine.kv_cache_bytes(rows, cap)
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=model.device)
    off = (-raw.data_ptr()) % 256
    model.engine.bind_kv_cache(raw[off:off + nbytes], rows, cap)
    return raw


def _prefill(model, ids, lens, B, T, logits, chunk=None):
    """The prompts into the cache and each row's last-token logits into logits[:B]: slam_prefill over all T columns, or
    (chunk = C) over the first min(T, C) and slam_extend over every further block of C. lens (first B entries: the prompt
    lengths) is left as it is; the chunks advance a copy, which ends equal to it."""
    if chunk is None or T <= chunk:
        model.engine.prefill(ids, lens, B, T, logits)
        return
    full = lens[:B]
    cur = full.clamp(max=chunk).contiguous()
    model.engine.prefill(ids[:, :chunk].contiguous(), cur, B, chunk, logits)
    for c0 in range(chunk, T, chunk):
        w = min(chunk, T - c0)
        new_lens = (full - c0).clamp(min=0, max=w).contiguous()
        model.engine.extend(ids[:, c0:c0 + w].contiguous(), new_lens, cur, B, w, logits)


class _Request(NamedTuple):
    """What one generate call asks for, after `generation_config` and the defaults: built by _resolve, passed down whole. A
    request for no tokens (max_new <= 0) is resolved up to `prefill_chunk` only: the prompts go back whatever else is asked."""
    inputs: torch.Tensor
    max_new: int
    nret: int
    return_logprobs: bool
    do_sample: bool
    temperature: float
    top_k: int
    top_p: float
    late: dict                       # min_p, typical_p, epsilon_cutoff, eta_cutoff: _warp's keywords
    warp: Optional[E.SlamWarpDesc]   # the engine sampler's description of them; None = off, the plain entry points
    eos: List[int]
    pad: int
    plan: _ConstraintPlan
    seed: Optional[int]
    sample_ids: Optional[torch.Tensor]
    prefill_chunk: Optional[int]
    on_device: bool = False          # the engine sampler picks the tokens
    guidance_scale: Optional[float] = None   # not None: guidance is on
    proposer: Optional[object] = None        # a _DraftProposer or a _LookupProposer: the speculative path


def _resolve(model, gc, extra: dict, a: dict) -> _Request:
    """generate's arguments `a` (name -> value, None = not given), `generation_config` and the unknown keywords `extra` as a
    _Request. Every refusal that needs no device is raised here, in this order, before the model's engine is touched."""
    prefill_chunk = a["prefill_chunk"]
    if prefill_chunk is not None and (isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, int) or prefill_chunk < 1):
        raise ValueError(f"prefill_chunk must be None or an int >= 1 (got {prefill_chunk!r})")
    if model.config.is_opt:
        raise ValueError("generate is not implemented for OPT models (the engine's KV-cached decode covers Qwen2 only)")

    def pick(name, default):
        v = a[name] if name in a else extra.pop(name, None)
        if v is not None:
            return v
        g = getattr(gc, name, None) if gc is not None else None
        return g if g is not None else default

    num_beams = pick("num_beams", 1)
    rep = pick("repetition_penalty", 1.0)
    if num_beams != 1:
        raise ValueError("beam search is not supported (num_beams must be 1)")
    if rep != 1.0:
        raise ValueError("repetition_penalty is not supported (must be 1.0)")
    max_new = int(pick("max_new_tokens", 32))
    do_sample = bool(pick("do_sample", False))
    temperature = float(pick("temperature", 1.0))
    top_k = int(pick("top_k", 0) or 0)
    top_p = float(pick("top_p", 1.0))
    late = dict(min_p=float(pick("min_p", 0.0)), typical_p=float(pick("typical_p", 1.0)),
                epsilon_cutoff=float(pick("epsilon_cutoff", 0.0)), eta_cutoff=float(pick("eta_cutoff", 0.0)))
    if not 0.0 <= late["min_p"] <= 1.0:
        raise ValueError(f"min_p must be in [0, 1] (got {late['min_p']})")
    if not 0.0 < late["typical_p"] <= 1.0:
        raise ValueError(f"typical_p must be in (0, 1] (got {late['typical_p']})")
    for name in ("epsilon_cutoff", "eta_cutoff"):
        if not 0.0 <= late[name] < 1.0:
            raise ValueError(f"{name} must be in [0, 1) (got {late[name]})")
    warp = E.SlamWarpDesc(**late)
    warp = warp if do_sample and warp.active else None
    eos = pick("eos_token_id", model.config.eos_token_id)
    eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
    pad = pick("pad_token_id", model.config.pad_token_id)
    if pad is None:
        pad = eos[0] if eos else 0
    plan = _constraint_plan(pick("no_repeat_ngram_size", 0), pick("min_new_tokens", 0), pick("min_length", 0),
                            pick("begin_suppress_tokens", None) or [], pick("suppress_tokens", None) or [],
                            pick("bad_words_ids", None) or [], eos)
    inputs = a["inputs"] if a["inputs"] is not None else a["input_ids"]
    if inputs is None or inputs.dim() != 2:
        raise ValueError("generate needs input_ids [B, T]")
    nret = int(pick("num_return_sequences", 1))
    if nret < 1:
        raise ValueError(f"num_return_sequences must be at least 1 (got {nret})")
    if nret > 1 and not do_sample:
        raise ValueError("num_return_sequences > 1 needs do_sample=True (greedy continuations would all be equal)")
    rq = _Request(inputs, max_new, nret, a["return_logprobs"], do_sample, temperature, top_k, top_p, late, warp, eos, int(pad),
                  plan, a["seed"], a["sample_ids"], prefill_chunk)
    if max_new <= 0:
        return rq
    if extra:
        raise TypeError(f"generate got unsupported arguments {sorted(extra)}")
    sampler = a["sampler"]
    if sampler not in (None, "torch", "engine"):
        raise ValueError(f"sampler must be None, 'torch' or 'engine', not {sampler!r}")
    draft, neg, neg_mask = a["assistant_model"], a["negative_prompt_ids"], a["negative_prompt_attention_mask"]
    lookup_k, lookup_n = pick("prompt_lookup_num_tokens", None), pick("max_matching_ngram_size", None)
    guidance_scale = pick("guidance_scale", None)
    guided, proposer = False, None
    if guidance_scale is not None:
        guidance_scale = float(guidance_scale)
        if not math.isfinite(guidance_scale):
            raise ValueError(f"guidance_scale must be finite (got {guidance_scale})")
        guided = guidance_scale != 1.0
    if not guided and (neg is not None or neg_mask is not None):
        raise ValueError("negative_prompt_ids / negative_prompt_attention_mask need a guidance_scale other than 1")
    if guided and neg is None and neg_mask is not None:
        raise ValueError("negative_prompt_attention_mask needs negative_prompt_ids")
    if guided and (draft is not None or lookup_k is not None):
        raise ValueError("guidance_scale does not combine with assistant_model or prompt_lookup_num_tokens "
                         "(the verify pass would need guided chunk scores)")
    if lookup_k is not None:
        if draft is not None:
            raise ValueError("prompt_lookup_num_tokens and assistant_model exclude each other: one source of proposals")
        proposer = _LookupProposer(lookup_k, lookup_n, rq, sampler)
    elif lookup_n is not None:
        raise ValueError("max_matching_ngram_size needs prompt_lookup_num_tokens")
    if draft is not None:
        proposer = _DraftProposer(model, draft, a["num_assistant_tokens"], rq, sampler)
    elif a["num_assistant_tokens"] is not None:
        raise ValueError("num_assistant_tokens needs an assistant_model")
    on_device = sampler == "engine" or proposer is not None
    if on_device:
        if do_sample and not 1 <= top_k <= 256:
            raise ValueError(f"sampler='engine' samples with 1 <= top_k <= 256 (got top_k={top_k})")
        if do_sample and not temperature > 0:
            raise ValueError(f"sampler='engine' needs temperature > 0 (got {temperature})")
        if do_sample and not 0 < top_p <= 1:
            raise ValueError(f"sampler='engine' needs 0 < top_p <= 1 (got {top_p})")
        if len(eos) > 16:
            raise ValueError(f"sampler='engine' takes at most 16 EOS ids (got {len(eos)})")
    elif rq.sample_ids is not None:
        raise ValueError("sample_ids are the row ids of sampler='engine'; the torch sampler has none")
    return rq._replace(on_device=on_device, guidance_scale=guidance_scale if guided else None, proposer=proposer)


class _EngineSampler:
    """The engine sampler of one generate call. `rows` is the shape of `sample_ids`, `draws` the most logits rows one launch
    reads. Only pick() and pick_at() choose between the plain and the warped entry points; callers set desc.step and n_eos."""

    def __init__(self, rq: _Request, rows: int, draws: int, vocab: int, dev):
        do_sample, seed = rq.do_sample, rq.seed
        if do_sample and seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())
        self.desc = E.SlamSampleDesc(do_sample=int(do_sample), top_k=rq.top_k if do_sample else 1,
                                     temperature=rq.temperature if do_sample else 1.0, top_p=rq.top_p if do_sample else 1.0,
                                     seed=int(seed or 0) & 0xFFFFFFFFFFFFFFFF, step=0, pad_id=rq.pad, n_eos=len(rq.eos))
        self.ws = torch.empty(E.sample_workspace_bytes(draws, vocab, self.desc.top_k), dtype=torch.uint8, device=dev)
        self.banned = None
        if rq.plan.single:  # the vocabulary-wide mask; the history-dependent bans are the _Constrainer's
            self.banned = torch.zeros(vocab, dtype=torch.uint8, device=dev)
            self.banned[torch.tensor(rq.plan.single, dtype=torch.long, device=dev)] = 1
        self.eos_i = torch.tensor(rq.eos, dtype=torch.int32, device=dev) if rq.eos else None
        self.row_ids = None
        if rq.sample_ids is not None:
            self.row_ids = torch.as_tensor(rq.sample_ids).to(dev, torch.int64).contiguous()
            if self.row_ids.shape != (rows,):
                raise ValueError(f"sample_ids must have shape [{rows}], got {list(self.row_ids.shape)}")
        self.warp = rq.warp

    def pick(self, scores, nxt, done, out):
        if self.warp is None:
            E.sample_tokens(scores, self.desc, nxt, self.ws, self.banned, self.row_ids, self.eos_i, done, out)
        else:
            E.sample_tokens_warped(scores, self.desc, nxt, self.ws, self.warp, None, 1, None, self.banned, self.row_ids,
                                   self.eos_i, done, out)

    def pick_at(self, scores, nxt, steps, group: int, col: int, out=None):
        """Row b is column b % group of sequence b // group, drawn at steps[b // group] + desc.step + b % group; no EOS."""
        if self.warp is None:
            E.sample_tokens_at(scores, self.desc, nxt, self.ws, steps, group, col, self.banned, self.row_ids, None, None, out)
        else:
            E.sample_tokens_warped(scores, self.desc, nxt, self.ws, self.warp, steps, group, col, self.banned, self.row_ids,
                                   None, None, out)


class _EnginePicker:
    """_decode's picker for sampler="engine": the kernel writes nxt (the decode step's input), new[:, step], uint8 flags."""

    def __init__(self, rq: _Request, new, nxt, vocab: int, dev):
        rows = new.shape[0]
        self.sampler = _EngineSampler(rq, rows, rows, vocab, dev)
        self.new, self.nxt = new, nxt if nxt is not None else torch.empty(rows, dtype=torch.int64, device=dev)
        self.done = torch.zeros(rows, dtype=torch.uint8, device=dev)

    def begin(self):
        return self.done

    def pick(self, scores, step: int):
        self.sampler.desc.step = step
        self.sampler.pick(scores, self.nxt, self.done, self.new)
        return self.nxt


class _TorchPicker:
    """_decode's picker for the torch sampler: one draw over the batch, and bool done flags that the kernels read as uint8."""

    def __init__(self, rq: _Request, new, eos_t, dev):
        self.rq, self.new, self.eos_t = rq, new, eos_t
        self.bad_idx = torch.tensor(rq.plan.single, dtype=torch.long, device=dev) if rq.plan.single else None
        self.g = None
        if rq.do_sample and rq.seed is not None:
            self.g = torch.Generator(device=dev)
            self.g.manual_seed(int(rq.seed))

    def begin(self):
        self.done = torch.zeros(self.new.shape[0], dtype=torch.bool, device=self.new.device)
        return self.done.view(torch.uint8)

    def pick(self, scores, step: int):
        rq = self.rq
        if self.bad_idx is not None:
            scores = scores.index_fill(1, self.bad_idx, float("-inf"))
        if rq.do_sample:
            scores = _warp(scores, rq.temperature, rq.top_k, rq.top_p, **rq.late)
            nxt = torch.multinomial(torch.softmax(scores, -1), 1, generator=self.g)[:, 0]
        else:
            nxt = scores.argmax(-1)
        nxt = torch.where(self.done, torch.full_like(nxt, rq.pad), nxt)
        self.new[:, step] = nxt
        if self.eos_t is not None:
            self.done |= torch.isin(nxt, self.eos_t)
        return nxt


def _decode(model, rq: _Request, picker, logits, lens, lp, cons, cfg) -> int:
    """The decode loop of both samplers, behind the prefill; the host looks at the done flags every 16 steps only. Returns the
    columns written. logits has the cache's rows; under guidance (cfg) only the first cfg.n are picked and scored."""
    R = logits.shape[0]
    BN = R if cfg is None else cfg.n
    done = picker.begin()  # uint8, for the kernels; picker.done is the same memory in the picker's own dtype
    raw = logits[:BN]
    n = 0
    for step in range(rq.max_new):
        scores = logits if cfg is None else cfg.apply(logits)
        if cons is not None:
            scores = cons.apply(scores, step, done)
        nxt = picker.pick(scores, step)
        if lp is not None:
            E.token_logprobs(raw, nxt, lp[0], step, lp[2], done, lp[1])
        n = step + 1
        if rq.eos and (step % 16 == 15 or n == rq.max_new) and bool(picker.done.all()):
            break
        if n < rq.max_new:
            if cfg is None:
                model.engine.decode_step(nxt, lens, R, logits)
            else:
                if nxt is not cfg.slot:  # the torch picker's token; the engine sampler wrote it there itself
                    cfg.slot.copy_(nxt)
                model.engine.decode_step(cfg.mirror(), lens, R, logits)
    return n


def _refuse_speculative(what: str, rq: _Request, sampler, why: str):  # both proposers, behind their own arguments' checks
    if rq.nret > 1:
        raise ValueError(f"{what} does not support num_return_sequences > 1")
    if rq.return_logprobs:
        raise ValueError(f"{what} does not support return_logprobs")
    if rq.plan.active:
        raise ValueError(f"{what} does not support history-dependent constraints (no_repeat_ngram_size, multi-token "
                         "bad_words_ids, min_new_tokens / min_length, begin_suppress_tokens)")
    if rq.do_sample and sampler != "engine":
        raise ValueError(f"{what} with do_sample=True needs sampler='engine': {why}")


class _DraftProposer:
    """generate(assistant_model=draft): a draft model proposes K tokens per row and round. _speculate binds its workspace and
    cache next to the target's; at the start of a round its cache (lens_d) lags the committed sequence by one token or two."""
    what, trace_attr, n_stats = "assistant_model", "_assist_trace", 5

    def __init__(self, model, draft, k, rq: _Request, sampler):
        from .unit_lm import UnitLM
        if not isinstance(draft, UnitLM):
            raise ValueError(f"assistant_model must be a UnitLM (got {type(draft).__name__})")
        if draft is model:
            raise ValueError("assistant_model must be another model than the target (it needs a KV cache of its own)")
        if draft.config.is_opt:
            raise ValueError("assistant_model must not be an OPT model (the engine's KV-cached decode covers Qwen2 only)")
        if torch.device(draft.device) != torch.device(model.device):
            raise ValueError(f"assistant_model is on {draft.device}, the target on {model.device}")
        if draft.config.vocab_size != model.config.vocab_size:
            raise ValueError(f"assistant_model has vocab_size {draft.config.vocab_size}, the target {model.config.vocab_size}: "
                             f"assisted generation needs one unit vocabulary")
        k = 4 if k is None else k
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= E.SPEC_MAX_K:
            raise ValueError(f"num_assistant_tokens must be an int 1 .. {E.SPEC_MAX_K} (got {k!r}); HF's heuristic schedule is "
                             f"not implemented")
        _refuse_speculative(self.what, rq, sampler, "draft and target must share the stateless draw")
        self.draft, self.K = draft, k

    def setup(self, lens, vocab: int):  # behind the target's copies of lens, in front of its prefill
        self.lens_d = lens.clone()
        self.logits = torch.empty(lens.shape[0], vocab, dtype=torch.float32, device=lens.device)

    def prefill(self, ids, lens, T: int, chunk):
        _prefill(self.draft, ids, lens, ids.shape[0], T, self.logits, chunk)

    def buffers(self, B: int, pad: int, nxt):  # the catch-up block: the pending token, the last proposal if all K were kept
        self.draft_ids = torch.full((B, 2), pad, dtype=torch.int64, device=nxt.device)
        self.draft_ids[:, 0] = nxt

    def propose(self, s):  # catch up with the committed sequence, then K proposals with the draw the target will use
        eng = self.draft.engine
        eng.extend(self.draft_ids, s.draft_new_lens, self.lens_d, s.B, 2, self.logits)
        for j in range(1, self.K + 1):
            s.sampler.desc.step = j - 1
            s.sampler.pick_at(self.logits, s.nxt, s.n_new, 1, j, s.chunk)
            if j < self.K:
                eng.decode_step(s.nxt, self.lens_d, s.B, self.logits)

    def accepted(self, st: list, n_live: int) -> int:  # behind slam_spec_accept; returns the tokens proposed this round
        self.draft.engine.kv_rewind(max(1, st[2]))
        return n_live * self.K

    def trace(self, s):
        return ()


class _LookupProposer:
    """generate(prompt_lookup_num_tokens=K): slam_ngram_propose proposes from the row's own history (the prompt, then `new` up
    to n_new). No second model, cache or catch-up step; the draft side of slam_spec_accept is written and read by nothing."""
    what, trace_attr, n_stats = "prompt_lookup_num_tokens", "_lookup_trace", 7  # slam_spec_accept's five, then the kernel's two
    draft = None

    def __init__(self, k, n, rq: _Request, sampler):
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= E.SPEC_MAX_K:
            raise ValueError(f"prompt_lookup_num_tokens must be an int 1 .. {E.SPEC_MAX_K} (got {k!r})")
        n = 2 if n is None else n
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= E.NGRAM_MAX:
            raise ValueError(f"max_matching_ngram_size must be an int 1 .. {E.NGRAM_MAX} (got {n!r})")
        _refuse_speculative(self.what, rq, sampler, "the verified positions are drawn with the stateless draw")
        self.K, self.ngram = k, n

    def buffers(self, B: int, pad: int, nxt):
        self.lens_d = torch.empty(B, dtype=torch.int32, device=nxt.device)
        self.draft_ids = torch.empty(B, 2, dtype=torch.int64, device=nxt.device)

    def propose(self, s):  # up to K per live row into chunk[:, 1 ..], pad where there is none: all K + 1 columns get verified
        E.ngram_propose(s.chunk, s.n_prop, self.ngram, s.pad, s.ids, s.prompt_len, s.new, s.n_new, s.done, s.sampler.eos_i,
                        s.stats[5:])

    def accepted(self, st: list, n_live: int) -> int:
        return st[6]

    def trace(self, s):
        return (s.n_prop.cpu(),)


def _speculate(model, rq: _Request, ids, lens, T: int):
    """Speculative decoding with rq.proposer on the engine sampler: ids [B, T] the compacted prompts, lens int32 [B]. Returns
    (new [B, n] int64, pad behind a row's end; n). At the start of a round the committed sequence of row b
    is its prompt + n_new[b] tokens and the target's cache holds it without its last token (lens_t). Every row of logits_all
    that the sampler reads for a live row is a real conditional of this round."""
    prop, dev, V, pad, max_new = rq.proposer, model.device, model.config.vocab_size, rq.pad, rq.max_new
    B, K, draft = ids.shape[0], prop.K, prop.draft  # draft: the proposer's model, None where it has none
    if B > E.SPEC_MAX_ROWS:
        raise ValueError(f"{prop.what} takes at most {E.SPEC_MAX_ROWS} rows (got {B})")
    if draft is not None and T + max_new > draft.config.max_tokens:
        raise ValueError(f"prompt length {T} + max_new_tokens {max_new} exceeds the assistant's max_tokens "
                         f"{draft.config.max_tokens}")
    K1 = K + 1
    pre = B * (T if rq.prefill_chunk is None else min(T, rq.prefill_chunk))
    cap = -(-(T + max_new + K) // 64) * 64
    model._ensure_workspace(max(pre, B * K1, 2 * B))
    if draft is not None:
        draft._ensure_workspace(max(pre, 2 * B))
    caches = [_bind_cache(m, B, cap) for m in (model, draft) if m is not None]
    sampler = _EngineSampler(rq, B, B * K1, V, dev)
    prompt_len, lens_t = lens.clone(), lens.clone()
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    if draft is not None:
        prop.setup(lens, V)
    _prefill(model, ids, lens, B, T, logits, rq.prefill_chunk)
    if draft is not None:
        prop.prefill(ids, lens, T, rq.prefill_chunk)
    # token 0 from the target's prefill logits, by the plain pick: new[:, 0], done on an EOS id
    new = torch.full((B, max_new), pad, dtype=torch.int64, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    nxt = torch.empty(B, dtype=torch.int64, device=dev)
    sampler.pick(logits, nxt, done, new)
    sampler.desc.n_eos = 0  # from here on slam_spec_accept looks for the EOS ids: a proposal that is one ends nothing yet
    if max_new == 1:
        done.fill_(1)
    live = done == 0
    n_new = torch.ones(B, dtype=torch.int32, device=dev)
    n_prop = torch.zeros(B, dtype=torch.int32, device=dev) if draft is None else None  # tokens proposed per row
    chunk = torch.full((B, K1), pad, dtype=torch.int64, device=dev)  # the pending token, then the proposals
    chunk[:, 0] = nxt
    tgt = torch.full((B, K1), pad, dtype=torch.int64, device=dev)
    prop.buffers(B, pad, nxt)
    draft_new_lens = live.to(torch.int32)
    tgt_new_lens = draft_new_lens * K1
    logits_all = torch.zeros(B, K1, V, dtype=torch.float32, device=dev)
    stats = torch.zeros(prop.n_stats, dtype=torch.int32, device=dev)
    # what the proposer works on, round after round
    s = types.SimpleNamespace(B=B, pad=pad, sampler=sampler, ids=ids, prompt_len=prompt_len, new=new, n_new=n_new, done=done,
                              nxt=nxt, n_prop=n_prop, chunk=chunk, draft_new_lens=draft_new_lens, stats=stats)
    model._hold = (ids, lens, caches, chunk, tgt, logits_all)
    rows_all, tgt_flat = logits_all.view(B * K1, V), tgt.view(-1)
    n_live = int(live.sum())
    rounds = proposed = accepted = 0
    tokens = B
    trace = getattr(model, prop.trace_attr)
    while n_live > 0:
        prop.propose(s)
        # target: the logits behind every chunk column, and its own token there with the draw a draft used
        model.engine.extend_logits(chunk, tgt_new_lens, lens_t, B, K1, logits_all)
        sampler.desc.step = 0
        sampler.pick_at(rows_all, tgt_flat, n_new, K1, 0)
        if trace is not None:
            rec = (chunk.cpu(), logits_all.cpu(), n_new.cpu(), tgt.cpu())
        E.spec_accept(chunk, tgt, K, max_new, pad, sampler.eos_i, prompt_len, n_new, done, new, lens_t, prop.lens_d,
                      prop.draft_ids, draft_new_lens, tgt_new_lens, stats)
        st = stats.tolist()  # the round's one host synchronisation
        if trace is not None:
            trace.append(rec + (n_new.cpu(),) + prop.trace(s))
        model.engine.kv_rewind(max(1, st[1]))
        proposed += prop.accepted(st, n_live)
        rounds += 1
        accepted += st[4]
        tokens += st[3]
        n_live = st[0]
    model.last_assist_stats = {"rounds": rounds, "proposed": proposed, "accepted": accepted, "tokens": tokens}
    n = int(n_new.max())
    return new[:, :n], n


def _trim(new, n: int, eos_t):  # HF stops right after the step on which the last row finished: drop the all-pad columns
    if eos_t is not None and n > 1:
        all_done = (torch.isin(new, eos_t).cumsum(1) > 0).all(0)
        if bool(all_done.any()):
            n = int(all_done.nonzero()[0]) + 1
            new = new[:, :n]
    return new, n


def generate(model, gc, extra: dict, args: dict):
    """UnitLM.generate: `args` holds its named arguments by name, `gc` is its generation_config, `extra` its **kwargs."""
    rq = _resolve(model, gc, extra, args)
    dev, nret, max_new, pad = model.device, rq.nret, rq.max_new, rq.pad
    neg, neg_mask = args["negative_prompt_ids"], args["negative_prompt_attention_mask"]
    seq_in = rq.inputs.to(dev, torch.int64)
    if max_new <= 0:
        seq = seq_in.repeat_interleave(nret, 0) if nret > 1 else seq_in
        return GenerateOutput(seq, seq.new_zeros(seq.shape[0], 0, dtype=torch.float32)) if rq.return_logprobs else seq
    B, T_in = seq_in.shape
    BN = B * nret  # rows decoded
    ids, lens, T = _compact_rows(seq_in, args["attention_mask"], pad, "prompt")
    guided = rq.guidance_scale is not None
    if guided:
        # the unconditional prompts: the negative prompts, or each row's last real token (HF's input_ids[:, -1:])
        if neg is not None:
            neg = neg.to(dev, torch.int64)
            if neg.dim() != 2 or neg.shape[0] != B:
                raise ValueError(f"negative_prompt_ids must be [{B}, T_neg] (got {list(neg.shape)})")
            if neg_mask is not None and neg_mask.shape != neg.shape:
                raise ValueError("negative_prompt_attention_mask must have the shape of negative_prompt_ids")
            nids, nlens, Tn = _compact_rows(neg, neg_mask, pad, "negative prompt")
        else:
            nids, nlens, Tn = ids.gather(1, (lens.long() - 1)[:, None]), torch.ones_like(lens), 1
        # one batch of 2 B rows, right-padded to the longer width: the B prompts, then their B unconditional twins
        both = torch.full((2 * B, max(T, Tn)), pad, dtype=torch.int64, device=dev)
        both[:B, :T] = ids
        both[B:, :Tn] = nids
        ids, lens, T = both, torch.cat([lens, nlens]), max(T, Tn)
    if T + max_new > model.config.max_tokens:
        raise ValueError(f"prompt length {T} + max_new_tokens {max_new} exceeds max_tokens {model.config.max_tokens}")
    V = model.config.vocab_size
    cfg = _Guidance(rq.guidance_scale, BN, V, dev) if guided else None
    if rq.proposer is not None:
        new, n = _speculate(model, rq, ids, lens, T)
        eos_t = torch.tensor(rq.eos, dtype=torch.long, device=dev) if rq.eos and n > 1 else None
        return torch.cat([seq_in, _trim(new, n, eos_t)[0]], 1)
    cap = -(-(T + max_new) // 64) * 64
    # rows prefilled and rows in the cache: under guidance the conditional rows, then as many unconditional ones
    P, R = (B, BN) if cfg is None else (2 * B, 2 * BN)
    model._ensure_workspace(max(P * (T if rq.prefill_chunk is None else min(T, rq.prefill_chunk)), 2 * R))
    raw = _bind_cache(model, R, cap)  # noqa: F841 - alive until the call returns
    logits = torch.empty(R, V, dtype=torch.float32, device=dev)
    eos_t = torch.tensor(rq.eos, dtype=torch.long, device=dev) if rq.eos else None
    if nret > 1:  # the prefilled rows first; slam_kv_repeat fills the rest
        lens = torch.cat([lens, torch.zeros(R - P, dtype=torch.int32, device=dev)])
    model._hold = (ids, lens)
    new = torch.empty(BN, max_new, dtype=torch.int64, device=dev)
    lp = None
    if rq.return_logprobs:  # lp[:, k] of step k, the rows' "EOS already emitted" flags, the reduction's workspace
        lp = (torch.empty(BN, max_new, dtype=torch.float32, device=dev), torch.zeros(BN, dtype=torch.uint8, device=dev),
              torch.empty(E.token_logprobs_workspace_bytes(BN, V), dtype=torch.uint8, device=dev))
    # prompt_len: a copy, because slam_decode_step advances lens
    # under guidance the bans edit the guided scores in place: the raw logits stay whole for the log-probs anyway
    cons = None
    if rq.plan.active:
        cons = _Constrainer(rq.plan, ids[:B], lens[:B].clone(), T_in, nret, new, lp is not None and cfg is None, dev)
    if rq.on_device:
        picker = _EnginePicker(rq, new, None if cfg is None else cfg.slot, V, dev)
    else:
        picker = _TorchPicker(rq, new, eos_t, dev)
    _prefill(model, ids, lens, P, T, logits, rq.prefill_chunk)
    if nret > 1:
        model.engine.kv_repeat(nret, lens, logits)
    n = _decode(model, rq, picker, logits, lens, lp, cons, cfg)
    new, n = _trim(new[:, :n], n, eos_t)
    seq = torch.cat([seq_in.repeat_interleave(nret, 0) if nret > 1 else seq_in, new], 1)
    return GenerateOutput(seq, lp[0][:, :n].contiguous()) if lp is not None else seq


def score_continuations(model, input_ids, attention_mask, continuations, continuation_lengths, num_per_prompt, score_chunk,
                        prefill_chunk, return_argmax, ignore_tokens):
    """UnitLM.score_continuations (the module's documentation has the contract)."""
    n = num_per_prompt
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"num_per_prompt must be an int >= 1 (got {n!r})")
    for name, v in (("score_chunk", score_chunk), ("prefill_chunk", prefill_chunk)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
            raise ValueError(f"{name} must be None or an int >= 1 (got {v!r})")
    if input_ids is None or input_ids.dim() != 2:
        raise ValueError("score_continuations needs input_ids [B, T]")
    if continuations is None or continuations.dim() != 2:
        raise ValueError("score_continuations needs continuations [B * num_per_prompt, T_c]")
    B, BN, Tc = input_ids.shape[0], input_ids.shape[0] * n, continuations.shape[1]
    if continuations.shape[0] != BN:
        raise ValueError(f"continuations has {continuations.shape[0]} rows; {B} prompts x num_per_prompt {n} need {BN}")
    if continuation_lengths is not None and tuple(continuation_lengths.shape) != (BN,):
        raise ValueError(f"continuation_lengths must have shape [{BN}], got {list(continuation_lengths.shape)}")
    if model.config.is_opt:
        raise ValueError("score_continuations is not implemented for OPT models (the engine's KV cache covers Qwen2 only)")
    dev = model.device
    seq_in = input_ids.to(dev, torch.int64)
    cont = continuations.to(dev, torch.int64)
    clens = (torch.full((BN,), Tc, dtype=torch.int32, device=dev) if continuation_lengths is None
             else continuation_lengths.to(dev, torch.int32))
    if continuation_lengths is not None and BN and (int(clens.min()) < 0 or int(clens.max()) > Tc):
        raise ValueError(f"continuation_lengths must lie in [0, {Tc}]")
    if Tc == 0:
        z = torch.zeros(BN, 0, dtype=torch.float32, device=dev)
        return (z, torch.zeros(BN, 0, dtype=torch.int64, device=dev)) if return_argmax else z
    pad = int(model.config.pad_token_id if model.config.pad_token_id is not None else 0)
    ids, lens, T = _compact_rows(seq_in, attention_mask, pad, "prompt")  # real tokens to the left, as generate does
    if T + Tc > model.config.max_tokens:
        raise ValueError(f"prompt length {T} + continuation length {Tc} exceeds max_tokens {model.config.max_tokens}")
    C = Tc if score_chunk is None else min(score_chunk, Tc)
    cap = -(-(T + Tc) // 64) * 64
    model._ensure_workspace(max(B * (T if prefill_chunk is None else min(T, prefill_chunk)), BN * C, 2 * BN))
    raw = _bind_cache(model, BN, cap)  # noqa: F841 - alive until the call returns
    V = model.config.vocab_size
    logits = torch.empty(BN, V, dtype=torch.float32, device=dev)
    if n > 1:
        lens = torch.cat([lens, torch.zeros(BN - B, dtype=torch.int32, device=dev)])
    # every block's operands, built before the first engine call: ids, real tokens per row, the first column's token and its
    # "row has no token here" flag (slam_token_logprobs writes 0.0 for it), the block's outputs
    valid = torch.arange(Tc, device=dev)[None] < clens[:, None]
    cont = torch.where(valid, cont, torch.full_like(cont, pad))
    blocks = []
    for c0 in range(0, Tc, C):
        w = min(C, Tc - c0)
        blk = cont[:, c0:c0 + w].contiguous()
        blocks.append((w, blk, (clens - c0).clamp(min=0, max=w).contiguous(), blk[:, 0].contiguous(),
                       (clens <= c0).to(torch.uint8).contiguous(), torch.empty(BN, w, dtype=torch.float32, device=dev),
                       torch.empty(BN, w, dtype=torch.int64, device=dev) if return_argmax else None))
    lpws = torch.empty(E.token_logprobs_workspace_bytes(BN, V), dtype=torch.uint8, device=dev)
    first = None
    if return_argmax:  # position 0's greedy choice: slam_sample_tokens (greedy) on the prefill logits
        first = torch.empty(BN, dtype=torch.int64, device=dev)
        gdesc = E.SlamSampleDesc(do_sample=0, top_k=1, temperature=1.0, top_p=1.0, seed=0, step=0, pad_id=pad, n_eos=0)
        sws = torch.empty(E.sample_workspace_bytes(BN, V, 1), dtype=torch.uint8, device=dev)
    lmask = ign = None
    if ignore_tokens is not None:
        ign = torch.as_tensor(list(ignore_tokens), dtype=torch.long, device=dev)
        lmask = torch.zeros(model.engine.padded_vocab(), dtype=torch.uint8, device=dev)
        lmask[ign] = 1
        model.engine.set_logit_mask(lmask)
    model._hold = (ids, lens, blocks)
    try:
        _prefill(model, ids, lens, B, T, logits, prefill_chunk)
        if n > 1:
            model.engine.kv_repeat(n, lens, logits)
        if ign is not None:
            logits.index_fill_(1, ign, float("-inf"))
        if first is not None:
            E.sample_tokens(logits, gdesc, first, sws, lmask)
        for w, blk, nl, tok0, inert, lp_b, am_b in blocks:
            # `inert` is the kernel's in/out `finished` array: read (1 = write 0.0 for the row), then overwritten with
            # `done` (none: zeros). Each block owns its tensor and it is used exactly once.
            E.token_logprobs(logits, tok0, lp_b, column=0, ws=lpws, done=None, finished=inert)
            model.engine.extend_score(blk, nl, lens, BN, w, logits, lp_b, am_b)
            if ign is not None:
                logits.index_fill_(1, ign, float("-inf"))
    finally:
        if lmask is not None:
            torch.cuda.current_stream(dev).synchronize()  # the kernels read the mask: keep it alive until done
            model.engine.set_logit_mask(None)
    lp = torch.cat([b[5] for b in blocks], 1) if len(blocks) > 1 else blocks[0][5]
    if not return_argmax:
        return lp
    # argmax_out[:, t] is the choice AFTER position t: shift by one behind the prefill's choice
    am = torch.cat([first[:, None]] + [b[6] for b in blocks], 1)[:, :Tc]
    return lp, torch.where(valid, am, torch.full_like(am, -1))
