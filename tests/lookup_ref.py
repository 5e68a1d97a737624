"""numpy restatement of slam_ngram_propose (include/slam_engine.h) - transformers' PromptLookupCandidateGenerator.get_candidates
on one row's history - and of one whole round of prompt-lookup decoding given the target's logits of the chunk: propose, then
the functions of tests/spec_ref.py. Shared by tests/test_lookup_host.py (against tests/golden/lookup_hf.npz) and
tests/test_gpu_lookup.py (the kernel and generate(prompt_lookup_num_tokens=) against it)."""
import numpy as np

from tests import spec_ref as S

STATS = ("rows", "proposed")


def propose(h, K, max_ngram, eos_ids=()):
    """The proposals for the history h (a sequence of ints): (tokens, n, idx) with n the n-gram size that matched and idx the
    start of the matching window; ([], 0, -1) when nothing matches. An EOS cut that empties the proposals keeps (n, idx)."""
    h = [int(t) for t in h]
    L = len(h)
    eos = set(int(e) for e in eos_ids)
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        for idx in range(0, L - n):  # the tail window itself (idx = L - n) is no candidate
            if h[idx:idx + n] == tail:
                cand = h[idx + n:min(idx + n + K, L)]
                for i, t in enumerate(cand):
                    if t in eos:
                        cand = cand[:i]
                        break
                return cand, n, idx  # the earliest match of the longest n; no fall-back when the cut leaves nothing
    return [], 0, -1


def history(prompt, prompt_len, new, n_new, b):
    """Row b's history: its prompt's real tokens, then its new tokens."""
    return list(np.asarray(prompt)[b, :int(prompt_len[b])]) + list(np.asarray(new)[b, :int(n_new[b])])


def propose_rows(chunk, prompt, prompt_len, new, n_new, done, K, max_ngram, fill_id, eos_ids=()):
    """One slam_ngram_propose launch on a copy of chunk [B, K + 1]: returns dict(chunk, n_prop, stats)."""
    chunk = np.array(chunk, dtype=np.int64)
    B = chunk.shape[0]
    assert chunk.shape == (B, K + 1)
    n_prop = np.zeros(B, np.int32)
    for b in range(B):
        cand = [] if done[b] else propose(history(prompt, prompt_len, new, n_new, b), K, max_ngram, eos_ids)[0]
        n_prop[b] = len(cand)
        chunk[b, 1:] = fill_id
        chunk[b, 1:1 + len(cand)] = cand
    stats = np.array([int((n_prop > 0).sum()), int(n_prop.sum())], np.int32)
    return dict(chunk=chunk, n_prop=n_prop, stats=stats)


def lookup_round(chunk, logits_all, prompt, prompt_len, new, n_new, done, K, max_ngram, max_new, pad_id, eos_ids, banned=None,
                 do_sample=False, top_k=1, temperature=1.0, top_p=1.0, seed=0, row_ids=None):
    """One round of generate(prompt_lookup_num_tokens=K): the proposals into chunk[:, 1:], the target's tokens from logits_all
    [B, K + 1, V] (row (b, j): the logits behind chunk column j), then slam_spec_accept. Returns (the dict of spec_ref.accept,
    the dict of propose_rows, excluded [B, K + 1] - all False under greedy)."""
    B = len(n_new)
    prop = propose_rows(chunk, prompt, prompt_len, new, n_new, done, K, max_ngram, pad_id, eos_ids)
    tgt, excl = S.target_tokens(logits_all, n_new, list(range(B)), banned, do_sample, top_k, temperature, top_p, seed, row_ids)
    res = S.accept(prop["chunk"], tgt, n_new, done, prompt_len, new, K, max_new, pad_id, eos_ids)
    return res, prop, excl
