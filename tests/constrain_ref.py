"""numpy restatement of slam_constrain_scores (include/slam_engine.h): the tokens a row's own history bans, and the scores.

The history of a row is a plain list of ints (the prompt's real tokens, then the new ones): pads and left padding are not in
it. Every function restates one of transformers' logits processors window for window; tests/test_constrain_host.py holds them
to the installed transformers' own output (tests/golden/constrain_hf.npz), exactly."""
import numpy as np

MAX_SEQS = 256     # SLAM_CONSTRAIN_MAX_SEQS
MAX_SEQ_LEN = 16   # SLAM_CONSTRAIN_MAX_SEQ_LEN
MAX_BEGIN = 256    # SLAM_CONSTRAIN_MAX_BEGIN


def ngram_bans(h, n):
    """NoRepeatNGramLogitsProcessor: nothing for n = 0 or len(h) < n; else every window h[j .. j + n - 1] whose first n - 1
    tokens equal the last n - 1 of h bans h[j + n - 1]."""
    h = [int(t) for t in h]
    L = len(h)
    if n <= 0 or L < n:
        return set()
    p = h[L - n + 1:]
    return {h[j + n - 1] for j in range(L - n + 1) if h[j:j + n - 1] == p}


def sequence_bans(h, seqs):
    """NoBadWordsLogitsProcessor, entries of two tokens and more: w bans w[-1] when len(w) <= len(h) and the last len(w) - 1
    tokens of h equal w[:-1]. Entries shorter than 2 or longer than MAX_SEQ_LEN are ignored, as the kernel ignores them."""
    h = [int(t) for t in h]
    L = len(h)
    out = set()
    for w in seqs:
        w = [int(t) for t in w]
        Lw = len(w)
        if Lw < 2 or Lw > MAX_SEQ_LEN or Lw > L:
            continue
        if h[L - (Lw - 1):] == w[:-1]:
            out.add(w[-1])
    return out


def banned_set(h, step, vocab, n=0, seqs=(), ban_eos=False, eos_ids=(), begin_ids=()):
    """The ids in [0, vocab) that slam_constrain_scores sets to -inf for a row with history h (len(h) = prompt length + step)."""
    b = ngram_bans(h, n) | sequence_bans(h, seqs)
    if ban_eos:
        b |= {int(t) for t in eos_ids}
    if step == 0:
        b |= {int(t) for t in begin_ids}
    return {t for t in b if 0 <= t < vocab}


def constrain(logits, histories, step, n=0, seqs=(), ban_eos=False, eos_ids=(), begin_ids=(), done=None):
    """logits fp32 [B, V]; histories: B lists. Returns (banned sets per row, scores): scores is a copy of logits with -inf at
    the banned ids; a row with done[b] is copied and its set is empty."""
    logits = np.asarray(logits, dtype=np.float32)
    B, V = logits.shape
    scores = logits.copy()
    sets = []
    for b in range(B):
        if done is not None and done[b]:
            sets.append(set())
            continue
        s = banned_set(histories[b], step, V, n, seqs, ban_eos, eos_ids, begin_ids)
        if s:
            scores[b, sorted(s)] = -np.inf
        sets.append(s)
    return sets, scores


def has_repeated_ngram(tokens, n):
    """True when some n-gram occurs twice in tokens."""
    tokens = [int(t) for t in tokens]
    seen = set()
    for j in range(len(tokens) - n + 1):
        g = tuple(tokens[j:j + n])
        if g in seen:
            return True
        seen.add(g)
    return False
