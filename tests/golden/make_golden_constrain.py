"""Writes tests/golden/constrain_hf.npz: what the installed transformers' logits processors ban on short unpadded histories.

    python tests/golden/make_golden_constrain.py

Histories are drawn from a six-token alphabet (vocabulary 8) so that n-gram and bad-word matches are frequent. A case is one row:
its history (prompt_len prompt tokens, then `step` new ones), the parameters, and the set of ids HF sets to -inf when
NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor (multi-token entries), MinNewTokensLengthLogitsProcessor,
MinLengthLogitsProcessor and SuppressTokensAtBeginLogitsProcessor run one after the other on zero scores. Integer logic: the
comparison in tests/test_constrain_host.py is exact. Lists of lists are stored flattened, as values plus offsets."""
import os

import numpy as np
import torch
from transformers.generation.logits_process import (MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
                                                    NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                    SuppressTokensAtBeginLogitsProcessor)

V, ALPHABET, CASES = 8, 6, 400


def flat(lists):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    val = np.array([t for x in lists for t in x], dtype=np.int32)
    return val, off


def main():
    rng = np.random.default_rng(20240611)
    hist, plen, ngram, seqs, seq_case, eos, min_new, min_len, begin, banned = [], [], [], [], [0], [], [], [], [], []
    for c in range(CASES):
        pl = int(rng.integers(1, 12))
        step = int(rng.integers(0, 30)) if c % 5 else 0
        h = rng.integers(0, ALPHABET, pl + step).tolist()
        n = int(rng.integers(0, 6))
        ws = [rng.integers(0, ALPHABET, int(rng.integers(2, 5))).tolist() for _ in range(int(rng.integers(0, 5)))]
        if c % 7 == 0:  # one entry longer than the history (ignored) and one that is the history's tail plus a token
            ws.append(rng.integers(0, ALPHABET, len(h) + 1).tolist())
            ws.append(h[-2:] + [int(rng.integers(0, ALPHABET))])
        ws = [list(w) for w in dict.fromkeys(tuple(w) for w in ws)]
        e = sorted(set(rng.integers(0, V, int(rng.integers(1, 4))).tolist()))
        mn = int(rng.integers(0, 8)) if c % 3 == 0 else 0
        ml = int(rng.integers(0, 30)) if c % 4 == 0 else 0
        bg = sorted(set(rng.integers(0, V, int(rng.integers(0, 3))).tolist()))
        ids = torch.tensor([h], dtype=torch.long)
        scores = torch.zeros(1, V)
        if n > 0:
            scores = NoRepeatNGramLogitsProcessor(n)(ids, scores)
        if ws:
            scores = NoBadWordsLogitsProcessor(ws, eos_token_id=None)(ids, scores)
        if mn > 0:
            scores = MinNewTokensLengthLogitsProcessor(pl, mn, e)(ids, scores)
        if ml > 0:
            scores = MinLengthLogitsProcessor(ml, e)(ids, scores)
        if bg:
            scores = SuppressTokensAtBeginLogitsProcessor(bg, pl)(ids, scores)
        hist.append(h)
        plen.append(pl)
        ngram.append(n)
        seqs.extend(ws)
        seq_case.append(len(seqs))
        eos.append(e)
        min_new.append(mn)
        min_len.append(ml)
        begin.append(bg)
        banned.append(torch.isinf(scores[0]).nonzero()[:, 0].tolist())
    out = dict(vocab=np.int32(V), prompt_len=np.array(plen, np.int32), ngram=np.array(ngram, np.int32),
               min_new_tokens=np.array(min_new, np.int32), min_length=np.array(min_len, np.int32),
               seq_case=np.array(seq_case, np.int32))
    for name, lists in (("hist", hist), ("seq", seqs), ("eos", eos), ("begin", begin), ("banned", banned)):
        out[name + "_val"], out[name + "_off"] = flat(lists)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "constrain_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", sum(len(b) > 0 for b in banned), "of", CASES, "cases ban something")


if __name__ == "__main__":
    main()
