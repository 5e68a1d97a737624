"""Writes tests/golden/lookup_hf.npz: what the installed transformers' PromptLookupCandidateGenerator proposes on short histories.

    python tests/golden/make_golden_lookup.py

Histories are drawn from vocabularies of 2 .. 6 ids so that matches exist at every n-gram size. A case is one row: its history,
K (num_output_tokens), max_matching_ngram_size, the EOS ids and the tokens get_candidates appends. A quarter of the cases are
random; the others end in a copy of an earlier stretch of themselves, so that a long match is certain, with the EOS id chosen
as the first token behind the match, as a later one, or as one behind the K tokens. Lengths 1 and 2 are forced every tenth case.
max_length is far away: HF's early return at max_length == input_length + 1 is the accept kernel's business here. Integer
logic: the comparison in tests/test_lookup_host.py is exact. Lists of lists are stored flattened, as values plus offsets."""
import os

import numpy as np
import torch
from transformers.generation.candidate_generator import PromptLookupCandidateGenerator

CASES = 400


def flat(lists):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    val = np.array([t for x in lists for t in x], dtype=np.int32)
    return val, off


def main():
    rng = np.random.default_rng(20240917)
    hist, ks, ns, eos, cand = [], [], [], [], []
    for c in range(CASES):
        V = int(rng.integers(2, 7))
        K = int(rng.integers(1, 16))
        n = int(rng.integers(1, 6)) if c % 8 else 16
        if c % 10 == 0:
            h = rng.integers(0, V, 1 + (c // 10) % 2).tolist()
        elif c % 4 == 0:
            h = rng.integers(0, V, int(rng.integers(3, 40))).tolist()
        else:  # body, then a copy of body[s : s + m]: the tail matches at every n <= m
            body = rng.integers(0, V, int(rng.integers(4, 30))).tolist()
            m = int(rng.integers(1, 7))
            s = int(rng.integers(0, len(body) - 1))
            h = body + body[s:s + m]
        e = []
        kind = c % 5
        if kind and len(h) > 2:
            # where HF's own match lies, found by a run without EOS ids: EOS in front of, inside and behind the candidates
            g0 = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=K, max_matching_ngram_size=n, max_length=10 ** 6)
            free = g0.get_candidates(torch.tensor([h]))[0][0, len(h):].tolist()
            if kind == 1 and free:
                e = [free[0]]
            elif kind == 2 and len(free) > 1:
                e = [free[len(free) // 2]]
            elif kind == 3:
                e = sorted(set([int(rng.integers(0, V)), V + 1]))  # one id that may occur, one that never does
            elif kind == 4 and free:
                e = sorted(set(range(V)) - set(free))[:1]  # an id behind or beside the candidates, never inside
        g = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(e) if e else None, num_output_tokens=K,
                                           max_matching_ngram_size=n, max_length=10 ** 6)
        out = g.get_candidates(torch.tensor([h]))[0]
        hist.append(h)
        ks.append(K)
        ns.append(n)
        eos.append(e)
        cand.append(out[0, len(h):].tolist())
    out = dict(K=np.array(ks, np.int32), max_ngram=np.array(ns, np.int32))
    for name, lists in (("hist", hist), ("eos", eos), ("cand", cand)):
        out[name + "_val"], out[name + "_off"] = flat(lists)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lookup_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", sum(len(x) > 0 for x in cand), "of", CASES, "cases propose something")


if __name__ == "__main__":
    main()
