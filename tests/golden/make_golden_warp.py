"""Writes tests/golden/warp_hf.npz: what transformers' own logits warpers keep. Run once, on the CPU, against the installed
transformers (python tests/golden/make_golden_warp.py); the tests only read the file.

Seeded continuous logits (3 N(0,1), 256 rows of V = 502) go through TemperatureLogitsWarper, TopKLogitsWarper,
TopPLogitsWarper, MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper in the order of
GenerationMixin._get_logits_processor (a warper that is off is left out, as HF leaves it out), with min_tokens_to_keep = 1.
80 configurations: temperature {0.8, 1.0} x top_k {0, 2, 25, 256} x top_p {1, 0.9} x {min_p 0.1, typical_p 0.9, epsilon 3e-3,
eta 3e-3, all four (0.05, 0.95, 1e-3, 2e-3)}, each on a window of 64 rows that moves through the 256.

  logits  float32 [256, 502]
  config  float64 [80, 8]   temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, first row of the window
  kept    uint8   [80, 64, 63]  np.packbits of HF's "score is finite" mask, row r of the window = logits row (first + r) % 256
"""
import itertools
import os

import numpy as np
import torch
from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper,
                                                    TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper,
                                                    TypicalLogitsWarper)

N, V, ROWS = 256, 502, 64
WARPS = [(0.1, 1.0, 0.0, 0.0), (0.0, 0.9, 0.0, 0.0), (0.0, 1.0, 3e-3, 0.0), (0.0, 1.0, 0.0, 3e-3), (0.05, 0.95, 1e-3, 2e-3)]


def hf_chain(scores, temperature, top_k, top_p, min_p, typical_p, eps, eta):
    chain = []
    if temperature != 1.0:
        chain.append(TemperatureLogitsWarper(temperature))
    if top_k != 0:
        chain.append(TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=1))
    if top_p < 1.0:
        chain.append(TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=1))
    if min_p > 0.0:
        chain.append(MinPLogitsWarper(min_p=min_p, min_tokens_to_keep=1))
    if typical_p < 1.0:
        chain.append(TypicalLogitsWarper(mass=typical_p, min_tokens_to_keep=1))
    if eps > 0.0:
        chain.append(EpsilonLogitsWarper(epsilon=eps, min_tokens_to_keep=1))
    if eta > 0.0:
        chain.append(EtaLogitsWarper(epsilon=eta, min_tokens_to_keep=1, device="cpu"))
    ids = torch.zeros(scores.shape[0], 1, dtype=torch.long)
    for w in chain:
        scores = w(ids, scores)
    return torch.isfinite(scores)


def main():
    logits = (torch.randn(N, V, generator=torch.Generator().manual_seed(20261)) * 3.0).float()
    config, kept = [], []
    grid = itertools.product((0.8, 1.0), (0, 2, 25, 256), (1.0, 0.9), WARPS)
    for c, (t, k, p, w) in enumerate(grid):
        first = (c * 16) % N
        rows = (first + torch.arange(ROWS)) % N
        mask = hf_chain(logits[rows].clone(), t, k, p, *w)
        assert mask.any(-1).all()
        config.append([t, k, p, *w, first])
        kept.append(np.packbits(mask.numpy(), axis=-1))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "warp_hf.npz")
    np.savez_compressed(out, logits=logits.numpy(), config=np.array(config, dtype=np.float64), kept=np.stack(kept))
    print(out, os.path.getsize(out), "bytes,", len(config), "configurations")


if __name__ == "__main__":
    main()
