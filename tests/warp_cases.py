"""The inputs of the slam_sample_tokens_warped kernel test and their fp64 reference, shared by tests/test_gpu_warp.py (the
kernel against it) and tests/test_warp_host.py (the cap on how many draws the 1e-5 band may excuse, asserted on the CPU so that
the GPU test cannot hide a failure behind exclusions). Logits 3 N(0,1), three banned ids, temperature 0.8, 64 draws per row
(steps 0 .. 63, row id = row index)."""
import functools

import numpy as np
import torch

from tests import sampling_ref as R
from tests import warp_ref as W

SHAPES = [(502, 64), (2049, 3), (152167, 3), (152576, 64)]  # (V, B): single launch; smallest two-launch; odd rows; full size
TOP_K = (1, 2, 25, 256)
TOP_P = (1.0, 0.9)
WARPS = {"min_p": (0.1, 1.0, 0.0, 0.0), "typical_p": (0.0, 0.9, 0.0, 0.0), "epsilon": (0.0, 1.0, 3e-3, 0.0),
         "eta": (0.0, 1.0, 0.0, 3e-3), "all": (0.05, 0.95, 1e-3, 2e-3)}
TEMPERATURE, SEED, STEPS, BAND = 0.8, 11, 64, 1e-5


@functools.lru_cache(maxsize=None)
def logits(V, B):
    return (torch.randn(B, V, generator=torch.Generator().manual_seed(7 * V + B)) * 3.0).numpy()


def banned(V):
    m = np.zeros(V, dtype=np.uint8)
    m[[1, V // 3, V - 2]] = 1
    return m


@functools.lru_cache(maxsize=None)
def ranked(V, B):
    """Per row the 256 best candidates in rank order (a prefix of it serves every top_k)."""
    x, bn = logits(V, B), banned(V)
    return [R.candidates(R.scores(x[b], bn), 256) for b in range(B)]


@functools.lru_cache(maxsize=None)
def reference(V, B, warp, top_k, top_p):
    """(tok int64 [B, STEPS] of the fp64 restatement, band bool [B, STEPS]: the row's margin or the draw's distance is within
    BAND) for the warp setting named `warp`."""
    x, bn, rk = logits(V, B), banned(V), ranked(V, B)
    tok = np.empty((B, STEPS), dtype=np.int64)
    band = np.empty((B, STEPS), dtype=bool)
    for b in range(B):
        t, dist, margin = W.sample_row(x[b], bn, top_k, TEMPERATURE, top_p, WARPS[warp], SEED, [b], np.arange(STEPS),
                                       fp64=True, ranked=rk[b])
        tok[b] = t[0]
        band[b] = (dist[0] <= BAND) | (margin <= BAND)
    return tok, band
