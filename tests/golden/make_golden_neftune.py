"""Writes tests/golden/neftune_hf.npz from transformers' own NEFTune hook (transformers.integrations.neftune
.neftune_post_forward_hook), for tests/test_neftune_host.py. Per (alpha, T, H) tuple: the magnitude the hook hands to
uniform_ (its `mag_norm`, as fp32 - captured from the call, not restated) and min / max / mean / variance of the first 2^20
elements of one seeded draw on a zero embedding output of shape [B, T, H].

    python tests/golden/make_golden_neftune.py
"""
import os

import numpy as np
import torch
import transformers
from transformers.integrations.neftune import neftune_post_forward_hook

N = 1 << 20
# (alpha, T, H): HF's recommended range 5 - 15 and its edges, the recipe shapes (hidden 896 / 1536 / 3584, OPT's 768) and tiny ones
CASES = [(5.0, 1024, 896), (10.0, 1024, 896), (15.0, 1024, 896), (5.0, 512, 1536), (5.0, 2048, 1536), (7.5, 1024, 3584),
         (5.0, 1024, 768), (5.0, 4, 256), (5.0, 16, 64), (0.1, 100, 256), (45.0, 37, 8), (1.0, 1, 8)]


def main():
    rows = []
    real = torch.Tensor.uniform_
    for i, (alpha, T, H) in enumerate(CASES):
        emb = torch.nn.Embedding(4, H)
        emb.neftune_noise_alpha = alpha
        emb.train()
        B = -(-N // (T * H))
        seen = []

        def capture(self, a=0.0, b=1.0, **kw):
            seen.append((float(a), float(b)))
            return real(self, a, b, **kw)

        torch.manual_seed(1000 + i)
        torch.Tensor.uniform_ = capture
        try:
            out = neftune_post_forward_hook(emb, None, torch.zeros(B, T, H))
        finally:
            torch.Tensor.uniform_ = real
        assert len(seen) == 1 and seen[0][0] == -seen[0][1]
        x = out.reshape(-1)[:N].double().numpy()
        emb.eval()  # and nothing in eval mode
        assert neftune_post_forward_hook(emb, None, torch.zeros(1, T, H)).abs().max() == 0
        rows.append((alpha, T, H, np.float32(seen[0][1]), x.min(), x.max(), x.mean(), x.var()))
    r = np.array(rows, dtype=np.float64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "neftune_hf.npz")
    np.savez(path, alpha=r[:, 0], T=r[:, 1].astype(np.int64), H=r[:, 2].astype(np.int64), mag_norm=r[:, 3].astype(np.float32),
             x_min=r[:, 4], x_max=r[:, 5], x_mean=r[:, 6], x_var=r[:, 7], n=np.int64(N),
             transformers_version=np.array(transformers.__version__))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
