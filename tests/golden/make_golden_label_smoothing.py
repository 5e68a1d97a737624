"""Writes tests/golden/label_smoothing_hf.npz: HF's own label smoothing on a few tiny logits tensors.

    python tests/golden/make_golden_label_smoothing.py        (needs transformers; the tests only read the .npz)

Each case: fp32 logits [B, T, V] and labels [B, T] with runs of -100, through
`transformers.trainer_pt_utils.LabelSmoother(epsilon)(logits, labels, shift_labels=True, num_items_in_batch=n)` - the call
`Trainer.compute_loss` makes under `label_smoothing_factor` - and autograd for d loss / d logits. The logits are handed over as
float64 copies of the fp32 values, so that HF's arithmetic is float64 wherever HF itself does not force float32 (it sums the
-log p_v of a position with dtype=float32: the one float32 step left, see tests/test_label_smoothing_host.py for what it costs).
Keys: n_cases, and per case i: logits_i (fp32), labels_i, eps_i, num_items_i (0 = None), loss_i, grad_i (float64)."""
import os

import numpy as np
import torch
from transformers.trainer_pt_utils import LabelSmoother

SHAPES = [(2, 7, 37), (2, 9, 37), (3, 5, 12)]


def cases():
    g = torch.Generator().manual_seed(20)
    for si, (B, T, V) in enumerate(SHAPES):
        logits = (torch.randn(B, T, V, generator=g) * 3.0).float()
        labels = torch.randint(0, V, (B, T), generator=g)
        labels[0, 2:4] = -100           # a run inside a row
        labels[-1, T - 2:] = -100       # a run at the end of a row
        if si == 1:
            labels[0, :3] = -100        # a run from the start (position 0 is never a target anyway)
        labels[0, 4], labels[1, 1] = 0, V - 1  # targets in the first and in the last column
        n_valid = int((labels[:, 1:] != -100).sum())
        for eps in (0.1, 0.3, 0.0):  # 0.0: HF's plain term alone, float64 throughout (the forced-float32 sum is multiplied by 0)
            for n in (None, n_valid + 5):
                yield logits, labels, eps, n


def main():
    out = {}
    i = 0
    for logits, labels, eps, n in cases():
        x = logits.double().clone().requires_grad_(True)
        loss = LabelSmoother(epsilon=eps)({"logits": x}, labels, shift_labels=True, num_items_in_batch=n)
        loss.backward()
        out[f"logits_{i}"] = logits.numpy()
        out[f"labels_{i}"] = labels.numpy()
        out[f"eps_{i}"] = np.float64(eps)
        out[f"num_items_{i}"] = np.int64(n or 0)
        out[f"loss_{i}"] = loss.detach().double().numpy()
        out[f"grad_{i}"] = x.grad.double().numpy()
        i += 1
    out["n_cases"] = np.int64(i)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "label_smoothing_hf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, i, "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
