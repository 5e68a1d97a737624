"""Label smoothing of the shifted language-modelling loss, restated in float64 numpy: what HF's
`transformers.trainer_pt_utils.LabelSmoother(epsilon)(logits, labels, shift_labels=True, num_items_in_batch=...)` computes and
what the engine's loss kernels implement under `slam_set_label_smoothing` (include/slam_engine.h).

Over the V columns of `logits`, for position t of a row whose target y = labels[t + 1] is valid (not -100; the last position of a
row has no target), with p = softmax(z) and lse = logsumexp(z):

    nll_t    = lse - z_y
    smooth_t = lse - (1 / V) * sum_v z_v                      (= the mean over v of -log p_v)
    loss     = ((1 - eps) * sum_t nll_t + eps * sum_t smooth_t) / denom
    d loss / d z_j = (p_j - (1 - eps) * [j == y] - eps / V) / denom

denom = num_items when it is given and positive, else the number of valid targets. Everything comes back in the [B, T] layout of
the logits themselves (row m = b * T + t of the engine's `row_loss`): positions without a valid target hold zeros."""
import numpy as np


def label_smoothing(logits, labels, eps, num_items=None, ignore_index=-100):
    """logits [B, T, V] (any float dtype), labels int [B, T]. Returns a dict of float64 arrays: loss (scalar), denom, nll [B, T],
    smooth [B, T], grad [B, T, V], valid [B, T] (bool)."""
    z = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    B, T, V = z.shape
    tgt = np.full((B, T), ignore_index, dtype=np.int64)
    tgt[:, :-1] = lab[:, 1:]
    valid = (tgt != ignore_index) & (tgt >= 0) & (tgt < V)
    mx = z.max(-1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))[..., 0]
    y = np.where(valid, tgt, 0)
    zy = np.take_along_axis(z, y[..., None], -1)[..., 0]
    nll = np.where(valid, lse - zy, 0.0)
    smooth = np.where(valid, lse - z.sum(-1) / V, 0.0)
    denom = float(num_items) if num_items is not None and num_items > 0 else float(valid.sum())
    loss = ((1.0 - eps) * nll.sum() + eps * smooth.sum()) / denom if denom > 0 else 0.0
    p = np.exp(z - lse[..., None])
    onehot = np.zeros_like(z)
    np.put_along_axis(onehot, y[..., None], 1.0, -1)
    grad = (p - (1.0 - eps) * onehot - eps / V) / (denom if denom > 0 else 1.0)
    grad = np.where(valid[..., None], grad, 0.0)
    return dict(loss=np.float64(loss), denom=denom, nll=nll, smooth=smooth, grad=grad, valid=valid)


def label_smoothing_torch(logits, labels, eps, num_items=None):
    """The same loss as a differentiable torch expression (for autograd through a model): logits [B, T, V] -> scalar, in the
    dtype of `logits`."""
    import torch
    z = logits[:, :-1]
    tgt = labels[:, 1:].to(z.device)
    V = z.shape[-1]
    valid = (tgt >= 0) & (tgt < V)
    lse = torch.logsumexp(z, -1)
    zy = z.gather(-1, tgt.clamp(min=0)[..., None])[..., 0]
    nll = torch.where(valid, lse - zy, torch.zeros_like(lse))
    smooth = torch.where(valid, lse - z.sum(-1) / V, torch.zeros_like(lse))
    denom = float(num_items) if num_items is not None and num_items > 0 else float(valid.sum())
    return ((1.0 - eps) * nll.sum() + eps * smooth.sum()) / denom
