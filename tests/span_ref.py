"""numpy restatement of the SPAN pack rule (slam_forward_unpadded_spans, include/slam_engine.h) and of the logits scatter: a
[B, T] batch whose row b holds its real tokens in the columns [starts[b], starts[b] + lens[b]) - right, left or both-side
padding - becomes one flattened row of M_packed tokens, B segments and one dummy tail segment. With starts = 0 it is
tests/unpad_ref.py's rule. Written on its own (no call into unpad_ref) so that the two can be compared.
Shared by tests/test_span_mask_host.py (the rule itself) and tests/test_gpu_span_mask.py (the kernels, bit for bit)."""
import numpy as np


def clamp_spans(starts, lens, T):
    """The kernels' memory guard: starts to [0, T], lens to [0, T - starts]. The identity on spans that keep their contract."""
    st = np.clip(np.asarray(starts, dtype=np.int64), 0, T)
    return st, np.minimum(np.clip(np.asarray(lens, dtype=np.int64), 0, None), T - st)


def m_packed(lens):
    return -(-int(np.sum(lens)) // 64) * 64


def pack(ids, labels, starts, lens, Mp=None, pad_id=0):
    """The arrays the pack kernel writes for m' in [0, Mp): ids, labels (None without labels), position_ids (int64), seg_start,
    seg_end, row (int32), off (int32 [B + 1], the exclusive prefix sum of the clamped lens). Token (b, t) inside its span goes to
    m' = off[b] + (t - starts[b]) with position t - starts[b]; labels' = -100 at a row's first real token; the tail
    [off[B], Mp) is one segment of pad ids with labels -100, positions from 0 and row -1. starts = None is all zeros."""
    ids = np.asarray(ids, dtype=np.int64)
    B, T = ids.shape
    st, ln = clamp_spans(np.zeros(B) if starts is None else starts, lens, T)
    assert st.shape == (B,) and ln.shape == (B,)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(ln)
    S = int(off[B])
    Mp = m_packed(ln) if Mp is None else int(Mp)
    assert Mp % 64 == 0 and S <= Mp <= -(-(B * T) // 64) * 64
    out = dict(ids=np.empty(Mp, np.int64), labels=None if labels is None else np.empty(Mp, np.int64),
               position_ids=np.empty(Mp, np.int64), seg_start=np.empty(Mp, np.int32), seg_end=np.empty(Mp, np.int32),
               row=np.empty(Mp, np.int32), off=off.astype(np.int32))
    if labels is not None:
        labels = np.asarray(labels, dtype=np.int64)
    for m in range(Mp):  # one packed position at a time, as one thread of the kernel sees it
        if m < S:
            b = int(np.searchsorted(off, m, side="right")) - 1
            k = m - int(off[b])
            t = int(st[b]) + k
            vals = (ids[b, t], -100 if k == 0 else (labels[b, t] if labels is not None else 0), k, off[b], off[b + 1], b)
        else:
            vals = (max(int(pad_id), 0), -100, m - S, S, Mp, -1)
        out["ids"][m], lab, out["position_ids"][m], out["seg_start"][m], out["seg_end"][m], out["row"][m] = vals
        if labels is not None:
            out["labels"][m] = lab
    return out


def scatter_rows(packed, off, starts, B, T):
    """The logits scatter: out[b, starts[b] + k] = packed[off[b] + k] for k < off[b + 1] - off[b], zeros on both sides.
    starts = None is all zeros (tests/unpad_ref.py's unpack_rows)."""
    packed = np.asarray(packed)
    st = np.zeros(B, np.int64) if starts is None else np.clip(np.asarray(starts, dtype=np.int64), 0, T)
    out = np.zeros((B, T) + packed.shape[1:], packed.dtype)
    for b in range(B):
        for t in range(T):
            k = t - int(st[b])
            if 0 <= k < int(off[b + 1]) - int(off[b]) and int(off[b]) + k < len(packed):
                out[b, t] = packed[int(off[b]) + k]
    return out


def spans_for(B, T, seed):
    """Test spans: lens in 1 .. T, starts drawn from {0, T - len, the middle}."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    kind = rng.integers(0, 3, B)
    starts = np.where(kind == 0, 0, np.where(kind == 1, T - lens, (T - lens) // 2))
    return starts.astype(np.int64), lens.astype(np.int64)
