"""numpy restatement of the pack rule of padding-free execution (slam_forward_unpadded, include/slam_engine.h): a right-padded
[B, T] batch with row lengths `lens` becomes one flattened row of M_packed tokens - B segments and one dummy tail segment.
Shared by tests/test_padding_free_host.py (the rule itself) and tests/test_gpu_padding_free.py (the pack kernel, bit for bit).
`python -m pytest tests/unpad_ref.py` runs the unit test at the bottom."""
import numpy as np


def m_packed(lens):
    """The host's choice of M_packed: sum(lens) rounded up to a multiple of 64."""
    return -(-int(np.sum(lens)) // 64) * 64


def pack(ids, labels, lens, Mp=None, pad_id=0):
    """The arrays the pack kernel writes for m' in [0, Mp): dict of ids, labels (None without labels), position_ids (int64),
    seg_start, seg_end, row (int32) and off (int32 [B + 1], the exclusive prefix sum of lens).
    Token (b, t), t < lens[b], goes to m' = off[b] + t; labels'[m'] = -100 at t == 0 (the loss targets labels'[m' + 1]); the tail
    [off[B], Mp) is one segment of pad ids with labels -100, positions from 0 and row -1."""
    ids = np.asarray(ids, dtype=np.int64)
    B, T = ids.shape
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.shape == (B,) and lens.min() >= 1 and lens.max() <= T
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(off[-1])
    Mp = m_packed(lens) if Mp is None else int(Mp)
    assert Mp % 64 == 0 and S <= Mp <= -(-(B * T) // 64) * 64
    out = dict(ids=np.full(Mp, max(int(pad_id), 0), np.int64), labels=None, position_ids=np.zeros(Mp, np.int64),
               seg_start=np.full(Mp, S, np.int32), seg_end=np.full(Mp, Mp, np.int32), row=np.full(Mp, -1, np.int32),
               off=off.astype(np.int32))
    if labels is not None:
        labels = np.asarray(labels, dtype=np.int64)
        out["labels"] = np.full(Mp, -100, np.int64)
    out["position_ids"][S:] = np.arange(Mp - S)
    for b in range(B):
        n, o = int(lens[b]), int(off[b])
        out["ids"][o:o + n] = ids[b, :n]
        if labels is not None:
            out["labels"][o:o + n] = labels[b, :n]
            out["labels"][o] = -100
        out["position_ids"][o:o + n] = np.arange(n)
        out["seg_start"][o:o + n] = o
        out["seg_end"][o:o + n] = o + n
        out["row"][o:o + n] = b
    return out


def unpack_rows(packed, off, B, T):
    """Per-position values back in the batch's layout: out[b, t] = packed[off[b] + t] for t < lens[b], zeros at the pads."""
    packed = np.asarray(packed)
    out = np.zeros((B, T) + packed.shape[1:], packed.dtype)
    for b in range(B):
        n = int(off[b + 1] - off[b])
        out[b, :n] = packed[off[b]:off[b] + n]
    return out


def test_pack_rule():
    ids = np.arange(1, 1 + 3 * 64).reshape(3, 64)
    lab = ids + 1000
    p = pack(ids, lab, [64, 1, 37])
    assert p["ids"].shape == (128,) and p["off"].tolist() == [0, 64, 65, 102]
    assert p["ids"][:64].tolist() == ids[0].tolist() and p["ids"][64] == ids[1, 0] and p["ids"][65:102].tolist() == ids[2, :37].tolist()
    assert p["labels"][0] == -100 and p["labels"][1:64].tolist() == lab[0, 1:].tolist()
    assert p["labels"][64] == -100 and p["labels"][65] == -100 and p["labels"][66] == lab[2, 1]
    assert p["position_ids"][63:67].tolist() == [63, 0, 0, 1]
    assert p["seg_start"][64] == 64 and p["seg_end"][64] == 65 and p["row"][64] == 1
    # the tail: 26 pad tokens, one segment, positions from 0
    assert (p["ids"][102:] == 0).all() and (p["labels"][102:] == -100).all() and (p["row"][102:] == -1).all()
    assert p["position_ids"][102:].tolist() == list(range(26))
    assert (p["seg_start"][102:] == 102).all() and (p["seg_end"][102:] == 128).all()
    # every real token's segment is its row's; a target never crosses a row: the label behind a row's last token is -100
    for b in range(3):
        assert p["labels"][p["off"][b]] == -100
    # round trip
    assert (unpack_rows(p["ids"], p["off"], 3, 64)[0] == ids[0]).all()
    assert (unpack_rows(p["ids"], p["off"], 3, 64)[1, 1:] == 0).all()
    # full rows: no tail
    q = pack(ids[:2], None, [64, 64])
    assert q["labels"] is None and q["ids"].tolist() == ids[:2].reshape(-1).tolist() and (q["row"] >= 0).all()
