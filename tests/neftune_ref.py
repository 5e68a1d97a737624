"""numpy restatement of NEFTune's noise (slam_set_neftune, include/slam_engine.h) on top of tests/dropout_ref.r16: the scale of
one noise level, the noise of an [M, H] launch and the two embedding forms with their one bf16 rounding. np.float32 multiply
and add round once each, to nearest: they reproduce the kernel's two uncontracted operations exactly.
Shared by tests/test_neftune_host.py (HF's magnitude, moments, structure) and tests/test_gpu_neftune.py (the kernels and the
model against it)."""
import math

import numpy as np

from tests.dropout_ref import r16

SITE = 0x4E454654  # the last counter word: no dropout site (2 * layer + site) reaches it


def scale(alpha, T, H):
    """s: the noise of one level, (float)((double)alpha / sqrt((double)T * H) / 65536.0). alpha as the engine holds it (fp32)."""
    return np.float32(float(np.float32(alpha)) / math.sqrt(float(T) * float(H)) / 65536.0)


def levels(M, H, seed, call, index0=0):
    """int64 [M, H]: t = 2 r16 - 65535 of the element with flat index index0 + m * H + h (odd, in [-65535, 65535])."""
    idx = np.arange(M * H, dtype=np.int64) + int(index0)
    return (2 * r16(seed, call, SITE, idx).astype(np.int64) - 65535).reshape(M, H)


def noise(M, H, s, seed, call, index0=0):
    """fp32 [M, H]: n = t * s, one fp32 multiply (t is exact in fp32)."""
    return levels(M, H, seed, call, index0).astype(np.float32) * np.float32(s)


def bf16_bits(x):
    """uint16 bits of fp32 values rounded to bf16, to nearest-even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rows(ids, V):
    """Table rows the gather reads: ids outside [0, V) read row 0."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.where((ids < 0) | (ids >= V), 0, ids)


def pos_rows(M, T, NP, position_ids=None):
    """Position-table rows of the OPT form: position_ids[m] or m % T, plus 2, clamped to the table."""
    p = (np.arange(M, dtype=np.int64) % int(T)) if position_ids is None else np.asarray(position_ids, dtype=np.int64)
    return np.clip(p + 2, 0, NP - 1)


def embed(ids, E, s, seed, call, index0=0, P=None, T=1, position_ids=None):
    """uint16 bf16 bits [M, H] of the armed embedding launch. E [V, H] and P [NP, H]: fp32 arrays of bf16-representable values.
    Without P: bf16(e + n). With P (OPT): bf16((E + P) + n), the two fp32 adds in this order."""
    E = np.asarray(E, dtype=np.float32)
    M, H = len(ids), E.shape[1]
    v = E[rows(ids, E.shape[0])]
    if P is not None:
        P = np.asarray(P, dtype=np.float32)
        v = v + P[pos_rows(M, T, P.shape[0], position_ids)]
    return bf16_bits(v + noise(M, H, s, seed, call, index0))
