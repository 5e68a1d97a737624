"""The 8-bit block-wise Adam moments of include/slam_engine.h ("adamw_state8") in numpy: the tables and the quantiser in fp32 with the
header's own operations (one division, comparisons against the fp32 midpoints, max - all exact to reproduce). The update in
float64 is tests/optim_exact_ref.py's adam_ref from the dequantised state. No GPU is needed."""
import numpy as np

BLOCK, F32 = 256, np.float32


def table(signed):
    """t[k], k = 0 .. 127 (exp_avg) or 0 .. 255 (exp_avg_sq): float64, rounded to fp32 once"""
    K = 127 if signed else 255
    k = np.arange(K + 1, dtype=np.float64)
    return np.where(k == 0, 0.0, 2.0 ** (-(K - k) / 8.0)).astype(F32)


def midpoints(t):
    return (t[:-1] + t[1:]) / F32(2)   # fp32 add, fp32 divide


def layout(n):
    """(bytes of one moment's allocation, byte offset of absmax[], blocks)"""
    blocks = (n + BLOCK - 1) // BLOCK
    return blocks * BLOCK + 4 * blocks, blocks * BLOCK, blocks


def split(alloc, n):
    """a uint8 allocation -> (codes[n], absmax[blocks] as float32, every other byte)"""
    size, off, blocks = layout(n)
    a = np.asarray(alloc, dtype=np.uint8)
    return a[:n], a[off:off + 4 * blocks].view(F32), np.concatenate([a[n:off], a[off + 4 * blocks:]])


def block_max(x):
    return np.abs(np.pad(x, (0, -x.size % BLOCK)).reshape(-1, BLOCK)).max(1)


def quantise(x, signed):
    """fp32 x[n] -> (uint8 codes[n], fp32 absmax[blocks])"""
    x = np.asarray(x, dtype=F32)
    amax = block_max(x)
    scale = np.repeat(amax, BLOCK)[:x.size]
    y = np.divide(np.abs(x), scale, out=np.zeros_like(x), where=scale > 0)   # one fp32 division; none in a zero block
    k = np.searchsorted(midpoints(table(signed)), y, side="left")             # the midpoints below y: a tie goes down
    return (np.where(k > 0, k | (np.signbit(x) * 128), 0) if signed else k).astype(np.uint8), amax


def dequantise(codes, absmax, signed):
    """-> fp32 t[k] * absmax, one fp32 multiply, the sign exact"""
    c = np.asarray(codes).astype(np.int64)
    v = table(signed)[c & 127 if signed else c] * np.repeat(absmax.astype(F32), BLOCK)[:c.size]
    return np.where(c & 128, -v, v).astype(F32) if signed else v
