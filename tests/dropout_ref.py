"""numpy restatement of the residual-dropout mask (engine option "dropout_thr16", include/slam_engine.h) on top of
tests/sr_ref.philox4x32_10: threshold and scale of a probability, the keep mask of one site, and the two kernels' arithmetic.
Shared by tests/test_dropout_host.py (drop rate, known structure) and tests/test_gpu_dropout.py (the kernels and the model
against it)."""
import numpy as np

from tests.sr_ref import MASK, philox4x32_10


def thr16(p):
    """round(p * 65536): the 16-bit threshold of a drop probability."""
    return int(round(float(p) * 65536.0))


def scale(thr):
    """1 / (1 - q), q = thr / 65536, in fp32 (q and 1 - q are exact there: one rounding, the division's)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(thr) / np.float32(65536.0))


def r16(seed, call, stream, index):
    """The 16 random bits of the elements at flat indices `index` (int64 array) of site stream = 2 * layer + site."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index = np.asarray(index, dtype=np.uint64)
    i8 = index >> np.uint64(3)
    w = philox4x32_10((i8 & MASK, i8 >> np.uint64(32), np.full_like(i8, int(call)), np.full_like(i8, int(stream))),
                      (seed & MASK, seed >> 32))
    j = (index & np.uint64(7)).astype(np.int64)
    words = np.stack(w, axis=0)
    word = np.take_along_axis(words, (j >> 1)[None, :], axis=0)[0]
    return ((word >> (16 * (j & 1)).astype(np.uint64)) & np.uint64(0xFFFF)).astype(np.uint32)


def keep_mask(M, H, thr, seed, call, stream, index0=0):
    """bool [M, H]: True where element (m, n) - flat index index0 + m * H + n - is KEPT (r16 >= thr)."""
    idx = np.arange(M * H, dtype=np.int64) + int(index0)
    return (r16(seed, call, stream, idx) >= np.uint32(thr)).reshape(M, H)


def dropout_add_f32(y, resid, keep, thr):
    """fp32 value of the forward before its one rounding to bf16: resid + (keep ? y * scale : 0)."""
    y = np.asarray(y, dtype=np.float32)
    resid = np.asarray(resid, dtype=np.float32)
    return np.where(keep, resid + y * scale(thr), resid).astype(np.float32)


def dropout_bwd_f32(dy, keep, thr):
    """fp32 value of the backward before its rounding: keep ? dy * scale : 0."""
    dy = np.asarray(dy, dtype=np.float32)
    return np.where(keep, dy * scale(thr), np.float32(0.0)).astype(np.float32)
