"""numpy restatement of the optimizer's stochastic rounding ("adamw_sr", include/slam_engine.h): Philox4x32-10, the mapping
from (seed, step, flat index, array) to an element's 16 random bits, and the rounding itself. Shared by tests/test_sr_host.py
(known answers) and tests/test_gpu_sr.py (the kernels against it, bit for bit)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two; returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & MASK for x in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def sr_bits(seed, step, index, which):
    """The 16 random bits of the elements at flat-buffer indices `index` (int64 array) of array `which` (0 p, 1 m, 2 v)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index = np.asarray(index, dtype=np.uint64)
    i8 = index >> 3
    w = philox4x32_10((i8 & MASK, i8 >> 32, np.full_like(i8, int(step)), np.full_like(i8, int(which))),
                      (seed & MASK, seed >> 32))
    j = (index & 7).astype(np.int64)
    words = np.stack(w, axis=0)                            # [4, n]
    word = np.take_along_axis(words, (j >> 1)[None, :], axis=0)[0]
    return ((word >> (16 * (j & 1)).astype(np.uint64)) & 0xFFFF).astype(np.uint32)


def rtn_bf16_bits(x):
    """Round-to-nearest-even bf16 bits of the fp32 array x (torch's conversion)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def sr_bf16(x, r16):
    """bf16 bits (uint16) of the stochastic rounding of the fp32 array x with the random bits r16: finite values add the bits
    below the kept mantissa and truncate, inf / NaN take the round-to-nearest conversion."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    out = ((u.astype(np.uint64) + r16.astype(np.uint64)) >> 16).astype(np.uint16)
    special = (u & 0x7F800000) == 0x7F800000
    return np.where(special, rtn_bf16_bits(x), out)


def sr_round(x, seed, step, index0, which):
    n = np.asarray(x).size
    return sr_bf16(x, sr_bits(seed, step, np.arange(n, dtype=np.int64) + int(index0), which))
