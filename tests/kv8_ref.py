"""The FP8 KV cache format of include/slam_engine.h (SLAM_KV_FP8_E4M3) restated on the CPU. A key or value vector - hd bf16
elements of one (layer, K | V, row, kv head, position) - is a weight row of tests/fp8_ref.py, word for word: the exponent from
the bf16 bits of its amax (0 for an all-zero vector), e4m3 codes of x 2^-e (round to nearest even), value(code) 2^e exact in
bf16. Codes keep the dim order. Buffer: all codes [L][2][bmax][nKV][cap][hd] bytes, then all exponents [L][2][bmax][nKV][cap]."""
import numpy as np
import torch

from tests import fp8_ref as F


def quantize(x: torch.Tensor):
    """x bf16 [..., hd] -> codes uint8 [..., hd], exponents int8 [...] (numpy)."""
    codes, e, _ = F.quantize(x.reshape(-1, x.shape[-1]).contiguous())
    return codes.reshape(tuple(x.shape)), e.reshape(tuple(x.shape[:-1]))


def dequantize(codes, exps) -> torch.Tensor:
    """value(code) 2^e as bf16, the shape of codes."""
    codes, exps = np.asarray(codes), np.asarray(exps)
    return F.dequantize(codes.reshape(-1, codes.shape[-1]), exps.reshape(-1)).view(*codes.shape)


def cache_bytes(L, bmax, nKV, cap, hd, fp8=True):
    return L * 2 * bmax * nKV * cap * (hd + 1 if fp8 else 2 * hd)


def split(buf, L, bmax, nKV, cap, hd):
    """A bound FP8 cache (uint8, cache_bytes long) -> codes [L][2][bmax][nKV][cap][hd] uint8, exponents [L][2][bmax][nKV][cap] int8."""
    b = np.asarray(buf.cpu()) if isinstance(buf, torch.Tensor) else np.asarray(buf)
    n = L * 2 * bmax * nKV * cap
    return b[:n * hd].reshape(L, 2, bmax, nKV, cap, hd), b[n * hd:n * (hd + 1)].view(np.int8).reshape(L, 2, bmax, nKV, cap)
