"""The FP8 decode-weight rule of include/slam_engine.h (slam_quantize_decode_w8) restated on the CPU, in numpy on integers and
float64 - no float8 dtype is used to compute anything here (torch.float8_e4m3fn serves the tests as a cross-check only).

Row n of W[N][K] (bf16), amax = max_k |W[n][k]| = f 2^x, 1 <= f < 2:
  e[n] = 0 for a zero row, else the smallest integer with amax <= 448 2^e (x - 8 when f <= 1.75, else x - 7, on the bf16
         bits), clamped to [EXP_MIN, EXP_MAX];
  q[n][k] = the OCP e4m3fn code of W[n][k] 2^-e[n], round to nearest even, the sign of zero kept;
  Wdq[n][k] = value(q[n][k]) 2^e[n]."""
import numpy as np
import torch

EXP_MIN, EXP_MAX = -100, 120
K_GRAIN = 64


def e4m3_value(code):
    """float64 value of every code of an integer array (0x7F / 0xFF: NaN)."""
    c = np.asarray(code).astype(np.int64)
    s, E, M = c >> 7, (c >> 3) & 15, c & 7
    v = np.where(E == 0, M / 8.0 * 2.0 ** -6, (1.0 + M / 8.0) * 2.0 ** (E - 7).astype(np.float64))
    v = np.where((c & 0x7F) == 0x7F, np.nan, v)
    return np.where(s == 1, -v, v)


_GRID = e4m3_value(np.arange(0x7F))  # the 127 non-negative finite values, ascending with the code: 0 .. 448


def e4m3_encode(x):
    """Codes of a float64 array with |x| <= 448: the nearest grid value, ties to the even code (adjacent codes alternate in
    their last mantissa bit), the sign bit copied from x (so -0.0 and every negative value that rounds to zero give 0x80)."""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    assert np.all(a <= 448.0)
    hi = np.clip(np.searchsorted(_GRID, a, side="left"), 0, 0x7E)
    lo = np.maximum(hi - 1, 0)
    dl, dh = a - _GRID[lo], _GRID[hi] - a  # exact: differences of neighbouring binary values
    pick_hi = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    code = np.where(pick_hi, hi, lo)
    return (code | (np.signbit(x).astype(np.int64) << 7)).astype(np.uint8)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF


def bits_to_bf16(bits) -> torch.Tensor:
    return torch.from_numpy(np.asarray(bits).astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def row_exponent(amax_bits):
    """The exponent rule on the 15 magnitude bits of amax, integers only."""
    a = np.asarray(amax_bits).astype(np.int64) & 0x7FFF
    xb, m = a >> 7, a & 0x7F
    e = xb - 127 - np.where(m <= 96, 8, 7)
    e = np.where(xb == 0, EXP_MIN, e)  # bf16 subnormals: x <= -127
    e = np.clip(e, EXP_MIN, EXP_MAX)
    return np.where(a == 0, 0, e).astype(np.int8)


def quantize(W: torch.Tensor):
    """codes uint8 [N][K] in COLUMN order (the engine's in-memory order is private), exponents int8 [N], Wdq bf16 [N][K]."""
    assert W.dtype == torch.bfloat16 and W.dim() == 2
    bits = bf16_bits(W)
    e = row_exponent((bits & 0x7FFF).max(axis=1))
    x = W.double().numpy() * 2.0 ** (-e.astype(np.float64))[:, None]  # exact in float64
    codes = e4m3_encode(x)
    return codes, e, dequantize(codes, e)


def dequantize(codes, e) -> torch.Tensor:
    """value(code) 2^e as the kernels form it: the fp32 product, truncated to its high 16 bits."""
    v = (e4m3_value(codes) * 2.0 ** np.asarray(e).astype(np.float64)[:, None]).astype(np.float32)
    return bits_to_bf16(v.view(np.uint32) >> 16)


def code_pos(k):
    """Byte of a row's code array that holds column k (kernels.h w8_code_pos): inside every 64-deep block, 16 bytes per MFMA
    lane quarter q - its 8 columns 8 q .. of the block's first 32-deep step, then its 8 of the second."""
    k = np.asarray(k)
    return (k & ~63) | (((k >> 3) & 3) << 4) | (((k >> 5) & 1) << 3) | (k & 7)
