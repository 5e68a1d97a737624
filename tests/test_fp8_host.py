"""CPU tier of the FP8 decode weights (slam_quantize_decode_w8, UnitLM.quantize_decode_weights): the restatement tests/fp8_ref.py
against torch.float8_e4m3fn where rounding can go wrong (every tie point between adjacent codes, one bf16 ulp either side, the
subnormal range, +-0), the exponent rule at its thresholds and clamps, Wdq exact in bf16, the private code order a bijection
of every 64-deep block, the new symbols declared / exported / bound, and every refusal that needs no device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import fp8_ref as R

NEW = ["slam_decode_w8_bytes", "slam_bind_decode_w8", "slam_quantize_decode_w8", "slam_decode_w8_state", "slam_decode_w8_launches",
       "slam_op_w8_bytes", "slam_op_w8_exps_offset", "slam_op_quantize_rows_fp8", "slam_op_dequantize_rows_fp8",
       "slam_op_gemm_skinny_w8"]
TINY = (2, 128, 2, 1, 64, 256, 502, 0, 1e-6, 10000.0)
E_INVAL, E_STATE, E_NOMEM = -1, -2, -3


def _torch_codes(x32: np.ndarray) -> np.ndarray:
    return torch.from_numpy(x32.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _bf16_neighbours(v: np.ndarray) -> np.ndarray:
    """v (exact in bf16, positive) and the bf16 values one ulp below and above it."""
    b = R.bf16_bits(torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16))
    assert np.array_equal(R.bits_to_bf16(b).float().numpy().astype(np.float64), v)  # the tie points ARE bf16 values
    return np.concatenate([R.bits_to_bf16(b + d).float().numpy().astype(np.float64) for d in (-1, 0, 1)])


def test_code_table():
    v = R.e4m3_value(np.arange(256))
    assert np.isnan(v[0x7F]) and np.isnan(v[0xFF]) and np.isfinite(np.delete(v, [0x7F, 0xFF])).all()
    assert v[0x7E] == 448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0x38] == 1.0 and v[0xB8] == -1.0
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.array_equal(np.delete(v, [0x7F, 0xFF]), np.delete(ref, [0x7F, 0xFF]))
    assert np.array_equal(np.signbit(v[0x80:0xFF]), np.ones(127, bool)) and np.signbit(v[0x80]) and v[0x80] == 0.0


def test_encode_agrees_with_torch_at_every_tie_and_next_to_it():
    g = R.e4m3_value(np.arange(0x7F))
    ties = (g[:-1] + g[1:]) / 2
    pts = np.concatenate([_bf16_neighbours(ties), g])
    pts = pts[pts <= 448.0]
    for x in (pts, -pts):
        assert np.array_equal(R.e4m3_encode(x), _torch_codes(x))
    # a tie goes to the even code
    c = R.e4m3_encode(ties)
    assert np.all(c % 2 == 0) and np.all(np.abs(R.e4m3_value(c) - ties) == np.diff(g) / 2)


def test_encode_subnormal_range_and_zeros():
    sub = np.arange(0, 2 ** 7 + 1) * 2.0 ** -13  # 0 .. 2^-6 in steps of a sixteenth of the subnormal spacing
    for x in (sub, -sub):
        assert np.array_equal(R.e4m3_encode(x), _torch_codes(x))
    assert R.e4m3_encode(np.array([0.0, -0.0])).tolist() == [0x00, 0x80]
    assert R.e4m3_encode(np.array([2.0 ** -10, -2.0 ** -10, 2.0 ** -40, -2.0 ** -40])).tolist() == [0x00, 0x80, 0x00, 0x80]
    assert R.e4m3_encode(np.array([3 * 2.0 ** -10, 448.0, -448.0])).tolist() == [0x02, 0x7E, 0xFE]


def _bf(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.bfloat16)


@pytest.mark.parametrize("e", [-20, 0, 5])
def test_exponent_rule_at_the_threshold(e):
    at = _bf([448.0 * 2.0 ** e])
    assert float(at[0]) == 448.0 * 2.0 ** e
    above = R.bits_to_bf16(R.bf16_bits(at) + 1)
    below = R.bits_to_bf16(R.bf16_bits(at) - 1)
    assert R.row_exponent(R.bf16_bits(at)).tolist() == [e]
    assert R.row_exponent(R.bf16_bits(above)).tolist() == [e + 1]
    assert R.row_exponent(R.bf16_bits(below)).tolist() == [e]
    assert R.row_exponent(R.bf16_bits(_bf([256.0 * 2.0 ** e]))).tolist() == [e]           # f = 1.0 of the same binade
    assert R.row_exponent(R.bf16_bits(_bf([255.0 * 2.0 ** e]))).tolist() == [e]           # f just below 2 of the one before
    assert R.row_exponent(R.bf16_bits(_bf([224.0 * 2.0 ** e]))).tolist() == [e - 1]       # 1.75 * 2^7 = 448 * 2^(e-1)
    # the definition: the smallest integer with amax <= 448 * 2^e, over a sweep of bit patterns
    bits = np.arange(1, 0x7F80, 1237)
    amax = R.bits_to_bf16(bits).double().numpy()
    exact = [min(max(next(k for k in range(-160, 130) if a <= 448.0 * 2.0 ** k), R.EXP_MIN), R.EXP_MAX) for a in amax]
    assert R.row_exponent(bits).tolist() == exact


def test_zero_row_and_both_clamps():
    W = torch.zeros(4, 64, dtype=torch.bfloat16)
    W[0, 3] = -0.0
    W[1, 5] = 2.0 ** -120          # e would be -128: clamped to -100, the value is below the grid and rounds to zero
    W[1, 6] = -2.0 ** -125
    W[2, 0] = 2.0 ** -133          # a bf16 subnormal
    W[3, 7] = 1.875 * 2.0 ** 127   # e = 120, the largest any finite bf16 needs: the upper clamp is never active
    W[3, 8] = -2.0 ** 111          # 2^-9 * 2^120: the smallest subnormal code
    codes, e, Wdq = R.quantize(W)
    assert e.tolist() == [0, R.EXP_MIN, R.EXP_MIN, R.EXP_MAX]
    assert codes[0, 3] == 0x80 and codes[0].astype(int).sum() == 0x80
    assert codes[1, 5] == 0x00 and codes[1, 6] == 0x80 and codes[2, 0] == 0x00
    assert codes[3, 7] == R.e4m3_encode(np.array([240.0]))[0] and codes[3, 8] == 0x81
    assert torch.equal(Wdq[3], W[3]) and float(Wdq[3, 7]) == 1.875 * 2.0 ** 127
    assert R.bf16_bits(Wdq[0])[3] == 0x8000 and R.bf16_bits(Wdq[1])[6] == 0x8000
    assert R.row_exponent(np.array([0x7F7F])).tolist() == [R.EXP_MAX]  # the largest finite bf16


def test_wdq_is_exact_in_bf16():
    # every finite code under a spread of exponents: the fp32 product has nothing below its high 16 bits
    codes = np.delete(np.arange(256), [0x7F, 0xFF]).astype(np.uint8)
    for e in (-100, -37, -1, 0, 9, 119):
        v = R.e4m3_value(codes) * 2.0 ** e
        v32 = v.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), v) and np.all((v32.view(np.uint32) & 0xFFFF) == 0)
        assert np.array_equal(R.dequantize(codes[None], np.array([e])).double().numpy()[0], v)
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(33, 192, generator=g) * 0.02).to(torch.bfloat16)
    codes, e, Wdq = R.quantize(W)
    assert not np.isin(codes, (0x7F, 0xFF)).any()
    x = W.double().numpy() * 2.0 ** -e.astype(np.float64)[:, None]
    assert np.abs(x).max(axis=1).max() <= 448.0 and np.abs(x).max(axis=1).min() > 224.0  # the smallest e that fits
    assert np.array_equal(codes, _torch_codes(x))
    assert np.array_equal(Wdq.double().numpy(), R.e4m3_value(codes) * 2.0 ** e.astype(np.float64)[:, None])
    # a quantised matrix is a fixed point (a row whose amax was rounded down may take the next exponent down: same values)
    c2, e2, W2 = R.quantize(Wdq)
    assert torch.equal(W2, Wdq) and np.all((e2 == e) | (e2 == e - 1))
    rel = float(((Wdq.double() - W.double()).square().sum() / W.double().square().sum()).sqrt())
    assert 0.015 < rel < 0.04  # three mantissa bits: 2^-4 / sqrt(3) = 3.6 % at the worst spot of a binade, 1.8 % at the best


def test_code_order_is_a_bijection_of_every_block():
    k = np.arange(256)
    p = R.code_pos(k)
    assert sorted(p.tolist()) == k.tolist() and np.array_equal(p // 64, k // 64)
    for q in range(4):  # a lane quarter's 16 bytes: its 8 columns of the first step, then its 8 of the second
        assert p[8 * q:8 * q + 8].tolist() == list(range(16 * q, 16 * q + 8))
        assert p[32 + 8 * q:32 + 8 * q + 8].tolist() == list(range(16 * q + 8, 16 * q + 16))


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    for n in ("decode_w8_bytes", "bind_decode_w8", "quantize_decode_w8", "decode_w8_state", "decode_w8_launches"):
        assert hasattr(E.Engine, n), n


def test_op_sizes_and_refusals_before_a_launch():
    lib = E.load_library()
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for N, K in ((70, 64), (70, 192), (1, 64), (37888, 3584)):
        assert lib.slam_op_w8_exps_offset(N, K) == al(N * K)
        assert lib.slam_op_w8_bytes(N, K) == al(N * K) + al(N)
    for N, K in ((0, 64), (-1, 64), (4, 0), (4, 32), (4, 96), (4, 72)):
        assert lib.slam_op_w8_bytes(N, K) == 0 and lib.slam_op_w8_exps_offset(N, K) == 0
    fake = C.c_void_p(1 << 20)
    odd = C.c_void_p((1 << 20) + 8)
    for kw in (dict(W=None), dict(q=None), dict(e=None), dict(N=0), dict(K=0), dict(K=32), dict(K=72), dict(W=odd), dict(q=odd)):
        a = dict(W=fake, q=fake, e=fake, N=70, K=64)
        a.update(kw)
        assert lib.slam_op_quantize_rows_fp8(a["W"], a["q"], a["e"], a["N"], a["K"], None) == E_INVAL, kw
        assert lib.slam_op_dequantize_rows_fp8(a["q"], a["e"], a["W"], a["N"], a["K"], None) == E_INVAL, kw
    for kw in (dict(e=None), dict(M=0), dict(N=0), dict(K=0), dict(K=32), dict(K=200), dict(X=odd), dict(q=odd), dict(Y=None)):
        a = dict(X=fake, q=fake, e=fake, Y=fake, M=4, N=70, K=64)
        a.update(kw)
        assert lib.slam_op_gemm_skinny_w8(a["X"], a["q"], a["e"], a["Y"], 1, None, None, a["M"], a["N"], a["K"], None, 0, None) == E_INVAL, kw


def test_engine_refusals_without_a_device():
    lib = E.load_library()
    fake = C.c_void_p(1 << 20)
    eng = E.Engine(E.SlamModelDesc(*TINY))
    L, H, QKV, HD, I, V = 2, 128, 256, 128, 256, 502
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    per = lambda N, K: al(N * K) + al(N)  # noqa: E731
    body = L * (per(QKV, H) + per(H, HD) + per(2 * I, H) + per(H, I))
    assert eng.decode_w8_bytes(False) == body and eng.decode_w8_bytes(True) == body + per(V, H)
    assert eng.decode_w8_state() == 0 and eng.decode_w8_launches() == 0
    assert lib.slam_quantize_decode_w8(eng.h, None) == E_STATE                       # no parameters
    assert lib.slam_bind_params(eng.h, fake, None) == 0
    assert lib.slam_quantize_decode_w8(eng.h, None) == E_STATE                       # no codes bound
    assert b"slam_bind_decode_w8" in lib.slam_last_error(eng.h)
    assert lib.slam_bind_decode_w8(eng.h, C.c_void_p((1 << 20) + 64), body, 0) == E_INVAL
    assert lib.slam_bind_decode_w8(eng.h, fake, body - 1, 0) == E_NOMEM
    assert lib.slam_bind_decode_w8(eng.h, fake, body, 1) == E_NOMEM
    assert eng.decode_w8_state() == 0
    assert lib.slam_bind_decode_w8(eng.h, fake, body, 0) == 0 and eng.decode_w8_state() == 1
    assert lib.slam_bind_params(eng.h, fake, None) == 0 and eng.decode_w8_state() == 1
    assert lib.slam_bind_decode_w8(eng.h, None, 0, 0) == 0 and eng.decode_w8_state() == 0
    for f in (lib.slam_decode_w8_state, lib.slam_decode_w8_launches):
        assert f(None) == 0
    assert lib.slam_decode_w8_bytes(None, 0) == 0
    assert lib.slam_bind_decode_w8(None, fake, body, 0) == E_INVAL and lib.slam_quantize_decode_w8(None, None) == E_INVAL
    eng.close()
    # OPT has no decode path; a body with a K that is no multiple of 64 is refused with a message and stays unbound
    opt = E.Engine(E.SlamModelDesc(2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0), arch=1, n_positions=64)
    assert opt.decode_w8_bytes(False) == 0
    assert lib.slam_bind_decode_w8(opt.h, fake, 1 << 30, 0) == E_INVAL and b"OPT" in lib.slam_last_error(opt.h)
    assert opt.decode_w8_state() == 0
    opt.close()
    odd = E.Engine(E.SlamModelDesc(2, 128, 2, 1, 64, 160, 502, 0, 1e-6, 10000.0))  # intermediate 160 = 5 * 32
    assert odd.decode_w8_bytes(False) == 0
    assert lib.slam_bind_decode_w8(odd.h, fake, 1 << 30, 0) == E_INVAL and b"multiples of 64" in lib.slam_last_error(odd.h)
    assert odd.decode_w8_state() == 0
    odd.close()


def _bare():
    from slamkit_amd.model.unit_lm import UnitLM
    return UnitLM.__new__(UnitLM)  # host-only: the arguments are checked before the model is touched


def test_python_argument_errors():
    m = _bare()
    m.config = types.SimpleNamespace(is_opt=True)
    with pytest.raises(ValueError, match="OPT"):
        m.quantize_decode_weights()
    m.config = types.SimpleNamespace(is_opt=False)
    for bad in ("int8", "fp8", "fp8_e5m2", None):
        with pytest.raises(ValueError, match="dtype"):
            m.quantize_decode_weights(dtype=bad)
    m.engine = E.Engine(E.SlamModelDesc(2, 128, 2, 1, 64, 160, 502, 0, 1e-6, 10000.0))
    with pytest.raises(ValueError, match="multiples of 64"):
        m.quantize_decode_weights()
    assert m.decode_weights is None
    m.engine.close()
