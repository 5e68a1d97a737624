"""CPU tier of the exact GEMM parity tests: the evidence that tests/test_gpu_gemm_exact.py would fail where a kernel is
subtly wrong, and that its input generator and its buffers keep their promises. No GPU, no library call."""
import pytest
import torch

from tests import gemm_exact_ref as R
from tests.gpu_util import check, rnd


# ------------------------------------------------------------------------------------- the generator keeps its promises
@pytest.mark.parametrize("K", [8, 72, 896, 4864, 9728])
def test_integer_operands_sum_exactly_in_any_order(K):
    """fp32 sums of the +-1 products equal the fp64 product bit for bit whatever the order (split at K / 2; 64-wide chunks
    taken from the back), and stay inside the range where a bf16 output is exact, at the density pick_density chooses."""
    d = R.pick_density(K)
    A, B = R.sparse_pm1(384, K, d, seed=11), R.sparse_pm1(512, K, d, seed=12)
    assert set(A.unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(A, A.to(torch.bfloat16).float())
    if K >= 896:  # the density is what was asked for (384 K samples: four sigma is below 0.01 here)
        assert abs(float((A != 0).float().mean()) - d) < 0.01
    ref = A.double() @ B.double().t()
    R.assert_bf16_exact_range(f"K={K} density={d}", ref)
    R.assert_f32_exact_range(f"K={K}", ref)
    h = (K // 2 + 7) // 8 * 8
    halves = A[:, :h] @ B[:, :h].t()
    halves = halves + A[:, h:] @ B[:, h:].t()
    back = torch.zeros(384, 512)
    for k0 in reversed(range(0, K, 64)):
        back += A[:, k0:k0 + 64] @ B[:, k0:k0 + 64].t()
    for name, got in (("split at K/2", halves), ("reversed chunks of 64", back)):
        assert got.dtype == torch.float32
        assert R.first_mismatch(got, ref)[0] == 0, name
        assert R.first_mismatch(got.to(torch.bfloat16), ref)[0] == 0, name  # and the bf16 store loses nothing


def test_small_ints_and_density_rule():
    v = R.small_ints((64, 40), -3, 3, seed=5)
    assert v.dtype == torch.float32 and float(v.min()) == -3 and float(v.max()) == 3 and torch.equal(v, v.round())
    assert torch.equal(v, R.small_ints((64, 40), -3, 3, seed=5))
    assert R.small_ints(24, 0, 1, seed=1).shape == (24,)
    assert [R.pick_density(k) for k in (8, 896, 4864, 4872, 9728)] == [0.5, 0.5, 0.5, 0.25, 0.25]


def test_bf16_ulp():
    x = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 255.0, 256.0, 0.3, 2.0 ** -126, 2.0 ** -130], dtype=torch.float64)
    want = [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 1.0, 2.0, 2.0 ** -9, 2.0 ** -133, 2.0 ** -133]
    assert R.bf16_ulp(x).tolist() == want
    # a value rounded to bf16 is within half an ulp; one more ulp away is over the bar
    ref = torch.linspace(-7, 9, 1001, dtype=torch.float64)
    got = ref.to(torch.bfloat16)
    n, worst, _, ulps = R.elementwise_excess(got, ref, 0.0)
    assert n == 0 and worst <= 0.5 and ulps <= 0.5
    off = (got.double() + 1.6 * R.bf16_ulp(ref)).to(torch.bfloat16)
    assert R.elementwise_excess(off, ref, 0.0)[0] > 900
    assert R.elementwise_excess(torch.full((4,), float("nan")), torch.zeros(4, dtype=torch.float64), 1.0)[0] == 4


# ------------------------------------------------------------------------------------------------ sensitivity, on data only
M, N, K = 1000, 1152, 896          # a test_gemm_nt shape: 8 x 9 tiles, the last row tile ragged
R0, C0, K0 = 3 * 128 + 32, 5 * 128, 40 * 8   # a 16-row fragment of tile (3, 5); the 8-element K-chunk 40


def _drop_chunk(out, X, W, rows, cols):
    """The result when rows [R0, R0 + rows) x columns [C0, C0 + cols) lose the K-chunk [K0, K0 + 8) of their contraction."""
    out = out.clone()
    out[R0:R0 + rows, C0:C0 + cols] -= X[R0:R0 + rows, K0:K0 + 8].double() @ W[C0:C0 + cols, K0:K0 + 8].double().t()
    return out


def _shift_bias(out, bias, rows, cols):
    """The result when rows [R0, R0 + rows) x columns [C0, C0 + cols) got the bias of the column group 8 further on."""
    out = out.clone()
    out[R0:R0 + rows, C0:C0 + cols] += (bias[C0 + 8:C0 + 8 + cols] - bias[C0:C0 + cols]).double()
    return out


def _check_misses(name, got64, ref64):
    """True when tests.gpu_util.check at test_gemm_nt's bars (4e-3 rel-RMS, 2e-2 of the abs-max) accepts `got`."""
    try:
        check(name, got64.to(torch.bfloat16).float(), ref64.float(), 4e-3, 2e-2)
        return True
    except AssertionError:
        return False


def test_exact_comparison_catches_what_the_aggregate_bars_miss():
    """Two defects a tile kernel can have, applied to reference data (no kernel runs): a 16-row fragment of tile (3, 5) that
    loses one 8-element chunk of the K = 896 contraction, and tile (.., 5) adding the bias of the column group 8 further on.

    The exact comparison on integer data flags both, and every smaller version of them down to ONE lane's 8-column store in
    ONE row, naming row, column and tile.

    What the existing bars do with the same defects on test_gemm_nt's Gaussian inputs was measured, and they are less blind
    than was assumed when these tests were planned: check()'s max-abs bar (2e-2 of the abs-max, about 0.17 .. 0.2 here) DOES catch
    the full-size defects - the lost chunk over 16 rows x 128 columns leaves a worst element 0.55 off (a 3-sigma x against a
    3-sigma w), the shifted bias is off by O(1) in every element. The smallest versions it misses, asserted below:
      * the lost K-chunk confined to one row x 8 columns (one lane's 16-byte store; still caught at one row x 128 columns);
      * the shifted bias confined to a single element whose two bias values happen to lie within the bar (0.2) of each other;
        one row x 8 columns is still caught.
    So the aggregate bars are blind to per-lane defects and, by construction, to any error below 2 % of the tensor's largest
    value - which is every wrong addend among the 896 of an output. The exact tests have no such floor."""
    # integer data: what test_gpu_gemm_exact.py feeds the kernels
    d = R.pick_density(K)
    Xi, Wi = R.sparse_pm1(M, K, d, seed=1), R.sparse_pm1(N, K, d, seed=2)
    bi, ri = R.small_ints(N, -3, 3, seed=3), R.small_ints((M, N), -3, 3, seed=4)
    ref_i = Xi.double() @ Wi.double().t() + bi.double() + ri.double()
    R.assert_bf16_exact_range("sensitivity reference", ref_i)
    assert R.first_mismatch(ref_i.to(torch.bfloat16), ref_i)[0] == 0
    for rows, cols in ((16, 128), (1, 128), (1, 8)):
        n, info = R.first_mismatch(_drop_chunk(ref_i, Xi, Wi, rows, cols).to(torch.bfloat16), ref_i)
        assert n > 0 and info["tile"] == (3, 5) and info["row"] == R0 and C0 <= info["col"] < C0 + cols, (rows, cols, n, info)
        assert info["got"] != info["expected"]
    for rows, cols in ((M - R0, 128), (16, 128), (1, 8)):
        n, info = R.first_mismatch(_shift_bias(ref_i, bi, rows, cols).to(torch.bfloat16), ref_i)
        assert n > 0 and info["tile"] == (3, 5) and info["row"] == R0, (rows, cols, n, info)
    with pytest.raises(AssertionError, match=r"row 416, column 64\d \(128 x 128 tile \(3, 5\)\)"):
        R.assert_exact("dropped chunk", _drop_chunk(ref_i, Xi, Wi, 16, 128).to(torch.bfloat16), ref_i)

    # Gaussian data: what test_gemm_nt feeds them, under its bars
    X, W, bias, res = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05), rnd(N, seed=3), rnd(M, N, seed=4)
    plain = X.double() @ W.double().t()
    full = plain + bias.double() + res.double()
    assert _check_misses("clean", full, full)
    for base in (plain, full):
        assert _check_misses("lost K-chunk, one row x 8 columns", _drop_chunk(base, X, W, 1, 8), base)
    assert abs(float(bias[C0 + 8] - bias[C0])) > 0.05   # the single-element defect is not a no-op
    assert _check_misses("shifted bias, one element", _shift_bias(full, bias, 1, 1), full)
    caught = {"chunk 16x128": not _check_misses("c", _drop_chunk(full, X, W, 16, 128), full),
              "bias 1000x128": not _check_misses("b", _shift_bias(full, bias, M - R0, 128), full)}
    print("[sensitivity] full-size defects caught by check():", caught)


# --------------------------------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("dtype,sentinel", [(torch.bfloat16, 1000.0), (torch.float32, float("nan"))])
def test_guarded_detects_one_element_in_either_band(dtype, sentinel):
    for shape in ((7, 24), (40,), (0,)):
        for where in (0, -1, R.GUARD - 1, -R.GUARD):
            payload, ok = R.guarded(shape, dtype, sentinel)
            assert payload.shape == shape and payload.data_ptr() % 16 == 0
            payload.fill_(3.0)      # a write inside the payload is not the checker's business
            ok("clean")
            band = payload._base[:R.GUARD] if where >= 0 else payload._base[-R.GUARD:]
            band.reshape(-1)[where if where >= 0 else band.numel() + where] = 2.0
            with pytest.raises(AssertionError, match="leading" if where >= 0 else "trailing"):
                ok("touched")


def test_guarded_sentinel_is_compared_as_bits():
    payload, ok = R.guarded((4, 8), torch.float32, 0.0)
    payload._base[0, 0] = -0.0      # equal as a number, not as bits
    with pytest.raises(AssertionError):
        ok("negative zero")


def test_poisoned_operands_read_back_equal():
    t = R.sparse_pm1(37, 24, 0.5, seed=3)
    p = R.poisoned(t)
    assert p.dtype == torch.bfloat16 and p.data_ptr() % 16 == 0
    assert torch.equal(p.float().cpu(), t)
    base = p._base
    assert base.shape[0] == 37 + 2 * R.GUARD and bool(torch.isnan(base[:R.GUARD]).all()) and bool(torch.isnan(base[-R.GUARD:]).all())
    b = R.poisoned(R.small_ints(16, -3, 3, seed=1))
    assert b.shape == (16,) and torch.equal(b.float().cpu(), R.small_ints(16, -3, 3, seed=1))
    # a poisoned element that reaches a product is visible in the exact comparison
    got = (base[R.GUARD - 1:R.GUARD - 1 + 37].float().cpu() @ t.t()).to(torch.bfloat16)
    n, info = R.first_mismatch(got, t.double() @ t.double().t())
    assert n > 0 and info["row"] == 0
