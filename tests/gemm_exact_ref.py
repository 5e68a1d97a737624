"""Helpers of the exact GEMM parity tests (test_gemm_exact_host.py, test_gpu_gemm_exact.py). Torch only, no GPU needed.

The idea: with operands in {-1, 0, +1} (and small-integer bias / residual / initial dW) every product and every partial sum
of a contraction is an integer far below 2^24, so fp32 accumulation is exact IN ANY ORDER. Tile shape, MFMA shape, split
plan, slab reduce order and launch form must then all give the same bits, and those bits are known from an fp64 product of
the same operands (torch, on the device: independent library code that knows nothing of the kernels' tiling). A bf16 output
is exact as long as |value| <= 256 (integers up to 256 are bf16 numbers): the tests assert that on the REFERENCE before they
compare - a condition on the inputs, not a tolerance.

Buffers: outputs live between two bands of GUARD sentinel rows (`guarded`), operands between two bands of NaN rows
(`poisoned`): a store outside the payload changes a band, an out-of-range operand element that reaches a stored output
makes it NaN, and the bit comparison reports either."""
import torch

GUARD = 128            # rows of each band (one 128-row tile: a whole ragged tile stored past the end lands in the band)
BF16_EXACT_MAX = 256   # every integer of magnitude <= 256 is a bf16 number
F32_EXACT_MAX = 2 ** 24


def _device(device=None):
    return device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")


def sparse_pm1(rows, cols, density, seed):
    """fp32 [rows][cols] with entries in {-1, 0, +1} (all bf16 numbers), non-zero with probability `density`."""
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(rows, cols, generator=g) < density
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1
    return (keep.to(torch.int64) * sign).float()  # integer product: zeros are +0


def small_ints(shape, lo, hi, seed):
    """fp32 integers in [lo, hi] (bias, residual, initial dW, `act` masks, gate|up pre-activations)."""
    g = torch.Generator().manual_seed(seed)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def pick_density(K):
    """Density of the +-1 operands for a contraction of length K: a sum of K products has variance K density^2, and the
    abs-max over a few million outputs must stay under 256 (profiles/gemm_exact.md has the measured maxima)."""
    return 0.5 if K <= 4864 else 0.25


def bits(t):
    """The tensor's bit patterns as integers (NaN-safe, sign-of-zero-sensitive comparison)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def guarded(shape, dtype, sentinel, device=None):
    """A payload of `shape` between GUARD sentinel rows on either side, all in ONE buffer (a 1-D shape counts elements as
    rows). The payload starts out as the sentinel too. Returns (payload view, check): check(name) raises when an element of
    either band no longer holds the sentinel's bits."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    rows = shape[0]
    buf = torch.full((rows + 2 * GUARD,) + shape[1:], sentinel, dtype=dtype, device=_device(device))
    payload = buf[GUARD:GUARD + rows]
    assert payload.is_contiguous() and payload.data_ptr() % 16 == 0, "guarded payload must stay 16-byte aligned"
    want = int(bits(buf.reshape(-1)[:1])[0])   # the sentinel's bits as this device's fill wrote them

    def check(name="buffer"):
        for band, lo in (("leading", 0), ("trailing", GUARD + rows)):
            bad = (bits(buf[lo:lo + GUARD]).reshape(-1) != want).nonzero()
            if bad.numel():
                i = int(bad[0])
                row_len = max(1, buf[0].numel())
                raise AssertionError(f"{name}: {bad.shape[0]} element(s) of the {band} guard band overwritten, first at band "
                                     f"row {i // row_len}, column {i % row_len}: {buf[lo:lo + GUARD].reshape(-1)[i].item()}")

    return payload, check


def poisoned(t, device=None):
    """bf16 copy of the operand `t` inside a larger buffer whose leading and trailing GUARD rows are NaN; returns the payload
    view (16-byte aligned, keeps the buffer alive)."""
    buf = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), float("nan"), dtype=torch.bfloat16, device=_device(device))
    payload = buf[GUARD:GUARD + t.shape[0]]
    payload.copy_(t.to(torch.bfloat16))
    assert payload.is_contiguous() and payload.data_ptr() % 16 == 0
    return payload


def first_mismatch(got, ref):
    """Bitwise comparison of `got` with the exact expectation `ref` (converted to got's dtype: exact under the bounds the
    tests assert). Returns (count, info): count of differing elements and, for the first one in row-major order, a dict with
    row, col, the 128 x 128 tile coordinates and both values (None when count is 0)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    exp = ref.to(device=got.device, dtype=got.dtype)
    bad = bits(got) != bits(exp)
    count = int(bad.sum())
    if not count:
        return 0, None
    cols = got.shape[-1] if got.dim() > 1 else got.numel()
    i = int(bad.reshape(-1).nonzero()[0])
    r, c = (i // cols, i % cols) if got.dim() > 1 else (0, i)
    return count, {"row": r, "col": c, "tile": (r // 128, c // 128), "got": float(got.reshape(-1)[i]),
                   "expected": float(exp.reshape(-1)[i])}


def assert_exact(name, got, ref):
    count, info = first_mismatch(got, ref)
    assert count == 0, (f"{name}: {count} of {got.numel()} elements differ from the exact result; first at row {info['row']}, "
                        f"column {info['col']} (128 x 128 tile {info['tile']}): got {info['got']}, expected {info['expected']}")


def assert_bf16_exact_range(name, ref):
    """The condition under which a bf16 output has no rounding: an integer reference with |ref| <= 256."""
    m = float(ref.abs().max())
    assert m <= BF16_EXACT_MAX, f"{name}: reference abs-max {m} > {BF16_EXACT_MAX}: the inputs are too dense for an exact bf16 output"
    assert bool((ref == ref.round()).all()), f"{name}: the reference is not integer-valued"


def assert_f32_exact_range(name, ref):
    m = float(ref.abs().max())
    assert m < F32_EXACT_MAX, f"{name}: reference abs-max {m} >= 2^24"
    assert bool((ref == ref.round()).all()), f"{name}: the reference is not integer-valued"


def bf16_ulp(x64):
    """Spacing of the bf16 numbers around each fp64 value (8 significant bits; the denormal spacing 2^-133 below 2^-126)."""
    _, e = torch.frexp(x64.abs().double())  # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    e = torch.where(x64 == 0, torch.full_like(e, -125), torch.clamp(e, min=-125))  # frexp(0) = (0, 0)
    return torch.ldexp(torch.ones_like(x64, dtype=torch.float64), e - 8)


def elementwise_excess(got, ref64, floor):
    """For outputs that pass through silu: every element must lie within one bf16 ulp of the fp64 value (half an ulp is the
    store's rounding, the other half an fp32 evaluation that lands on the other side of a tie) plus the absolute `floor`.
    Returns (count over the bar, worst |error| / bar, flat index of the worst element, worst |error| in ulps)."""
    err = (got.double() - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ulp = bf16_ulp(ref64)
    ratio = err / (ulp + floor)
    worst = int(ratio.reshape(-1).argmax())
    return int((ratio > 1).sum()), float(ratio.reshape(-1)[worst]), worst, float((err / ulp).max())
