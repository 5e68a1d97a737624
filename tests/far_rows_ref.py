"""Helpers of the far-row parity tests (test_far_rows_host.py, test_gpu_far_rows.py): plain torch, no kernel, any device.

THE BUFFER. The flagship workload keeps logits and d-logits in one bf16 buffer of [tokens][VP = 152,320]: a row is 304,640
bytes, so row ROW_2G = 7,049 holds byte 2^31 and row ROW_4G = 14,098 holds byte 2^32 (which is element 2^31). A kernel that
forms an address on that buffer with a 32-bit byte offset, a signed byte offset or an `int` element index is wrong for every
row from there on. M_FAR = 14,592 = 57 * 256 rows is the smallest multiple of 256 with a whole 256-row tile beyond byte 2^32:
tile 55 (rows 14,080 .. 14,335) straddles it, tile 56 (rows 14,336 .. 14,591) lies beyond it. The buffer is 4.14 GiB.

EXACT GEMM OPERANDS are the ones of tests/gemm_exact_ref.py, values in {-1, 0, +1} drawn here on the device that holds them, in
row chunks (a 2 G element operand never exists as one random tensor). An output element of a contraction of length K over
operands of densities a and b is a sum of K terms that are +-1 with probability a b: variance K a b. DENSITY picks a and b per
contraction so that 256 (the largest magnitude up to which every integer is a bf16 number) is at least 8 standard deviations
away - at the 2e7 outputs of the largest case the chance of one excursion is 2e-8 - and every test still asserts |ref| <= 256
on the reference it compares with: a condition, not a measurement. fp32 outputs (weight gradients) need |ref| < 2^24 only.

REFERENCES never form a tensor of 2 GiB: fp32 torch.matmul over chunks of at most CHUNK = 1,024 rows (exact: integers below
2^24 in any order), summed in float64 where a contraction runs over the chunks.

`where(m)` names a row by its place relative to the two boundaries and by its 128- and 256-row tile; every failure message of
the GPU file carries it with the count and the first differing (row, column, got, expected)."""
import math

import torch

VP, V = 152320, 152167
M_FAR = 14592
ROW_BYTES = 2 * VP
ROW_2G = (1 << 31) // ROW_BYTES
ROW_4G = (1 << 32) // ROW_BYTES
CHUNK = 1024
BF16_EXACT_MAX = 256
F32_EXACT_MAX = 2 ** 24
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

assert (ROW_2G, ROW_4G) == (7049, 14098) and M_FAR == 57 * 256
assert (M_FAR // 256 - 1) * 256 * ROW_BYTES >= 1 << 32 > (M_FAR // 256 - 2) * 256 * ROW_BYTES   # tile 56 beyond, tile 55 straddles
assert ((M_FAR - 256) // 256 - 1) * 256 * ROW_BYTES < 1 << 32                                    # 56 * 256 rows would not do

# (density of the first operand, density of the second) per contraction length
DENSITY = {128: (0.5, 0.5),            # head forward: X [M][128] W [VP][128]
           VP: (1 / 16, 1 / 16),       # head dgrad: dY [M][VP] against W [N][VP] (NT) or W [VP][K] (NN)
           M_FAR: (1 / 16, 0.5)}       # head wgrad: dY [M][VP]^T X [M][K]: fp32 output


def sigma(K):
    a, b = DENSITY[K]
    return math.sqrt(K * a * b)


# ------------------------------------------------------------------------------------------------ where
def row_class(m, row_bytes=ROW_BYTES):
    lo, hi = m * row_bytes, (m + 1) * row_bytes
    for name, edge in (("2^31 B", 1 << 31), ("2^32 B", 1 << 32)):
        if lo <= edge < hi:
            return f"straddles {name}"
    return "before 2 GiB" if hi <= 1 << 31 else "between" if hi <= 1 << 32 else "beyond 4 GiB"


def where(m, row_bytes=ROW_BYTES):
    """Row m of a buffer of row_bytes-long rows: its class and its tiles. row_bytes = None: a small output whose rows are
    not token rows (a weight gradient): the tiles alone."""
    if row_bytes is None:
        return f"row {m} (256-row tile {m // 256}, 128-row tile {m // 128})"
    return f"row {m} ({row_class(m, row_bytes)}; 256-row tile {m // 256}, 128-row tile {m // 128})"


# ------------------------------------------------------------------------------------------------ operands
def fill_pm1(dst, density, seed, row_lo=0):
    """dst [rows][cols] (bf16, any device) <- entries in {-1, 0, +1}, non-zero with probability `density`, drawn in chunks of
    CHUNK rows (chunk i from its own generator: reproducible chunk by chunk); rows below row_lo are +0."""
    rows, cols = dst.shape
    g = torch.Generator(device=dst.device)
    for r0 in range(0, rows, CHUNK):
        r1 = min(rows, r0 + CHUNK)
        g.manual_seed(seed * 100003 + r0)
        u = torch.rand((r1 - r0, cols), generator=g, device=dst.device)
        v = torch.where(u < density / 2, -1.0, 1.0) * (u < density)      # integer-valued; zeros are +0 after the next line
        dst[r0:r1] = (v + 0.0).to(dst.dtype)
    if row_lo > 0:
        dst[:row_lo] = 0.0
    return dst


def small_ints(shape, lo, hi, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=device).float()


# ------------------------------------------------------------------------------------------------ references
def chunks(rows, step=CHUNK):
    return [(r0, min(rows, r0 + step)) for r0 in range(0, rows, step)]


def nt_rows(X, W32t, r0, r1):
    """rows [r0, r1) of X W^T, fp32 (exact for these operands): W32t = W.float().t(), made once by the caller."""
    return (X[r0:r1].float() @ W32t) + 0.0     # + 0.0: -0 of the library product becomes +0, like the kernels' accumulators


def tn_ref(dY, X):
    """dY [M][N]^T X [M][K] in float64, contraction over M in chunks (each chunk's product exact in fp32)."""
    out = torch.zeros(dY.shape[1], X.shape[1], dtype=F64, device=dY.device)
    for r0, r1 in chunks(dY.shape[0]):
        out += (dY[r0:r1].float().t() @ X[r0:r1].float()).double()
    return out + 0.0


def assert_range(name, ref, limit=BF16_EXACT_MAX, strict=False):
    m = float(ref.abs().max())
    assert (m < limit) if strict else (m <= limit), f"{name}: reference abs-max {m} beyond {limit}: operands too dense for an exact output"


# ------------------------------------------------------------------------------------------------ comparison
def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Mismatch:
    """Collects a bit comparison made chunk by chunk: count, first differing element, classes of the rows that differ."""

    def __init__(self, name, row_bytes=ROW_BYTES):
        self.name, self.row_bytes, self.count, self.total, self.first, self.classes = name, row_bytes, 0, 0, None, {}

    def add(self, got, exp, row0=0):
        """got, exp: the same rows [row0, row0 + n) of output and expectation; exp is converted to got's dtype (exact under the
        conditions the tests assert)."""
        assert got.shape == exp.shape, (got.shape, exp.shape)
        e = exp.to(got.dtype)
        bad = bits(got) != bits(e)
        self.total += got.numel()
        n = int(bad.sum())
        if not n:
            return
        self.count += n
        rows = bad.reshape(bad.shape[0], -1).any(1).nonzero()[:, 0]
        if self.row_bytes is not None:
            for r in rows.tolist():
                self.classes.setdefault(row_class(row0 + r, self.row_bytes), row0 + r)
        if self.first is None:
            r = int(rows[0])
            c = int(bad[r].reshape(-1).nonzero()[0])
            self.first = (row0 + r, c, float(got[r].reshape(-1)[c]), float(e[r].reshape(-1)[c]))

    def check(self):
        if self.count:
            m, c, g, e = self.first
            cls = "; differing rows are: " + ", ".join(f"{k} (first row {v})" for k, v in self.classes.items()) if self.classes else ""
            raise AssertionError(f"{self.name}: {self.count} of {self.total} elements differ in bits; first at {where(m, self.row_bytes)}, "
                                 f"column {c}: got {g}, expected {e}{cls}")
