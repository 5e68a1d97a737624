"""-m gpu: the GEMM family of slamkit_amd/csrc/gemm.hip, kernel by kernel through the C ABI, held to EQUALITY.

Operands are in {-1, 0, +1} with small-integer bias / residual / initial dW (tests/gemm_exact_ref.py): every partial sum is an
integer below 2^24, fp32 accumulation is exact in any order, so every tile shape, MFMA shape, split plan, reduce order and
launch form must store the same bits - the ones of a torch fp64 product of the same operands. Every bf16-output case first
asserts on the reference alone that |ref| <= 256 (no rounding at the store), every fp32 one that |ref| < 2^24.

Every output and the weight-gradient workspace sit between guard bands (the workspace at exactly the byte count the entry
point promises, rounded up to 16), pre-filled with a value no result can take; every operand sits between NaN bands. Options
go through slam_set_option(None, ..) and are put back to GemmTune's defaults (kernels.h) in a finally.

The two outputs that pass through silu (the fused SwiGLU forward's `act`, the rewritten `gu` of its backward) cannot be
exact; they are held ELEMENTWISE: |error| <= one bf16 ulp of the fp64 value (half an ulp for the store's rounding, half for an
fp32 evaluation landing on the other side of a tie) + an absolute floor. The floor is 0 for the forward. For the backward,
whose d(gate) factor 1 + g (1 - sigmoid(g)) cancels, it is measured in the test: twice the worst error of a plain fp32 torch
evaluation of the same formula against fp64 on the same inputs - the yardstick is the reference, never the kernel.
gu [M][2I] has no column the backward leaves alone (include/slam_engine.h: "rewritten in place with d(gate|up)"), so all of it
is compared and only the bands around it are guarded.

Which kernel each shape reaches, and what the runs measured: profiles/gemm_exact.md."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_exact_ref as R
from tests.gpu_util import lib, ptr, stream, sync

pytestmark = pytest.mark.gpu

SENT = 1000.0            # bf16 number outside [-256, 256]: not a legal result
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32

# GemmTune's defaults (slamkit_amd/csrc/kernels.h) of every option these tests touch
DEFAULTS = {"gemm_glds": 1, "gemm_tn_dma": 1, "gemm_group_rows": 3, "gemm_group_rows_256": 4, "gemm_nt_store": 0, "gemm_256": 1,
            "gemm_256_dswiglu": 1, "gemm_256_persist": 1, "gemm_256_stagger": 1200, "gemm_group_cols_256": 0, "gemm_nt224": 1,
            "gemm_tn_splits": 0, "gemm_tn_balanced": 1, "gemm_tn224": 1, "gemm_tn224_max_split": 16, "gemm_mf32": 0,
            "gemm_256_w4": 0, "gemm_256_roles": 0, "gemm_256_batch_loads": 1}


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            assert k in DEFAULTS, k
            assert lib().slam_set_option(None, k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            lib().slam_set_option(None, k.encode(), v)


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The operands and references are computed once per shape and shared; they go when the file is done."""
    yield
    for cached in (nt_case, swiglu_fwd_ref, dswiglu_case, tn_case):
        cached.cache_clear()
    torch.cuda.empty_cache()


def _f64(t):
    return t.double() + 0.0   # + 0.0: a -0 of the library product becomes +0, the kernels' accumulators start at +0


# =============================================================================================== NT family
class NTCase:
    """Y[M][N] = X[M][K] W[N][K]^T: poisoned operands (made on first use) and exact expectations (made on first use)."""

    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        d = R.pick_density(K)
        self.X, self.W = R.poisoned(R.sparse_pm1(M, K, d, seed=1)), R.poisoned(R.sparse_pm1(N, K, d, seed=2))
        self.P = _f64(self.X.double() @ self.W.double().t())
        R.assert_f32_exact_range(f"nt {self}", self.P)
        self._ops, self._exp = {}, {}

    def __str__(self):
        return f"{self.M}x{self.N}x{self.K}"

    def op(self, name):
        if name not in self._ops:
            M, N = self.M, self.N
            make = {"bias": lambda: R.small_ints(N, -3, 3, seed=3), "res": lambda: R.small_ints((M, N), -3, 3, seed=4),
                    "mask": lambda: R.small_ints((M, N), -2, 2, seed=5)}[name]   # post-ReLU `act`: <= 0 means masked
            self._ops[name] = R.poisoned(make())
        return self._ops[name]

    def expect(self, epi):
        if epi not in self._exp:
            P = self.P
            ref = {"plain": lambda: P,
                   "bias_res": lambda: P + self.op("bias").double() + self.op("res").double(),
                   "res": lambda: P + self.op("res").double(),
                   "relu": lambda: torch.relu(P + self.op("bias").double()),
                   "drelu": lambda: torch.where(self.op("mask") > 0, P, torch.zeros_like(P))}[epi]()
            R.assert_bf16_exact_range(f"nt {self} {epi}", ref)
            self._exp[epi] = ref.to(BF16)
        return self._exp[epi]


@functools.lru_cache(maxsize=None)
def nt_case(M, N, K):
    return NTCase(M, N, K)


def run_nt(c, epi, tag, glds=1):
    """One launch of the entry point behind `epi` into a guarded, sentinel-filled Y; exact comparison, then the bands.
    slam_op_gemm_nt takes the staging mode as an argument, the ReLU entry points from the gemm_glds option."""
    L, (M, N, K) = lib(), (c.M, c.N, c.K)
    Y, bands = R.guarded((M, N), BF16, SENT)
    if epi in ("plain", "bias_res", "res"):
        rc = L.slam_op_gemm_nt(ptr(c.X), ptr(c.W), ptr(Y), ptr(c.op("bias")) if epi == "bias_res" else None,
                               ptr(c.op("res")) if epi != "plain" else None, M, N, K, glds, stream())
    elif epi == "relu":
        rc = L.slam_op_gemm_nt_relu(ptr(c.X), ptr(c.W), ptr(Y), ptr(c.op("bias")), M, N, K, stream())
    else:
        rc = L.slam_op_gemm_nt_drelu(ptr(c.X), ptr(c.W), ptr(Y), ptr(c.op("mask")), M, N, K, stream())
    sync()
    name = f"gemm_nt {epi} {c} [{tag}]"
    assert rc == 0, f"{name}: rc {rc}"
    R.assert_exact(name, Y, c.expect(epi))
    bands(name)
    return Y


EPILOGUES = ("plain", "bias_res", "relu", "drelu")


@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (7, 8, 72), (127, 120, 200), (129, 136, 72), (300, 264, 328)])
def test_nt_register_staging(M, N, K):
    """gemm_kernel with register staging: a single row, K tails (72, 200, 328 = 5 K-tiles + 8), column tails (8, 120, 136,
    264 - the 4-column epilogue's n < Cn guard), row tails, several tiles in both directions."""
    c = nt_case(M, N, K)
    with options(gemm_glds=0):
        for epi in EPILOGUES:
            run_nt(c, epi, "register staging", glds=0)


@pytest.mark.parametrize("mf32", [0, 1], ids=["mfma16x16x32", "mfma32x32x16"])
@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (127, 128, 128), (129, 256, 64), (385, 384, 192)])
def test_nt_128_dma(M, N, K, mf32):
    """The 128 x 128 LDS-DMA kernel (rows past M are clamped by the loads, never stored) on both MFMA shapes, with normal and
    streaming stores, and block orders of group height 1, 3 (a short last group at 4 row tiles) and 64 (more than the tile rows)."""
    c = nt_case(M, N, K)
    outs = {}
    for nt_store in (0, 1):
        for group_rows in (1, 3, 64):
            with options(gemm_256=0, gemm_mf32=mf32, gemm_nt_store=nt_store, gemm_group_rows=group_rows):
                for epi in EPILOGUES:
                    Y = run_nt(c, epi, f"128 dma mf32={mf32} nt_store={nt_store} group_rows={group_rows}")
                    assert torch.equal(Y, outs.setdefault(epi, Y))


@pytest.mark.parametrize("mf32", [0, 1], ids=["mfma16x16x32", "mfma32x32x16"])
def test_nt_256_one_block_per_tile(mf32):
    """gemm_nt_256_kernel, one block per tile: 256 tiles are the fewest the forced mode takes; every epilogue."""
    c = nt_case(4096, 4096, 128)
    with options(gemm_256=2, gemm_256_persist=0, gemm_mf32=mf32):
        for epi in EPILOGUES:
            run_nt(c, epi, f"256 per tile mf32={mf32}")


PERSISTENT_FORMS = [("mfma16", {}), ("mfma32", {"gemm_mf32": 1}), ("mfma32-w4", {"gemm_mf32": 1, "gemm_256_w4": 1}),
                    ("roles", {"gemm_256_roles": 1}), ("stagger0", {"gemm_256_stagger": 0}), ("group_cols3", {"gemm_group_cols_256": 3})]


@pytest.mark.parametrize("K", [192, 320])
def test_nt_256_persistent(K):
    """288 tiles on one block per CU: some blocks own two tiles, with 3 and 5 K-tiles per tile. Plain epilogue (the persistent
    launch takes no bias / residual / ReLU operand): eight-wave on both MFMA shapes, four-wave, loader / storer roles, no
    late start, 4 x 3 tile groups - the same bits every time."""
    c = nt_case(2304, 8192, K)
    first = None
    for form, opts in PERSISTENT_FORMS:
        with options(gemm_256=2, gemm_256_persist=1, **opts):
            Y = run_nt(c, "plain", f"256 persistent {form}")
        first = Y if first is None else first
        assert torch.equal(Y, first)


@pytest.mark.parametrize("M,N,K", [(256, 224, 128), (512, 896, 320)])
def test_nt_224(M, N, K):
    """gemm_nt224 = 2. (512, 896, 320) runs gemm_nt_224_kernel (2 x 4 tiles, 5 K-tiles). (256, 224, 128) does NOT: gemm_nt
    sends every N that is no multiple of 128 to register staging before the 224-wide kernel is considered, so only N = 896 k
    reaches it through the entry point - the shape stays, as the fallback it is (profiles/gemm_exact.md)."""
    c = nt_case(M, N, K)
    with options(gemm_nt224=2, gemm_256=0):
        for epi in ("plain", "res"):
            run_nt(c, epi, "nt224")


# =============================================================================================== fused SwiGLU
_worst = {}   # worst elementwise error in bf16 ulps per output kind, printed for profiles/gemm_exact.md


def held_elementwise(name, kind, got, ref64, floor):
    n, ratio, i, ulps = R.elementwise_excess(got, ref64, floor)
    _worst[kind] = max(_worst.get(kind, 0.0), ulps)
    print(f"[exact] {name}: worst |err| = {ulps:.3f} bf16 ulp, worst |err| / bar = {ratio:.3f} (floor {floor:.3e}); so far {kind}: {_worst[kind]:.3f} ulp")
    cols = got.shape[1]
    assert n == 0, (f"{name}: {n} of {got.numel()} elements over the elementwise bar, worst at row {i // cols}, column {i % cols}: "
                    f"got {float(got.reshape(-1)[i])}, fp64 {float(ref64.reshape(-1)[i])}, |err| / bar {ratio:.3f}")


@functools.lru_cache(maxsize=None)
def swiglu_fwd_ref(M, N, K):
    gu = nt_case(M, N, K).P.view(M, N // 64, 2, 32)   # W rows in 32-row gate / up blocks
    return (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(M, N // 2)


def run_swiglu_fwd(M, N, K, tag):
    c, L = nt_case(M, N, K), lib()
    Y, y_bands = R.guarded((M, N), BF16, SENT)
    act, a_bands = R.guarded((M, N // 2), BF16, NAN)
    rc = L.slam_op_gemm_nt_swiglu(ptr(c.X), ptr(c.W), ptr(Y), ptr(act), M, N, K, stream())
    sync()
    name = f"gemm_nt_swiglu {c} [{tag}]"
    assert rc == 0, f"{name}: rc {rc}"
    R.assert_exact(name + " Y", Y, c.expect("plain"))
    held_elementwise(name + " act", "act", act, swiglu_fwd_ref(M, N, K), 0.0)
    y_bands(name + " Y")
    a_bands(name + " act")


class DSwigluCase:
    """d(act)[M][I] = dY[M][H] Wt[I][H]^T never stored; gu[M][2I] (32-column gate / up blocks, half-integers in [-2, 2]:
    silu on both sides of zero) rewritten with d(gate) = d up s (1 + g (1 - s)), d(up) = d g s, s = sigmoid(g)."""

    def __init__(self, M, N, K):
        c = nt_case(M, N, K)
        self.c, self.M, self.N, self.K = c, M, N, K
        self.gu0 = (R.small_ints((M, 2 * N), -4, 4, seed=6) * 0.5).to(BF16).cuda()

        def formula(d, gu):
            g, u = gu[:, :, 0], gu[:, :, 1]
            s = torch.sigmoid(g)
            dv = d.view(M, N // 32, 32)
            return torch.stack([dv * u * s * (1 + g * (1 - s)), dv * g * s], 2).reshape(M, 2 * N)

        self.ref = formula(c.P, self.gu0.double().view(M, N // 32, 2, 32))
        emu = formula(c.P.float(), self.gu0.float().view(M, N // 32, 2, 32))   # c.P is exact in fp32 (asserted in NTCase)
        self.floor = 2.0 * float((emu.double() - self.ref).abs().max())
        print(f"[exact] dswiglu {c}: measured floor = {self.floor:.3e} (2 x worst fp32 torch error; ref abs-max {float(self.ref.abs().max()):.1f})")


@functools.lru_cache(maxsize=None)
def dswiglu_case(M, N, K):
    return DSwigluCase(M, N, K)


def run_dswiglu(M, N, K, tag):
    k, L = dswiglu_case(M, N, K), lib()
    gu, bands = R.guarded((M, 2 * N), BF16, SENT)
    gu.copy_(k.gu0)
    rc = L.slam_op_gemm_nt_dswiglu(ptr(k.c.X), ptr(k.c.W), ptr(gu), M, N, K, stream())
    sync()
    name = f"gemm_nt_dswiglu {k.c} [{tag}]"
    assert rc == 0, f"{name}: rc {rc}"
    held_elementwise(name, "gu", gu, k.ref, k.floor)
    bands(name)


@pytest.mark.parametrize("mf32", [0, 1], ids=["mfma16x16x32", "mfma32x32x16"])
@pytest.mark.parametrize("M,N,K", [(129, 256, 64), (385, 384, 192)])
def test_swiglu_128_dma(M, N, K, mf32):
    with options(gemm_256=0, gemm_mf32=mf32):
        run_swiglu_fwd(M, N, K, f"128 dma mf32={mf32}")
        run_dswiglu(M, N, K, f"128 dma mf32={mf32}")


@pytest.mark.parametrize("mf32", [0, 1], ids=["mfma16x16x32", "mfma32x32x16"])
def test_swiglu_256_one_block_per_tile(mf32):
    M, N, K = 4096, 4096, 128
    with options(gemm_256=2, gemm_256_persist=0, gemm_mf32=mf32):
        run_swiglu_fwd(M, N, K, f"256 per tile mf32={mf32}")
    for dsw in (0, 1):   # 0: the backward stays on the 128 x 128 kernel
        for batch in (0, 1):
            with options(gemm_256=2, gemm_256_persist=0, gemm_mf32=mf32, gemm_256_dswiglu=dsw, gemm_256_batch_loads=batch):
                run_dswiglu(M, N, K, f"256 per tile mf32={mf32} dswiglu={dsw} batch_loads={batch}")


@pytest.mark.parametrize("K", [192, 320])
def test_swiglu_256_persistent(K):
    M, N = 2304, 8192
    for form, opts in PERSISTENT_FORMS[:4]:
        with options(gemm_256=2, gemm_256_persist=1, **opts):
            run_swiglu_fwd(M, N, K, f"256 persistent {form}")
        for dsw, batch in ((1, 0), (1, 1)) + (((0, 1),) if not opts else ()):
            with options(gemm_256=2, gemm_256_persist=1, gemm_256_dswiglu=dsw, gemm_256_batch_loads=batch, **opts):
                run_dswiglu(M, N, K, f"256 persistent {form} dswiglu={dsw} batch_loads={batch}")


# =============================================================================================== NN
@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (129, 72, 136), (127, 200, 120), (255, 64, 264), (385, 192, 384)])
def test_nn(M, N, K):
    """dX[M][K] = dY[M][N] W[N][K] (+ resid): register staging with the in-register transpose of W; contraction tails (72,
    200), output-width tails (8, 136, 120, 264), row tails, one row."""
    d = R.pick_density(N)
    dY, W = R.poisoned(R.sparse_pm1(M, N, d, seed=1)), R.poisoned(R.sparse_pm1(N, K, d, seed=2))
    res = R.poisoned(R.small_ints((M, K), -3, 3, seed=4))
    P = _f64(dY.double() @ W.double())
    for use_res in (False, True):
        ref = P + res.double() if use_res else P
        name = f"gemm_nn {M}x{N}x{K} res={use_res}"
        R.assert_bf16_exact_range(name, ref)
        dX, bands = R.guarded((M, K), BF16, SENT)
        rc = lib().slam_op_gemm_nn(ptr(dY), ptr(W), ptr(dX), ptr(res) if use_res else None, M, N, K, stream())
        sync()
        assert rc == 0, f"{name}: rc {rc}"
        R.assert_exact(name, dX, ref)
        bands(name)


# =============================================================================================== TN (weight gradients)
class TNCase:
    """dW[N][K] (+)= dY[M][N]^T X[M][K], contraction over M."""

    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        d = R.pick_density(M)
        self.dY, self.X = R.poisoned(R.sparse_pm1(M, N, d, seed=8)), R.poisoned(R.sparse_pm1(M, K, d, seed=9))
        self.dW0 = R.small_ints((N, K), -5, 5, seed=10).cuda()
        self.P = _f64(self.dY.double().t() @ self.X.double())
        R.assert_f32_exact_range(f"tn {M}x{N}x{K}", self.P)
        R.assert_f32_exact_range(f"tn {M}x{N}x{K} accumulated", self.P + self.dW0.double())
        self.results = []   # dW after the accumulating pass of every run: the same bits under every plan


@functools.lru_cache(maxsize=None)
def tn_case(M, N, K):
    return TNCase(M, N, K)


def run_tn(c, tag, image=False, background=0):
    """accumulate = 0 onto a NaN-filled dW, then accumulate = 1 onto small integers; the workspace holds NaN before either
    call (a slab read that was never written shows) and is exactly as long as the entry point says, to 16 bytes."""
    L, (M, N, K) = lib(), (c.M, c.N, c.K)
    nbytes = L.slam_op_gemm_tn_workspace(M, N, K)
    assert nbytes > 0
    ws, ws_bands = R.guarded(((nbytes + 15) // 16 * 4,), F32, NAN)
    dW, dw_bands = R.guarded((N, K), F32, NAN)
    for acc in (0, 1):
        name = f"gemm_tn{'_image' if image else ''} {M}x{N}x{K} accumulate={acc} background={background} [{tag}]"
        if acc:
            dW.copy_(c.dW0)
        ws.fill_(NAN)
        if image:
            img, img_bands = R.guarded((N, K), BF16, SENT)
            rc = L.slam_op_gemm_tn_image(ptr(c.dY), ptr(c.X), ptr(dW), ptr(img), acc, M, N, K, ptr(ws), background, stream())
        else:
            rc = L.slam_op_gemm_tn(ptr(c.dY), ptr(c.X), ptr(dW), acc, M, N, K, ptr(ws), stream())
        sync()
        assert rc == 0, f"{name}: rc {rc}"
        R.assert_exact(name, dW, c.P + c.dW0.double() if acc else c.P)
        if image:
            n, info = R.first_mismatch(img, dW.to(BF16))
            assert n == 0, f"{name}: the bf16 image differs from dW.to(bfloat16) in {n} elements, first {info}"
            img_bands(name + " image")
        dw_bands(name + " dW")
        ws_bands(name + " workspace")
    c.results.append(dW.clone())
    assert torch.equal(c.results[0], c.results[-1]), f"{name}: dW differs from the first plan's"


def run_tn_all(c, tag):
    run_tn(c, tag)
    for background in (0, 1):
        run_tn(c, tag, image=True, background=background)


@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (63, 136, 72), (65, 128, 128), (333, 72, 40), (520, 128, 128)])
def test_tn_generic_register_staging(M, N, K):
    """gemm_kernel<TA, TB, F32OUT> with register staging + reduce_splits_kernel: a one-row contraction, contractions that are
    no multiple of the 64-row K-tile under tile-multiple outputs (65, 520) and ragged ones (63, 333). (520, 128, 128) under
    gemm_tn_splits 1, 2, 3, 7: with 3, pieces of 192 rows and a last one of 136 = two K-tiles and 8 rows."""
    c = tn_case(M, N, K)
    run_tn_all(c, "generic, default options")
    if M == 520:
        for splits in (1, 2, 3, 7):
            with options(gemm_tn_splits=splits):
                run_tn_all(c, f"generic, gemm_tn_splits={splits}")


@pytest.mark.parametrize("M,N,K", [(64, 128, 128), (320, 256, 128)])
def test_tn_generic_dma(M, N, K):
    """The split-K fallback on whole tiles (gemm_tn_balanced = 0): LDS-DMA staging, and register staging of the same shapes
    (gemm_tn_dma = 0), in 1, 2 and 5 pieces."""
    c = tn_case(M, N, K)
    for dma in (1, 0):
        for splits in (1, 2, 5):
            with options(gemm_tn_balanced=0, gemm_tn_dma=dma, gemm_tn_splits=splits):
                run_tn_all(c, f"generic, gemm_tn_dma={dma} gemm_tn_splits={splits}")


@pytest.mark.parametrize("M,N,K", [(256, 512, 256), (1600, 512, 256), (8192, 1152, 896)])
def test_tn_balanced(M, N, K):
    """gemm_tn_bal_kernel + reduce_bal_kernel under the default options: the shapes test_gemm_tn_bf16_image_is_the_rounded_result
    lists for the equal-pieces, mixed and unsplit plans, foreground and background planning."""
    run_tn_all(tn_case(M, N, K), "balanced, default options")


@pytest.mark.parametrize("M,N,K", [(64, 256, 224), (320, 224, 256), (2048, 768, 672)])
def test_tn_224(M, N, K):
    """gemm_tn_224_kernel + reduce_224_kernel forced on (gemm_tn224 = 2): one K-tile, the transposed store orientation
    (320, 224, 256), several tiles; unsplit (gemm_tn224_max_split = 1, and every background launch) and up to 16 pieces."""
    c = tn_case(M, N, K)
    for max_split in (1, 16):
        with options(gemm_tn224=2, gemm_tn224_max_split=max_split):
            run_tn_all(c, f"tn224, max_split={max_split}")
