"""-m gpu: every kernel that touches the [tokens][152,320] logits / d-logits buffer, run on that buffer at rows beyond byte 2^31
and byte 2^32 (tests/far_rows_ref.py: M_FAR = 14,592 rows, 4.14 GiB, row 7,049 holds byte 2^31 and row 14,098 byte 2^32).

GEMMs are held to EQUALITY over the WHOLE output on operands in {-1, 0, +1}: the head forward (output beyond 4 GiB), the head
dgrad (X operand beyond 4 GiB, NT and NN) and the head wgrad (contraction over the far rows; also with d-logits that are zero
below row 14,099, where anything fetched from a wrapped address is a visible non-zero). Every reference is an fp32 torch
product over chunks of at most 1,024 rows and is asserted to lie inside the exact range before it is compared.
The movers and scalers (copy_cols, unpad_logits, scale_bf16, scale_rows_bf16, scale_rows_unpadded_bf16) are held to the bits
of a chunked torch restatement. Cross entropy is held per element to float64 by the rule of tests/row_exact_ref.py, with the
bound its docstring derives for 75 online steps per lane (delta_steps; proven on the CPU by tests/test_far_rows_host.py).

Operands and outputs sit between the 256-element bands of row_exact_ref.guarded; outputs start as NaN; every launch runs twice
and must give the same bits; bands are checked after each launch. The big inputs are built on the device in row chunks, shared
per module and released by a module fixture. No test holds more than 16 GiB of device memory (each prints its peak).
A failure names the row class ("before 2 GiB", "straddles 2^31 B", "between", "straddles 2^32 B", "beyond 4 GiB"), the 128- and
256-row tile, the count and the first differing (row, column, got, expected).

Which kernel each case reaches, the times and the measured figures: profiles/far_rows.md."""
import functools

import numpy as np
import pytest
import torch

from tests import far_rows_ref as FR
from tests import row_exact_ref as R
from tests.gpu_util import lib, ptr, stream, sync
from tests.test_gpu_gemm_exact import options
from tests.test_gpu_row_exact import ce_protocol

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
M, VP, V = FR.M_FAR, FR.VP, FR.V
FAR0 = FR.ROW_4G + 1          # the first row that lies wholly beyond byte 2^32
B_, T_ = 19, 768
assert B_ * T_ == M


# =============================================================================================== shared inputs
@functools.lru_cache(maxsize=None)
def big_dy(far_only):
    """The d-logits [M_FAR][VP] in {-1, 0, +1} (density 1/16) between bands; far_only: zero below row FAR0, the same values from
    there on. -> (payload, band check)"""
    dY, chk = R.guarded((M, VP), BF16, DEV)
    FR.fill_pm1(dY, FR.DENSITY[VP][0], 11, row_lo=FAR0 if far_only else 0)
    return dY, chk


def operand(t):
    return R.guarded(tuple(t.shape), BF16, DEV, fill=t)[0]


def pm1(rows, cols, density, seed):
    return operand(FR.fill_pm1(torch.empty(rows, cols, dtype=BF16, device=DEV), density, seed))


def drop_big():
    for cached in (big_dy, head_fwd_case, dgrad_case, nn_case, tn_case):
        cached.cache_clear()
    torch.cuda.empty_cache()


_foreign = [0]   # bytes other modules of a whole-suite run keep allocated: measured when this module begins, not this file's


@pytest.fixture(scope="module", autouse=True)
def _release():
    torch.cuda.synchronize()
    _foreign[0] = torch.cuda.memory_allocated()
    yield
    drop_big()


@pytest.fixture(autouse=True)
def _peak():
    """What a case holds at its peak, the module's shared inputs included: everything allocated above what the process held
    when the module began."""
    torch.cuda.reset_peak_memory_stats()
    yield
    gib = (torch.cuda.max_memory_allocated() - _foreign[0]) / 2 ** 30
    print(f"[far-rows] peak device memory of this case: {gib:.2f} GiB (other modules hold {_foreign[0] / 2 ** 30:.2f} GiB)")
    assert gib <= 16.0


def same_bits_chunked(name, a, b, row_bytes=FR.ROW_BYTES):
    mm = FR.Mismatch(name, row_bytes)
    for r0, r1 in FR.chunks(a.shape[0]):
        mm.add(a[r0:r1], b[r0:r1], r0)
    mm.check()


# =============================================================================================== GEMM: output beyond 4 GiB
@functools.lru_cache(maxsize=None)
def head_fwd_case():
    a, b = FR.DENSITY[128]
    X, W = pm1(M, 128, a, 1), pm1(VP, 128, b, 2)
    return X, W, W.float().t().contiguous()


HEAD_FWD = [("128-mfma16", dict(gemm_256=0, gemm_mf32=0), 1), ("128-mfma32", dict(gemm_256=0, gemm_mf32=1), 1),
            ("128-nt_store", dict(gemm_256=0, gemm_nt_store=1), 1),
            ("256-persistent", dict(gemm_256=2), 1), ("256-per-tile", dict(gemm_256=2, gemm_256_persist=0), 1),
            ("256-mfma32-w4", dict(gemm_256=2, gemm_mf32=1, gemm_256_w4=1), 1), ("256-roles", dict(gemm_256=2, gemm_256_roles=1), 1),
            ("256-nt_store", dict(gemm_256=2, gemm_nt_store=1), 1), ("register-staging", dict(gemm_glds=0), 0)]


@pytest.mark.parametrize("form,opts,glds", HEAD_FWD, ids=[f[0] for f in HEAD_FWD])
def test_gemm_nt_output_beyond_4GiB(form, opts, glds):
    """The head forward: Y [14592][152320] = X [14592][128] W [152320][128]^T, 57 x 595 tiles of 256 x 256 (114 x 1190 of
    128 x 128); every element of the 4.14 GiB output against the fp32 product of its row chunk."""
    X, W, W32t = head_fwd_case()
    Y, bands = R.guarded((M, VP), BF16, DEV)
    name = f"gemm_nt {M}x{VP}x128 [{form}]"
    for run in (1, 2):
        Y.fill_(NAN)
        with options(**opts):
            rc = lib().slam_op_gemm_nt(ptr(X), ptr(W), ptr(Y), None, None, M, VP, 128, glds, stream())
        sync()
        assert rc == 0, f"{name}: rc {rc}"
        bands(f"{name} run {run}")
        mm = FR.Mismatch(f"{name} run {run}")
        for r0, r1 in FR.chunks(M):
            ref = FR.nt_rows(X, W32t, r0, r1)
            FR.assert_range(name, ref)
            mm.add(Y[r0:r1], ref, r0)
        mm.check()


# =============================================================================================== GEMM: X operand beyond 4 GiB
def rows_ref(X, Wt32, name):
    """X [M][K] Wt32 [K][n] as bf16 [M][n], exact: chunked fp32 products, each asserted to stay within +-256"""
    out = torch.empty(X.shape[0], Wt32.shape[1], dtype=BF16, device=DEV)
    for r0, r1 in FR.chunks(X.shape[0]):
        ref = FR.nt_rows(X, Wt32, r0, r1)
        FR.assert_range(name, ref)
        out[r0:r1] = ref.to(BF16)
    return out


@functools.lru_cache(maxsize=None)
def dgrad_case(N):
    W = pm1(N, VP, FR.DENSITY[VP][1], 20 + N)
    return W, rows_ref(big_dy(False)[0], W.float().t().contiguous(), f"dgrad reference N={N}")


DGRAD = [("N128-128-mfma16", 128, dict(gemm_256=0, gemm_mf32=0), 1), ("N128-128-mfma32", 128, dict(gemm_256=0, gemm_mf32=1), 1),
         ("N128-register-staging", 128, dict(gemm_glds=0), 0), ("N1280-256-persistent", 1280, dict(gemm_256=2), 1),
         ("N896-nt224", 896, dict(gemm_nt224=2, gemm_256=0), 1)]


@pytest.mark.parametrize("form,N,opts,glds", DGRAD, ids=[f[0] for f in DGRAD])
def test_gemm_nt_x_operand_beyond_4GiB(form, N, opts, glds):
    """The head dgrad: dX [14592][N] = dY [14592][152320] W [N][152320]^T, 2,380 K-tiles, exact. N = 1280 is 285 tiles of
    256 x 256 on 256 persistent blocks (29 own two), N = 896 the 256 x 224 kernel."""
    (dY, dy_bands), (W, ref) = big_dy(False), dgrad_case(N)
    name = f"gemm_nt {M}x{N}x{VP} [{form}]"
    for run in (1, 2):
        Y, bands = R.guarded((M, N), BF16, DEV)
        with options(**opts):
            rc = lib().slam_op_gemm_nt(ptr(dY), ptr(W), ptr(Y), None, None, M, N, VP, glds, stream())
        sync()
        assert rc == 0, f"{name}: rc {rc}"
        bands(f"{name} run {run}")
        dy_bands(f"{name} run {run}: d-logits")
        same_bits_chunked(f"{name} run {run}", Y, ref)


@functools.lru_cache(maxsize=None)
def nn_case():
    W = pm1(VP, 136, FR.DENSITY[VP][1], 31)
    return W, rows_ref(big_dy(False)[0], W.float(), "gemm_nn reference")


def test_gemm_nn_dy_beyond_4GiB():
    """The head dgrad without a transposed weight image: dX [14592][136] = dY [14592][152320] W [152320][136]."""
    (dY, dy_bands), (W, ref) = big_dy(False), nn_case()
    name = f"gemm_nn {M}x{VP}x136"
    for run in (1, 2):
        dX, bands = R.guarded((M, 136), BF16, DEV)
        rc = lib().slam_op_gemm_nn(ptr(dY), ptr(W), ptr(dX), None, M, VP, 136, stream())
        sync()
        assert rc == 0, f"{name}: rc {rc}"
        bands(f"{name} run {run}")
        dy_bands(f"{name} run {run}: d-logits")
        same_bits_chunked(f"{name} run {run}", dX, ref)


# =============================================================================================== GEMM: contraction over far rows
@functools.lru_cache(maxsize=2)   # far_only varies fastest: both cases of one K stay while its forms run
def tn_case(K, far_only):
    X = pm1(M, K, FR.DENSITY[M][1], 40 + K)
    P = FR.tn_ref(big_dy(far_only)[0], X)
    dW0 = FR.small_ints((VP, K), -5, 5, 50 + K, DEV)
    FR.assert_range(f"tn K={K}", P.abs() + 5, FR.F32_EXACT_MAX, strict=True)
    assert bool((P == P.round()).all())
    return X, P.float(), (P + dW0.double()).float(), dW0


TN = [("K224-tn224-unsplit", 224, dict(gemm_tn224=2, gemm_tn224_max_split=1)), ("K224-tn224-split16", 224, dict(gemm_tn224=2, gemm_tn224_max_split=16)),
      ("K256-tn224-transposed", 256, dict(gemm_tn224=2)), ("K128-balanced", 128, {}),
      ("K128-generic-dma", 128, dict(gemm_tn_balanced=0, gemm_tn_dma=1)), ("K128-generic-register", 128, dict(gemm_tn_balanced=0, gemm_tn_dma=0)),
      ("K72-ragged-register", 72, {})]


@pytest.mark.parametrize("far_only", [False, True], ids=["all-rows", "far-rows-only"])
@pytest.mark.parametrize("form,K,opts", TN, ids=[f[0] for f in TN])
def test_gemm_tn_contraction_over_far_rows(form, K, opts, far_only):
    """The head wgrad: dW [152320][K] (+)= dY [14592][152320]^T X [14592][K] through slam_op_gemm_tn and slam_op_gemm_tn_image
    (background 0 and 1), accumulate 0 onto NaN then 1 onto small integers; the image must be dW.to(bfloat16) bit for bit; the
    workspace has exactly slam_op_gemm_tn_workspace bytes. far-rows-only: dY is zero below row 14,099, so dW is the far rows'
    contribution alone and a fetch from a wrapped (near) address shows as a missing or a spurious term."""
    L = lib()
    (dY, dy_bands), (X, P, Pacc, dW0) = big_dy(far_only), tn_case(K, far_only)
    nbytes = L.slam_op_gemm_tn_workspace(M, VP, K)
    assert nbytes > 0
    ws, ws_bands = R.workspace(nbytes, DEV)
    what = "dY zero below row %d (rows beyond 4 GiB only)" % FAR0 if far_only else "dY dense in every row"
    for image, background in ((False, 0), (True, 0), (True, 1)):
        for acc in (0, 1):
            for run in (1, 2):
                name = (f"gemm_tn{'_image' if image else ''} {M}x{VP}x{K} [{form}; {what}] accumulate={acc} background={background} run {run}")
                dW, dw_bands = R.guarded((VP, K), F32, DEV, fill=dW0 if acc else None)
                ws.fill_(NAN)
                with options(**opts):
                    if image:
                        img, img_bands = R.guarded((VP, K), BF16, DEV)
                        rc = L.slam_op_gemm_tn_image(ptr(dY), ptr(X), ptr(dW), ptr(img), acc, M, VP, K, ptr(ws), background, stream())
                    else:
                        rc = L.slam_op_gemm_tn(ptr(dY), ptr(X), ptr(dW), acc, M, VP, K, ptr(ws), stream())
                sync()
                assert rc == 0, f"{name}: rc {rc}"
                dw_bands(name + " dW")
                ws_bands(name + " workspace")
                dy_bands(name + " d-logits")
                mm = FR.Mismatch(name, None)
                mm.add(dW, Pacc if acc else P)
                mm.check()
                if image:
                    img_bands(name + " image")
                    mi = FR.Mismatch(name + ": bf16 image vs dW.to(bfloat16)", None)
                    mi.add(img, dW.to(BF16))
                    mi.check()


# =============================================================================================== cross entropy
@pytest.mark.parametrize("num_items", [0.0, 57.0])
@pytest.mark.parametrize("eps", [0.0, R.EPS_SMOOTH], ids=["plain", "smooth"])
def test_cross_entropy_wide_row(eps, num_items):
    """(a) The real vocabulary near the origin: the whole protocol of test_gpu_row_exact.test_cross_entropy (special rows, NaN
    and 3e38 pads, aliased, NULL d-logits) at V = 152,167, Vp = 152,320: 75 steps per thread, under delta_steps(75)."""
    assert R.ce_big_steps(VP) == 75
    ce_protocol(V, VP, 3, 7, eps, num_items, R.delta_steps(75))


def far_labels():
    """labels [19][768], all valid, then around the rows that hold byte 2^31 and byte 2^32 and at the end: ignored rows, labels
    outside [0, V), targets in the first and in the last valid column. Row m is scored against the label at flat index m + 1."""
    lab = torch.randint(0, V, (B_, T_), generator=torch.Generator().manual_seed(3)).reshape(-1)
    for row, val in ((FR.ROW_2G - 1, -100), (FR.ROW_2G, V - 1), (FR.ROW_2G + 1, V), (FR.ROW_2G + 2, -7),
                     (FR.ROW_4G - 1, V), (FR.ROW_4G, V - 1), (FR.ROW_4G + 1, -100), (FR.ROW_4G + 2, 0), (FR.ROW_4G + 3, V - 1),
                     (M - 4, -100), (M - 3, V + 5), (M - 2, V - 1)):
        assert row % T_ != T_ - 1
        lab[row + 1] = val
    return lab.reshape(B_, T_)


def fill_logits(z):
    """bf16 logits N(0, 8) clamped to +-30 in the V valid columns, +0 in the pads; chunk by chunk from per-chunk seeds"""
    g = torch.Generator(device=DEV)
    for r0, r1 in FR.chunks(M):
        g.manual_seed(7_000_003 + r0)
        z[r0:r1, :V] = (torch.randn((r1 - r0, V), generator=g, device=DEV) * 8.0).clamp_(-30.0, 30.0).to(BF16)
        z[r0:r1, V:] = 0.0


CE_ROWS = 128   # rows per float64 chunk: 156 MB per float64 tensor of the reference


@pytest.mark.parametrize("num_items", [0.0, 9973.0])
@pytest.mark.parametrize("eps", [0.0, R.EPS_SMOOTH], ids=["plain", "smooth"])
def test_cross_entropy_far_rows(eps, num_items):
    """(b) (B, T) = (19, 768): 14,592 rows of the real vocabulary, every row and every column against float64 under
    delta_steps(75); pad columns and unscored rows +0 by bits; row_loss, row_smooth and the loss; a second launch into a
    second buffer and an aliased launch (d-logits over the logits) must give the same bits."""
    drop_big()
    L = lib()
    delta = R.delta_steps(R.ce_big_steps(VP))
    lab = far_labels()
    tgt, count = R.ce_targets(lab, V)
    denom = float(num_items) if num_items > 0 else float(count)
    tgt_d, labd = tgt.to(DEV), lab.to(DEV)
    valid = tgt_d >= 0
    assert int((~valid).sum()) >= B_ + 6 and count < M
    tag = f"ce far rows V={V} Vp={VP} {B_}x{T_} eps={eps:.1f} items={num_items:.0f}"

    def launch(zd, dl, rl, rs, sc):
        if eps:
            return L.slam_op_cross_entropy_smooth(ptr(zd), ptr(labd), num_items, ptr(dl), ptr(rl), ptr(rs), ptr(sc), B_, T_, VP, V, eps, stream())
        return L.slam_op_cross_entropy(ptr(zd), ptr(labd), num_items, ptr(dl), ptr(rl), ptr(sc), B_, T_, VP, V, stream())

    def run(zd, cz, alias):
        dl, cd = (zd, cz) if alias else R.guarded((M, VP), BF16, DEV)
        rl, c1 = R.guarded(M, F32, DEV)
        rs, c2 = R.guarded(M, F32, DEV)
        sc, c3 = R.guarded(2, F32, DEV)
        assert launch(zd, dl, rl, rs, sc) == 0
        sync()
        for chk in (cz, cd, c1, c2, c3):
            chk(f"{tag} alias={alias}")
        return dl, rl, rs, sc

    z, cz = R.guarded((M, VP), BF16, DEV)
    fill_logits(z)
    dl, rl, rs, sc = run(z, cz, False)
    assert float(sc[0]) == denom
    # ---- float64, chunk by chunk
    bad = {"dlogits": 0, "pads": 0, "unscored": 0}
    first, flips = None, 0
    rl_ref, rl_S, rs_ref, rs_S = [], [], [], []
    for r0, r1 in FR.chunks(M, CE_ROWS):
        r = R.cross_entropy_rows(z[r0:r1].double(), tgt_d[r0:r1], V, denom, eps)
        ref, S = r["dlogits"]
        got = dl[r0:r1]
        R.assert_normal(tag, ref)
        g64 = got.double()
        lo, hi = R.bf16_rne(ref - delta * S).double(), R.bf16_rne(ref + delta * S).double()
        ok = (lo <= g64) & (g64 <= hi)
        n = int((~ok).sum())
        flips += int((g64 != R.bf16_rne(ref).double()).sum())
        if n and first is None:
            i = int((~ok).reshape(-1).nonzero()[0])
            m, c = r0 + i // VP, i % VP
            first = (f"first at {FR.where(m)}, column {c}: got {float(g64.reshape(-1)[i])!r} not in [{float(lo.reshape(-1)[i])!r}, "
                     f"{float(hi.reshape(-1)[i])!r}], float64 {float(ref.reshape(-1)[i])!r}")
        bad["dlogits"] += n
        bad["pads"] += int((R.bits(got[:, V:]) != 0).sum())
        bad["unscored"] += int((R.bits(got[~valid[r0:r1]]) != 0).sum())
        rl_ref.append(r["row_loss"][0])
        rl_S.append(r["row_loss"][1])
        rs_ref.append(r["row_smooth"][0])
        rs_S.append(r["row_smooth"][1])
        del r, ref, S, lo, hi, ok, g64
    print(f"[far-rows] {tag} dlogits: n={M * VP} flips={flips / (M * VP):.3e} violations={bad['dlogits']} (delta {delta:.3e})")
    assert bad["dlogits"] == 0, f"{tag}: {bad['dlogits']} d-logits outside the rounding bound; {first}"
    assert bad["pads"] == 0, f"{tag}: {bad['pads']} pad columns of d-logits are not +0"
    assert bad["unscored"] == 0, f"{tag}: {bad['unscored']} elements of ignored / out-of-range rows of d-logits are not +0"
    rl_ref, rl_S, rs_ref, rs_S = (torch.cat(x) for x in (rl_ref, rl_S, rs_ref, rs_S))

    def rows_f32(what, got, ref, S):
        err = (got.double() - ref).abs()
        okr = err <= delta * S
        worst = float((err[S > 0] / S[S > 0]).max())
        print(f"[far-rows] {tag} {what}: worst |err|/S={worst:.3e} = {worst / delta:.3f} of the bound {delta:.3e}")
        if not bool(okr.all()):
            m = int((~okr).nonzero()[0])
            raise AssertionError(f"{tag} {what}: {int((~okr).sum())} rows outside the bound; first at {FR.where(m)}: got {float(got[m])!r}, "
                                 f"float64 {float(ref[m])!r}, S {float(S[m])!r}")
        assert bool((R.bits(got[~valid]) == 0).all()), f"{tag} {what}: unscored rows must be +0"
    rows_f32("row_loss", rl, rl_ref, rl_S)
    if eps:
        rows_f32("row_smooth", rs, rs_ref, rs_S)
    loss = ((1.0 - eps) * rl_ref.sum() + eps * rs_ref.sum()) / denom
    S_loss = ((1.0 - eps) * rl_S.sum() + eps * rs_S.sum()) / denom
    assert R.accept_f32(tag + " loss", sc[1:], loss.reshape(1), S_loss.reshape(1), R.delta_sum(M) + (delta - R.DELTA)) == 0
    # ---- the same launch again, into a second buffer
    dl2, rl2, rs2, sc2 = run(z, cz, False)
    same_bits_chunked(f"{tag}: d-logits, run 1 vs run 2", dl2, dl)
    for what, a, b in (("row_loss", rl2, rl), ("loss", sc2, sc)) + ((("row_smooth", rs2, rs),) if eps else ()):
        assert torch.equal(R.bits(a), R.bits(b)), f"{tag}: {what} differs between run 1 and run 2"
    del dl2
    # ---- aliased: the gradient replaces the logits
    dla, rla, rsa, sca = run(z, cz, True)
    same_bits_chunked(f"{tag}: aliased d-logits vs the separate buffer's", dla, dl)
    for what, a, b in (("row_loss", rla, rl), ("loss", sca, sc)) + ((("row_smooth", rsa, rs),) if eps else ()):
        assert torch.equal(R.bits(a), R.bits(b)), f"{tag}: {what} differs between the aliased and the separate launch"


# =============================================================================================== movers and scalers
def fill_bits(x):
    """every bf16 bit pattern, NaNs and infinities included: a mover must keep them all"""
    g = torch.Generator(device=DEV)
    xi = x.view(torch.int16)
    for r0, r1 in FR.chunks(x.shape[0]):
        g.manual_seed(9_000_011 + r0)
        xi[r0:r1] = torch.randint(-32768, 32768, (r1 - r0, x.shape[1]), generator=g, device=DEV, dtype=torch.int32).to(torch.int16)


def normal_chunk(r0, r1, cols):
    g = torch.Generator(device=DEV).manual_seed(8_000_009 + r0)
    return torch.randn((r1 - r0, cols), generator=g, device=DEV).to(BF16)


def test_copy_cols_far_rows():
    """logits_out: [14592][152320] -> [14592][152167]; source row 14,098 and destination row 14,112 hold byte 2^32."""
    drop_big()
    src, cs = R.guarded((M, VP), BF16, DEV)
    fill_bits(src)
    name = f"copy_cols {M}x{VP} -> {M}x{V}"
    for run in (1, 2):
        dst, cd = R.guarded((M, V), BF16, DEV)
        assert lib().slam_op_copy_cols(ptr(src), VP, ptr(dst), V, M, V, stream()) == 0
        sync()
        cs(name), cd(name)
        mm = FR.Mismatch(f"{name} run {run}")
        for r0, r1 in FR.chunks(M):
            mm.add(dst[r0:r1], src[r0:r1, :V], r0)
        mm.check()
        del dst


def ragged_lens():
    lens = np.array([T_ - (37 * b) % 300 for b in range(B_)], dtype=np.int32)
    lens[4], lens[11] = 0, T_
    return lens


@pytest.mark.parametrize("Vout", [V, 152160], ids=["V152167-elementwise", "V152160-16B-chunks"])
def test_unpad_logits_far_rows(Vout):
    """Padding-free logits_out: packed rows [Mp][152320] back to [19][768][V] with `off` as slam_op_unpad_pack leaves it;
    lens ragged, one 0 and one T. The destination crosses byte 2^31 and byte 2^32; pad positions are +0 by bits."""
    drop_big()
    L = lib()
    lens = ragged_lens()
    total = int(lens.sum())
    Mp = -(-total // 64) * 64
    assert FR.ROW_2G < total and Mp <= M
    mm_ = -(-(B_ * T_) // 64) * 64
    nbytes = L.slam_unpadded_scratch_bytes(B_, T_)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    assert scratch.data_ptr() % 256 == 0
    ids = torch.zeros(B_, T_, dtype=torch.int64, device=DEV)
    lens_d = torch.from_numpy(lens).to(DEV)
    assert L.slam_op_unpad_pack(ptr(ids), None, ptr(lens_d), B_, T_, Mp, 0, ptr(scratch), nbytes, stream()) == 0
    sync()
    off = scratch[mm_ * 36: mm_ * 36 + 4 * (B_ + 1)].view(torch.int32)       # behind three int64 and three int32 arrays of Mmax
    off_h = off.cpu().numpy()
    assert off_h.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    src, cs = R.guarded((Mp, VP), BF16, DEV)
    fill_bits(src)
    name = f"unpad_logits {B_}x{T_} V={Vout} Mp={Mp}"
    for run in (1, 2):
        dst, cd = R.guarded((M, Vout), BF16, DEV)
        assert L.slam_op_unpad_logits(ptr(src), VP, ptr(dst), Vout, ptr(off), B_, T_, Mp, stream()) == 0
        sync()
        cs(name), cd(name)
        di, si = dst, src
        mm = FR.Mismatch(f"{name} run {run}", 2 * Vout)
        for b in range(B_):
            n, o = int(lens[b]), int(off_h[b])
            if n:
                mm.add(di[b * T_: b * T_ + n], si[o:o + n, :Vout], b * T_)
            if n < T_:
                pad = di[b * T_ + n: (b + 1) * T_]
                mm.add(pad, torch.zeros_like(pad), b * T_ + n)
        mm.check()
        del dst, di


def scaled_expect(xc, s):
    """bf16_rne of the fp32 product: the kernel multiplies in fp32 and rounds once"""
    return R.bf16_rne((xc.float() * s).double())


def run_scaler(name, launch, coef_of_rows):
    """x [M_FAR][VP] of N(0, 1) bf16 values, rebuilt before each of two launches; every element against bf16_rne(x * coef)."""
    drop_big()
    x, cx = R.guarded((M, VP), BF16, DEV)
    for run in (1, 2):
        for r0, r1 in FR.chunks(M):
            x[r0:r1] = normal_chunk(r0, r1, VP)
        assert launch(x) == 0
        sync()
        cx(name)
        mm = FR.Mismatch(f"{name} run {run}")
        for r0, r1 in FR.chunks(M):
            x0 = normal_chunk(r0, r1, VP)
            for a, b in FR.chunks(r1 - r0, 256):
                mm.add(x[r0 + a:r0 + b], scaled_expect(x0[a:b], coef_of_rows(r0 + a, r0 + b)), r0 + a)
        mm.check()


@pytest.mark.parametrize("s", [0.5, 0.3])
def test_scale_bf16_far_rows(s):
    """grad_scale over the whole d-logits buffer: a power of two (exact) and 0.3 (one rounding of the fp32 product)."""
    s32 = float(np.float32(s))
    run_scaler(f"scale_bf16 {M}x{VP} by {s}", lambda x: lib().slam_op_scale_bf16(ptr(x), M * VP, s32, stream()),
               lambda r0, r1: s32)


def test_scale_rows_bf16_far_rows():
    """slam_scale_loss_rows: T = 768, 19 distinct coefficients (both signs, a zero, a power of two)."""
    coef = torch.tensor([0.3 * (b + 1) * (-1) ** b for b in range(B_)], dtype=F32)
    coef[5], coef[18] = 0.0, -0.71
    coef[7] = 0.25
    assert len(set(coef.tolist())) == B_
    cd = R.guarded(B_, F32, DEV, fill=coef)[0]
    per_row = cd[torch.arange(M, device=DEV) // T_]
    run_scaler(f"scale_rows_bf16 {M}x{VP} T={T_}", lambda x: lib().slam_op_scale_rows_bf16(ptr(x), ptr(cd), M, T_, VP, stream()),
               lambda r0, r1: per_row[r0:r1, None])


def test_scale_rows_unpadded_bf16_far_rows():
    """slam_scale_loss_unpadded: 19 packed segments and a tail of 200 rows with row = -1, which must scale by 0 (signed zeros);
    rows 14,099 .. 14,391 are real rows beyond 4 GiB, the tail lies behind them."""
    lens = np.full(B_, T_, dtype=np.int64)
    lens[B_ - 1] -= 200
    row = torch.full((M,), -1, dtype=torch.int32)
    row[: int(lens.sum())] = torch.repeat_interleave(torch.arange(B_, dtype=torch.int32), torch.from_numpy(lens))
    assert int(row[FAR0]) == B_ - 1 and int(row[M - 200]) == -1 and int(row[M - 201]) == B_ - 1
    coef = torch.tensor([0.45 + 0.07 * b for b in range(B_)], dtype=F32)
    cd = R.guarded(B_, F32, DEV, fill=coef)[0]
    rowd = torch.empty(M + 512, dtype=torch.int32, device=DEV).fill_(0x7FFFFFFF)[256:256 + M]     # far indices on either side
    rowd.copy_(row)
    per_row = torch.where(rowd >= 0, cd[rowd.clamp(min=0).long()], torch.zeros((), device=DEV))
    run_scaler(f"scale_rows_unpadded_bf16 {M}x{VP}", lambda x: lib().slam_op_scale_rows_unpadded_bf16(ptr(x), ptr(cd), ptr(rowd), M, VP, stream()),
               lambda r0, r1: per_row[r0:r1, None])
