"""CPU tier of the far-row tests (tests/far_rows_ref.py, tests/test_gpu_far_rows.py): the five op entries of the logits
movers and scalers are exported, bound and refuse bad arguments before anything reaches the device (the fake pointers below are
never dereferenced); the row classes of `where`; the operand densities keep the exact references inside the bf16-exact range;
and the rounding bound of a 75-step cross-entropy row, delta_steps (tests/row_exact_ref.py), holds for an fp32 restatement of
the row with every lane strictly sequential, at Vp = 152,320."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import far_rows_ref as FR
from tests import row_exact_ref as R

NEW = ["slam_op_copy_cols", "slam_op_unpad_logits", "slam_op_scale_bf16", "slam_op_scale_rows_bf16", "slam_op_scale_rows_unpadded_bf16"]
E_INVAL = -1
FAKE = C.c_void_p(1 << 20)


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n


def test_copy_cols_refuses_before_launch():
    lib, f = E.load_library(), FAKE

    def call(src=f, lds=FR.VP, dst=f, ldd=FR.V, M=8, ncols=FR.V):
        return lib.slam_op_copy_cols(src, lds, dst, ldd, M, ncols, None)
    assert call(src=None) == E_INVAL and call(dst=None) == E_INVAL
    assert call(M=0) == E_INVAL and call(M=-3) == E_INVAL and call(ncols=0) == E_INVAL
    assert call(lds=FR.V - 1) == E_INVAL      # a source row shorter than the columns copied
    assert call(ldd=FR.V - 1) == E_INVAL


def test_unpad_logits_refuses_before_launch():
    lib, f = E.load_library(), FAKE

    def call(src=f, Vp=FR.VP, dst=f, V=FR.V, off=f, B=2, T=8, Mp=64):
        return lib.slam_op_unpad_logits(src, Vp, dst, V, off, B, T, Mp, None)
    assert call(src=None) == E_INVAL and call(dst=None) == E_INVAL and call(off=None) == E_INVAL
    assert call(B=0) == E_INVAL and call(T=0) == E_INVAL and call(Mp=0) == E_INVAL and call(V=0) == E_INVAL
    assert call(V=FR.VP + 1) == E_INVAL       # V > Vp
    assert call(Vp=FR.VP + 4) == E_INVAL      # Vp % 8: the packed rows are read in 16-byte chunks


def test_scalers_refuse_before_launch():
    lib, f = E.load_library(), FAKE
    assert lib.slam_op_scale_bf16(None, 64, 0.5, None) == E_INVAL
    assert lib.slam_op_scale_bf16(f, 0, 0.5, None) == E_INVAL
    assert lib.slam_op_scale_bf16(f, -8, 0.5, None) == E_INVAL
    assert lib.slam_op_scale_bf16(f, 68, 0.5, None) == E_INVAL        # n % 8

    def rows(x=f, coef=f, M=16, T=8, ncols=FR.VP):
        return lib.slam_op_scale_rows_bf16(x, coef, M, T, ncols, None)
    assert rows(x=None) == E_INVAL and rows(coef=None) == E_INVAL
    assert rows(M=0) == E_INVAL and rows(T=0) == E_INVAL and rows(ncols=0) == E_INVAL
    assert rows(ncols=FR.V) == E_INVAL                                 # ncols % 8

    def unp(x=f, coef=f, row=f, Mp=64, ncols=FR.VP):
        return lib.slam_op_scale_rows_unpadded_bf16(x, coef, row, Mp, ncols, None)
    assert unp(x=None) == E_INVAL and unp(coef=None) == E_INVAL and unp(row=None) == E_INVAL
    assert unp(Mp=0) == E_INVAL and unp(ncols=0) == E_INVAL and unp(ncols=FR.V) == E_INVAL


def test_row_classes():
    assert (FR.ROW_2G, FR.ROW_4G, FR.M_FAR) == (7049, 14098, 14592)
    assert FR.M_FAR * FR.ROW_BYTES < 16 << 30
    assert FR.row_class(0) == FR.row_class(7048) == "before 2 GiB"
    assert FR.row_class(7049) == "straddles 2^31 B"
    assert FR.row_class(7050) == FR.row_class(14097) == "between"
    assert FR.row_class(14098) == "straddles 2^32 B"
    assert FR.row_class(14099) == FR.row_class(FR.M_FAR - 1) == "beyond 4 GiB"
    assert FR.where(14336) == "row 14336 (beyond 4 GiB; 256-row tile 56, 128-row tile 112)"
    # the unpadded logits [M][V]: 304,334-byte rows cross 2^32 B one row later than that
    assert FR.row_class(14112, 2 * FR.V) == "straddles 2^32 B"
    m = FR.Mismatch("probe")
    got, exp = torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(4, 8)
    m.add(got, exp, 14096)
    m.check()
    got[3, 5] = 1.0
    m.add(got, exp, 14096)
    with pytest.raises(AssertionError, match=r"1 of 64 elements differ.*row 14099 \(beyond 4 GiB; 256-row tile 55, 128-row tile 110\), column 5: got 1.0, expected 0.0"):
        m.check()


@pytest.mark.parametrize("K", sorted(FR.DENSITY))
def test_densities_keep_the_exact_references_in_range(K):
    """256 is at least 8 standard deviations of an output away (analytic), and a slice of each contraction, computed here with
    the generators and the references the GPU file uses, has the predicted spread and stays far inside."""
    a, b = FR.DENSITY[K]
    s = FR.sigma(K)
    assert FR.BF16_EXACT_MAX >= 8.0 * s, (K, s)
    ra, rb = (96, 512) if K != FR.M_FAR else (256, 128)
    if K == FR.M_FAR:       # contraction over the rows
        A = FR.fill_pm1(torch.empty(K, ra, dtype=torch.bfloat16), a, 1)
        Bm = FR.fill_pm1(torch.empty(K, rb, dtype=torch.bfloat16), b, 2)
        ref = FR.tn_ref(A, Bm)
    else:
        A = FR.fill_pm1(torch.empty(ra, K, dtype=torch.bfloat16), a, 1)
        Bm = FR.fill_pm1(torch.empty(rb, K, dtype=torch.bfloat16), b, 2)
        ref = FR.nt_rows(A, Bm.float().t().contiguous(), 0, ra).double()
        assert torch.equal(ref, A.double() @ Bm.double().t() + 0.0)      # the fp32 product is exact
    assert bool((ref == ref.round()).all())
    assert set(A.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert abs(float((A != 0).float().mean()) / a - 1) < 0.05
    FR.assert_range(f"slice of the {K}-deep contraction", ref)
    sd = float(ref.std())
    print(f"[far-rows] K={K}: densities {a} x {b}, sigma predicted {s:.2f} measured {sd:.2f}, abs-max of {ref.numel()} outputs {float(ref.abs().max()):.0f}")
    assert abs(sd / s - 1) < 0.1
    assert float(ref.abs().max()) <= 6.0 * s


# ------------------------------------------------------------------------------------------------ the bound at 75 steps
def _tree(a, op):
    """pairwise combination over the last axis (64 lanes by butterfly, 4 waves through LDS): log2 levels, not a sequence"""
    while a.shape[-1] > 1:
        a = op(a[..., 0::2], a[..., 1::2]).astype(np.float32)
    return a[..., 0]


def _fp32_ce_lanes(zf, tgt, V, denom, eps):
    """ce_big_kernel's arithmetic in numpy fp32 for rows zf [M][Vp]: 256 lanes, lane l owns the 8-column chunks l, l + 256, ..
    and walks them STRICTLY SEQUENTIALLY with the online max / sum (and the plain sum of the valid logits); lanes are combined
    pairwise. Returns (dlogits, row_loss, row_smooth, steps per lane)."""
    f = np.float32
    M, Vp = zf.shape
    nch = Vp // 8
    steps = -(-nch // 256)
    pad = np.full((M, steps * 256 * 8), -3.0e38, dtype=np.float32)
    pad[:, :Vp] = zf
    on = np.zeros(steps * 256 * 8, dtype=bool)
    on[:V] = True
    x = pad.reshape(M, steps, 256, 8)
    on = on.reshape(steps, 256, 8)
    mx = np.full((M, 256), -3.0e38, dtype=np.float32)
    sm = np.zeros((M, 256), dtype=np.float32)
    zs = np.zeros((M, 256), dtype=np.float32)
    for k in range(steps):
        fk = np.where(on[k][None], x[:, k], f(-3.0e38)).astype(np.float32)
        nm = np.maximum(mx, fk.max(-1))
        cs = np.zeros((M, 256), dtype=np.float32)
        for j in range(8):
            cs = (cs + np.where(on[k][None, :, j], np.exp(fk[:, :, j] - nm, dtype=np.float32), f(0))).astype(np.float32)
            zs = (zs + np.where(on[k][None, :, j], x[:, k, :, j], f(0))).astype(np.float32)
        sm = (sm * np.exp(mx - nm, dtype=np.float32) + cs).astype(np.float32)
        mx = nm
    bm = mx.max(-1, keepdims=True)
    bs = _tree((sm * np.exp(mx - bm, dtype=np.float32)).astype(np.float32), np.add)[:, None]
    zsum = _tree(zs, np.add)
    lse = (bm + np.log(bs, dtype=np.float32)).astype(np.float32)[:, 0]
    valid = tgt >= 0
    zy = zf[np.arange(M), np.where(valid, tgt, 0)]
    rl = np.where(valid, lse - zy, f(0)).astype(np.float32)
    rs = np.where(valid, lse - zsum / f(V), f(0)).astype(np.float32)
    inv, sc, e32 = f(1) / bs, f(1) / f(denom), f(eps)
    p = (np.exp(zf[:, :V] - bm, dtype=np.float32) * inv).astype(np.float32)
    if eps:
        p = (p - e32 / f(V)).astype(np.float32)
    rows = np.nonzero(valid)[0]
    p[rows, tgt[rows]] -= (f(1) - e32) if eps else f(1)
    d = np.zeros_like(zf)
    d[:, :V] = p * sc
    d[~valid] = 0
    return d, rl, rs, steps


@pytest.mark.parametrize("eps", [0.0, R.EPS_SMOOTH], ids=["plain", "smooth"])
def test_fp32_wide_cross_entropy_meets_the_stepped_rule(eps):
    """The (3, 7) case of test_gpu_far_rows.py's wide-row test at the real vocabulary. 75 steps per lane; delta_steps(75) =
    2^-16 + 568 2^-24, and the restatement has 0 violations under it (DELTA itself is printed alongside: it is NOT required to
    hold here, the budget behind it stops at 32 sequential adds)."""
    B, T, V, Vp = 3, 7, FR.V, FR.VP
    z, lab, under = R.ce_case(B, T, V, Vp, 1)
    r = R.cross_entropy(z, lab, V, 57.0, eps)
    d, rl, rs, steps = _fp32_ce_lanes(z.numpy().astype(np.float32), r["tgt"].numpy(), V, 57.0, eps)
    assert steps == R.ce_big_steps(Vp) == 75
    delta = R.delta_steps(steps)
    assert delta == 2.0 ** -16 + 568 * 2.0 ** -24 and R.delta_steps(3) == R.delta_steps(4) == R.DELTA < R.delta_steps(5)
    keep = torch.ones(B * T, dtype=torch.bool)
    keep[under] = False
    ref, S = r["dlogits"]
    got = torch.from_numpy(d).to(torch.bfloat16)
    assert R.accept_bf16("fp32 wide ce dlogits", got[keep], ref[keep], S[keep], delta) == 0
    assert R.accept_bf16("fp32 wide ce dlogits, saturated rows", got[~keep], ref[~keep], S[~keep], delta, underflow=True) == 0
    assert R.accept_f32("fp32 wide ce row_loss", torch.from_numpy(rl), *r["row_loss"], delta) == 0
    assert R.accept_f32("fp32 wide ce row_smooth", torch.from_numpy(rs), *r["row_smooth"], delta) == 0
    R.accept_f32("fp32 wide ce row_smooth under DELTA (informative)", torch.from_numpy(rs), *r["row_smooth"], R.DELTA)
    assert math.isclose(delta, 4.9e-5, rel_tol=0.02)
