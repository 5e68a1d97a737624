"""-m gpu: the attention kernels of slamkit_amd/csrc/attention.hip through the C ABI, held to EQUALITY on integer-score inputs.

Inputs (tests/attn_exact_ref.py; their conditions are proved on the CPU by tests/test_attn_exact_host.py): every score is an
integer, every softmax weight is 2^-a on a tie set of 1, 2 or 4 keys and exactly zero elsewhere, and the tie set's code is
shared by key i + 1 and key seg_start - 1, just outside the window. Every value the kernels round on the way (P, O, dS) is a
bf16 number, so
  * o, dv and (head_dim 64) dq must equal bf16(plain fp64 reference) bit for bit, zeros included;
  * dk (x LN2) and head_dim-128 dq (x 1/sqrtf(128)) lie within one bf16 ulp of it, exactly zero where it is zero (dk in
    tests of its own, test_exact_dk*);
  * lse2 = max + a lies within one fp32 ulp.
The reference is test_gpu_attn_block._attn_ref64 - masked softmax attention and autograd in fp64, no tiling.

Every operand (qkv, o, d_o, lse2) sits between NaN bands of 128 rows, every output (o, lse2, dqkv) is NaN before the launch and
sits between sentinel bands, the backward workspace is exactly slam_op_attn_bwd_workspace bytes (to 16), NaN before every
launch, between sentinel bands. No NaN may reach an output, no band may change.

A failure names row, head, column, segment, position, tile, fragment, chunk and the row's tie set (attn_exact_ref.locate).
Which code path each case reaches, and what the runs measured: profiles/attn_exact.md."""
import functools
from itertools import product

import pytest
import torch

from tests import attn_exact_ref as R
from tests.gpu_util import lib, ptr, stream, sync
from tests.test_gpu_attn_block import _attn_ref64

pytestmark = pytest.mark.gpu

DEFAULT_TUNE = {"attn_jq": 1, "attn_kw": 1, "attn_nch": 4, "attn_prio": 0}   # g_attn_tune in attention.hip
_share = {}   # elements not bit-equal to bf16(reference) / elements, per tensor kind that has a one-ulp bar (for the profile)


def _id(cid):
    return f"{cid[0]}-{cid[1]}-{cid[2]}-{cid[3]}"


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    device_case.cache_clear()
    torch.cuda.empty_cache()


class DeviceCase:
    """Poisoned device operands and the expectations of one generated case."""

    def __init__(self, c, with_backward=True):
        self.c = c
        self.qkv = R.poisoned(c.qkv_dev, R.BF16, "cuda")
        self.d_o = R.poisoned(c.d_o, R.BF16, "cuda")
        self.ss, self.se = c.seg_start.cuda(), c.seg_end.cuda()
        self.exp = R.expectations(c, _attn_ref64, "cuda") if with_backward else None
        self.name = R.describe(c)


@functools.lru_cache(maxsize=None)
def device_case(cid, flip):
    return DeviceCase(R.cases_of(*cid)[flip])


def _finite(name, t):
    bad = ~torch.isfinite(t.float())
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        cols = t.shape[1] if t.dim() > 1 else 1
        raise AssertionError(f"{name}: {int(bad.sum())} non-finite element(s) (a poisoned operand row or an unwritten output), "
                             f"first at row {i // cols}, column {i % cols}")


def run_fwd(d, tag=""):
    c = d.c
    o, o_bands = R.guarded((c.M, c.nH * c.hd), R.BF16, "cuda")
    lse, l_bands = R.guarded(c.nH * c.M, R.F32, "cuda")
    rc = lib().slam_op_attn_fwd(ptr(d.qkv), ptr(o), ptr(lse), ptr(d.ss), c.M, c.nH, c.nKV, c.hd, stream())
    sync()
    name = f"attn fwd {d.name}{tag}"
    assert rc == 0, f"{name}: rc {rc}"
    o_bands(name + " o"), l_bands(name + " lse2")
    _finite(name + " o", o), _finite(name + " lse2", lse.view(c.nH, c.M).t())
    return o, lse


def run_bwd(d, o, lse, rope=False, tag=""):
    """slam_op_attn_bwd, or slam_op_attn_bwd_rope with all positions zero. o and lse2 go in as poisoned copies."""
    c, L = d.c, lib()
    o_in, lse_in = R.poisoned(o, R.BF16, "cuda"), R.poisoned(lse, R.F32, "cuda")
    nbytes = L.slam_op_attn_bwd_workspace(c.M, c.nH, c.hd)
    assert nbytes > 0
    ws, ws_bands = R.guarded((nbytes + 15) // 16 * 4, R.F32, "cuda")
    dqkv, d_bands = R.guarded((c.M, c.ld), R.BF16, "cuda")
    name = f"attn bwd{' rope' if rope else ''} {d.name}{tag}"
    if rope:
        ntab = 2 * c.M * (c.hd // 2)
        tab, t_bands = R.guarded(ntab, R.F32, "cuda")
        pos = torch.zeros(c.M, dtype=torch.int64, device="cuda")
        rc = L.slam_op_attn_bwd_rope(ptr(d.qkv), ptr(o_in), ptr(d.d_o), ptr(lse_in), ptr(dqkv), ptr(ws), ptr(d.ss), ptr(d.se),
                                     ptr(pos), c.M, 1e4, c.M, c.nH, c.nKV, c.hd, ptr(tab), stream())
    else:
        rc = L.slam_op_attn_bwd(ptr(d.qkv), ptr(o_in), ptr(d.d_o), ptr(lse_in), ptr(dqkv), ptr(ws), ptr(d.ss), ptr(d.se),
                                c.M, c.nH, c.nKV, c.hd, stream())
    sync()
    assert rc == 0, f"{name}: rc {rc}"
    d_bands(name + " dqkv"), ws_bands(name + " workspace")
    if rope:
        t_bands(name + " rope tables")
    _finite(name + " dqkv", dqkv)
    return dqkv


def check_fwd(d, o, lse, tag=""):
    c, e = d.c, d.exp
    R.assert_bits(f"attn fwd {d.name}{tag} o", c, "o", o, e.o)
    got = lse.view(c.nH, c.M).t().double().cpu()
    R.assert_within(f"attn fwd {d.name}{tag} lse2", c, "lse2", got, e.lse2, R.f32_ulp(e.lse2))
    return float((got - e.lse2).abs().max())


def check_bwd(d, dqkv, tag="", **launch):
    """dv and dq: bits at head_dim 64; head_dim-128 dq within one bf16 ulp, exactly zero where the reference is."""
    c, e = d.c, d.exp
    a, b = c.nH * c.hd, (c.nH + c.nKV) * c.hd
    name = f"attn bwd {d.name}{tag}"
    R.assert_bits(name + " dv", c, "dv", dqkv[:, b:], e.dv, **launch)
    if c.hd == 64:
        R.assert_bits(name + " dq", c, "dq", dqkv[:, :a], e.dq, **launch)
    else:
        R.assert_within(name + " dq", c, "dq", dqkv[:, :a], e.dq_ref, R.bf16_ulp(e.dq_ref), **launch)
        _count("dq128", dqkv[:, :a], e.dq_ref)


def check_dk(d, dqkv, tag="", **launch):
    """dk within one bf16 ulp of the reference, exactly zero where the reference is."""
    c, e = d.c, d.exp
    a, b = c.nH * c.hd, (c.nH + c.nKV) * c.hd
    got = dqkv[:, a:b]
    zero = e.dk_ref == 0
    off = got.double().cpu()[zero]
    if off.numel():
        print(f"[attn-exact] dk {d.name}{tag}: {int((off != 0).sum())} of {int(zero.sum())} elements with a zero reference are not zero, "
              f"largest {float(off.abs().max()):.3e}")
    _count("dk", got, e.dk_ref)
    R.assert_within(f"attn bwd {d.name}{tag} dk", c, "dk", got, e.dk_ref, R.bf16_ulp(e.dk_ref), **launch)


def _count(kind, got, ref64):
    n = int((R.bits(got.cpu()) != R.bits((ref64 + 0.0).to(R.F32).to(R.BF16))).sum())
    t = _share.setdefault(kind, [0, 0])
    t[0], t[1] = t[0] + n, t[1] + got.numel()
    print(f"[attn-exact] {kind}: {n} of {got.numel()} elements not bit-equal to bf16(reference); so far {t[0]} of {t[1]} = {t[0] / t[1]:.3e}")


# =============================================================================================== exact cases
def _default_outputs(d):
    """o, lse2 and dqkv of the default launch shape, launched once per case."""
    if not hasattr(d, "out"):
        o, lse = run_fwd(d)
        d.out = (o, lse, run_bwd(d, o, lse))
    return d.out


@pytest.mark.parametrize("cid", R.case_ids(), ids=_id)
def test_exact_forward_backward(cid):
    """o, lse2, dq and dv of every case at the default launch shape; a single KV head runs both key parities."""
    for flip in range(len(R.cases_of(*cid))):
        d = device_case(cid, flip)
        o, lse, dqkv = _default_outputs(d)
        check_fwd(d, o, lse)
        check_bwd(d, dqkv)


@pytest.mark.parametrize("cid", R.case_ids(), ids=_id)
def test_exact_dk(cid):
    """dk of every case at the default launch shape: within one bf16 ulp of the reference, exactly zero where it is zero.

    The zero half is what found the one defect these tests met: every chunk partial of dK is rounded by LN2 at its own magnitude,
    so a key row whose partials cancel (all queries that point at a key carry one code: dk_j = 8 code x sum_i dS_ij) came back
    as 1e-7 .. 1e-6 in 9 of the 24 cases (ragged_1433 (4, 2, 64): 64 of the 53,184 elements with a zero reference, largest
    9.54e-07). attn_dkv_reduce_kernel now also sums the unscaled partials and stores zero where that sum is zero
    (profiles/attn_exact.md)."""
    for flip in range(len(R.cases_of(*cid))):
        d = device_case(cid, flip)
        check_dk(d, _default_outputs(d)[2])


def _launch_shapes(d, check):
    L = lib()
    try:
        for prio, jq, nch in product((0, 1), (1, 2), (1, 2, 3, 4)):
            for k, v in (("attn_prio", prio), ("attn_jq", jq), ("attn_nch", nch)):
                assert L.slam_set_option(None, k.encode(), v) == 0, (k, v)
            check(f" [prio={prio} jq={jq} nch={nch}]", jq, nch)
    finally:
        for k, v in DEFAULT_TUNE.items():
            L.slam_set_option(None, k.encode(), v)


@pytest.mark.parametrize("name", R.LAUNCH_SHAPES)
def test_exact_launch_shapes(name):
    """attn_jq 1 / 2 x attn_nch 1..4 x attn_prio 0 / 1 at head_dim 64: the same bits of o, dq and dv under every launch shape
    (they equal the one expectation), and a second launch bit-identical to the first in every column."""
    d = device_case((name,) + R.HEADS_EVERYWHERE, 0)

    def check(tag, jq, nch):
        o, lse = run_fwd(d, tag)
        check_fwd(d, o, lse, tag)
        dqkv = run_bwd(d, o, lse, tag=tag)
        check_bwd(d, dqkv, tag, nch=nch, jq=jq)
        o2, lse2 = run_fwd(d, tag)
        assert torch.equal(R.bits(o), R.bits(o2)) and torch.equal(R.bits(lse), R.bits(lse2)), f"{tag}: forward not bit-reproducible"
        assert torch.equal(R.bits(dqkv), R.bits(run_bwd(d, o, lse, tag=tag))), f"{tag}: backward not bit-reproducible"

    _launch_shapes(d, check)


@pytest.mark.parametrize("name", R.LAUNCH_SHAPES)
def test_exact_dk_launch_shapes(name):
    """dk under every launch shape stays within its bar (before the reduce kernel's zero rule the four attn_nch = 4 shapes of
    ragged_1433 did not: see test_exact_dk)."""
    d = device_case((name,) + R.HEADS_EVERYWHERE, 0)
    o, lse, _ = _default_outputs(d)
    failures = []

    def check(tag, jq, nch):
        try:
            check_dk(d, run_bwd(d, o, lse, tag=tag), tag, nch=nch, jq=jq)
        except AssertionError as e:
            failures.append(str(e))

    _launch_shapes(d, check)
    assert not failures, f"{len(failures)} of 16 launch shapes; first: {failures[0]}"


@pytest.mark.parametrize("name", ["residue_63", "ragged_1433"])
def test_exact_rotated_backward_with_identity_tables(name):
    """slam_op_attn_bwd_rope with all positions zero (cos = 1, sin = 0) returns the bits of slam_op_attn_bwd in every column."""
    d = device_case((name,) + R.HEADS_EVERYWHERE, 0)
    o, lse, plain = _default_outputs(d)
    rotated = run_bwd(d, o, lse, rope=True)
    check_bwd(d, rotated, " identity rotation")
    bad = R.bits(plain) != R.bits(rotated)
    if bool(bad.any()):
        r, col = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{d.name}: {int(bad.sum())} elements of the rotated backward differ from slam_op_attn_bwd's, first at row {r}, "
                             f"column {col}: {float(rotated[r, col])!r} against {float(plain[r, col])!r}")


# =============================================================================================== deferred-max schedule
_worst_lse = [0.0]


@pytest.mark.parametrize("segments", list(R.SCHEDULE_SEGMENTS))
@pytest.mark.parametrize("profile", list(R.SCHEDULE_PROFILES))
def test_deferred_max_schedule(profile, segments):
    """Forward only (the backward has no running max): key levels that put the running max at its decision points - a tile
    that exceeds it by exactly 8 (stays, P = 256) or by 9 (moves), first visible keys at -250 m, rows of one wave that move
    while their neighbours do not. All weights are powers of two (P is bf16-exact), v is positive: o carries fp32 rounding
    only and must lie within one bf16 ulp of the fp64 value; lse2 within the project's 1e-4 of max(1, |ref|)."""
    c = R.make_schedule_case(profile, segments)
    d = DeviceCase(c, with_backward=False)
    o_ref, lse_ref, _ = _attn_ref64(c.qkv_ref.cuda(), c.d_o.cuda(), c.seg_lens, c.nH, c.nKV, c.hd)
    o_ref, lse_ref = o_ref.cpu(), lse_ref.cpu()
    o, lse = run_fwd(d, f" {profile}")
    name = f"deferred max {profile} {segments}"
    R.assert_within(name + " o", c, "o", o, o_ref, R.bf16_ulp(o_ref))
    got = lse.view(c.nH, c.M).t().double().cpu()
    rel = (got - lse_ref).abs() / lse_ref.abs().clamp_min(1.0)
    _worst_lse[0] = max(_worst_lse[0], float(rel.max()))
    print(f"[attn-exact] {name}: worst lse2 error / max(1, |ref|) = {float(rel.max()):.3e}; so far {_worst_lse[0]:.3e}")
    R.assert_within(name + " lse2", c, "lse2", got, lse_ref, 1e-4 * lse_ref.abs().clamp_min(1.0))
