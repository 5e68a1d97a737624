"""CPU tier: the decode references of tests/decode_ref.py are right, and the inputs of tests/test_gpu_decode_edges.py meet
the conditions its exact and boundary-key claims rest on. No device is touched."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests import decode_ref as R

# the (N, K) and M of the exact gemm_skinny cases of tests/test_gpu_decode_edges.py
SKINNY_NK = [(1, 8), (17, 40), (63, 72), (65, 104), (130, 1224), (502, 256), (1000, 2048)]
SKINNY_M = [1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80, 128, 130]
SENSITIVITY_FACTOR = 10  # a lost boundary key moves a head's output by at least this many tolerances


@pytest.mark.parametrize("nk", SKINNY_NK, ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_skinny_int_case_is_exact_in_fp32(nk):
    N, K = nk
    assert 9 * K + 16 < 2 ** 24
    for M in (1, 17, 130):
        c = R.skinny_int_case(M, N, K, seed=M + N + K)
        for t, lim in ((c["X"], 3), (c["W"], 3), (c["bias"], 8), (c["resid"], 8)):
            assert t.dtype == torch.bfloat16 and float(t.float().abs().max()) <= lim
            assert torch.equal(t.float(), t.float().round())
        ex = R.skinny_exact(c, True, True)
        assert ex.dtype == torch.int64 and int(ex.abs().max()) <= 9 * K + 16
        f32 = c["X"].float() @ c["W"].float().t() + c["bias"].float() + c["resid"].float()
        assert torch.equal(f32.to(torch.int64), ex) and torch.equal(f32, ex.float())
        assert torch.equal(R.skinny_exact(c, False, False), c["xw"])
        # the sum is not trivially small: a dropped K segment or row would show
        if K >= 40:
            assert int(c["xw"].abs().max()) > 8


def _dense(qkv, bias, lens, kc, vc, nH, nKV, hd, theta):
    """Independent formulation: natural-log softmax of ln2 * scores over the cache with the new row appended by torch.cat."""
    B, G = qkv.shape[0], nH // nKV
    x = (qkv.double() + bias.double()).view(B, nH + 2 * nKV, hd)
    cos, sin = O.rope_cos_sin(lens.view(B, 1).long(), hd, theta)  # [B][1][hd]
    q, k = O.apply_rope(x[:, :nH, None], x[:, nH:nH + nKV, None], cos.double(), sin.double())
    q = (q[:, :, 0] * (R.LOG2E / math.sqrt(hd))).float().to(torch.bfloat16).double()
    k = k[:, :, 0].float().to(torch.bfloat16).double()
    v = x[:, nH + nKV:].float().to(torch.bfloat16).double()
    out = []
    for b in range(B):
        p = int(lens[b])
        K = torch.cat([kc[b, :, :p].double(), k[b][:, None]], 1).repeat_interleave(G, 0)  # [nH][p + 1][hd]
        V = torch.cat([vc[b, :, :p].double(), v[b][:, None]], 1).repeat_interleave(G, 0)
        w = F.softmax(math.log(2.0) * torch.einsum("hd,hjd->hj", q[b], K), dim=-1)
        out.append(torch.einsum("hj,hjd->hd", w, V))
    return torch.stack(out), k.to(torch.bfloat16), v.to(torch.bfloat16)


@pytest.mark.parametrize("shape", [(14, 2, 64), (12, 2, 128), (8, 1, 64), (2, 2, 64), (12, 12, 64)], ids=str)
def test_attn_decode_ref_matches_dense_softmax(shape):
    nH, nKV, hd = shape
    lens = [130, 0, 1, 64, 77]
    B, cap = len(lens), 192
    theta = 10000.0 if hd == 64 else 1e6
    g = torch.Generator().manual_seed(nH * hd)
    kc = torch.randn(B, nKV, cap, hd, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, nKV, cap, hd, generator=g).to(torch.bfloat16)
    qkv = torch.randn(B, (nH + 2 * nKV) * hd, generator=g) * 2
    bias = (torch.randn((nH + 2 * nKV) * hd, generator=g) * 0.5).to(torch.bfloat16)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    o, k_new, v_new = R.attn_decode_ref(qkv, bias, lens_t, kc, vc, nH, nKV, hd, theta)
    o2, k2, v2 = _dense(qkv, bias, lens_t, kc, vc, nH, nKV, hd, theta)
    assert o.shape == (B, nH, hd) and o.dtype == torch.float64
    assert float((o - o2).abs().max()) <= 1e-12 * max(1.0, float(o2.abs().max()))
    assert torch.equal(k_new, k2) and torch.equal(v_new, v2)
    # the row with one key: the output is the new V, the same for every head of a group
    assert torch.equal(o[1], v_new[1].double().repeat_interleave(nH // nKV, 0))


def test_needle_case_layout():
    c = R.ragged_case(64, 7, 2, 64)
    assert c["kc"].shape == (8, 2, R.RAGGED_CAP, 64) and c["lens"].tolist() == R.RAGGED_LENS
    for b, pos in enumerate(R.RAGGED_LENS):
        ns = c["needles"][b]
        assert ns == sorted(set(ns)) and ns[0] == 0 and ns[-1] == pos and all(0 <= j <= pos for j in ns)
        for j in (pos - 1, 31, 32, 63, 64, 127, 128, 1023, 1024):
            assert (j in ns) == (0 <= j <= pos)
        assert torch.isnan(c["kc"][b, :, pos:].float()).all() and torch.isnan(c["vc"][b, :, pos:].float()).all()
        assert torch.isfinite(c["kc"][b, :, :pos].float()).all() and torch.isfinite(c["vc"][b, :, :pos].float()).all()
        for r, j in enumerate(ns[:-1]):
            assert (c["kc"][b, :, j] == 0).all()
            want = torch.zeros(64)
            want[r::len(ns)] = R.NEEDLE_C
            assert torch.equal(c["vc"][b, :, j].float(), want.expand(2, 64))
    o, k_new, v_new = R.case_ref(c)
    assert torch.isfinite(o).all()
    assert (k_new == 0).all()  # the new token is a needle: K = 0 after bias and RoPE
    for b in range(8):
        n = len(c["needles"][b])
        want = torch.zeros(64)
        want[n - 1::n] = R.NEEDLE_C
        assert torch.equal(v_new[b].float(), want.expand(2, 64))
    assert R.needle_positions(300, 128, 256) == [0, 15, 16, 63, 64, 255, 256, 299, 300]


def test_chunk_formula_and_limited_plans():
    assert R.attn_decode_chunk(8, 14, 2, 64, R.RAGGED_BOUND) == 64      # 17 splits
    assert R.attn_decode_chunk(8, 12, 12, 64, R.RAGGED_BOUND) == 256   # OPT's 12 / 12 heads: 5 splits
    assert R.attn_decode_chunk(64, 12, 12, 64, 300) == 320             # B nKV > 512: one split
    assert R.attn_decode_chunk(2, 14, 2, 64, 8192) == 64
    for hd, G in R.LIMITED:
        chunks = [R.limited_chunk(hd, G, wb) for wb in R.LIMITED_BOUNDS]
        splits = [-(-R.RAGGED_BOUND // ch) for ch in chunks]
        assert splits[0] == 1 and 1 < splits[1] <= 4 and chunks[2] == 64 and splits[2] == 17, (hd, G, chunks)
        assert R.attn_decode_chunk(8, 2 * G, 2, hd, R.RAGGED_BOUND, 0) == -1


def _sensitivity_cases():
    for hd, G, nKV in R.INSTANCES:
        chunk = R.attn_decode_chunk(len(R.RAGGED_LENS), G * nKV, nKV, hd, R.RAGGED_BOUND)
        yield f"ragged-hd{hd}-g{G}-kv{nKV}", (lambda hd=hd, G=G, nKV=nKV, chunk=chunk: R.ragged_case(hd, G, nKV, chunk))
    for hd, G in R.LIMITED:
        for wb in R.LIMITED_BOUNDS:
            yield f"limited-hd{hd}-g{G}-ws{wb}", (lambda hd=hd, G=G, wb=wb: R.ragged_case(hd, G, 2, R.limited_chunk(hd, G, wb)))
    for name in R.MANY_ROWS:
        yield name, (lambda name=name: R.many_rows_case(name))


_SENS = list(_sensitivity_cases())


@pytest.mark.parametrize("make", [m for _, m in _SENS], ids=[n for n, _ in _SENS])
def test_needles_dominate_the_tolerance(make):
    """A condition on the inputs of the GPU test, not a measurement of the kernel: masking any single needle key changes
    every head's fp64 output by at least 10 x the per-head tolerance."""
    s = R.needle_sensitivity(make())
    print(f"[needle] smallest per-head change when one needle is lost: {s:.3f}")
    assert s >= SENSITIVITY_FACTOR * R.ATTN_TOL, s
