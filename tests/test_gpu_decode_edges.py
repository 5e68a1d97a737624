"""-m gpu: the KV-cached decode path at the shapes and edges generation runs and the other suites do not reach.

 * gemm_skinny, bit for bit: integer operands whose fp32 sums are exact in any order (tests/decode_ref.py), every row tile
   (M 1 .. 130: MT 1 .. 4 and the 64-row grid.z chunks), N and K tails (K % 32 != 0, K % 128 != 0), every epilogue, both
   outputs, and every workspace form (full, limited to two / three splits, one split, none);
 * gemm_skinny at the new row tiles on gaussian operands against fp64, at the bars of test_gemm_skinny_vs_torch;
 * attn_decode for every (head_dim, G) instantiation on a ragged batch (0 .. 1087 keys in one launch, so short rows see
   many empty splits) whose boundary keys are needles: a lost, doubled or misplaced key at 0, pos - 1, pos, a split boundary
   or a wave / slot stride boundary moves a head's output by >= 10 x the per-head tolerance, and every cache row the kernel
   may not read is NaN; workspace-limited split plans; many rows;
 * slam_prefill + slam_decode_step at B = 33 and B = 70 into a cache of NaN, against one full forward and the fp32 oracle."""
import math

import pytest
import torch

from oracle import slam_oracle as O
from tests import decode_ref as R
from tests.gpu_util import lib, ptr, rel_err, stream, sync
from tests.test_gpu_generate import LOGITS_TOL, _mk

pytestmark = pytest.mark.gpu

SKINNY_NK = [(1, 8), (17, 40), (63, 72), (65, 104), (130, 1224), (502, 256), (1000, 2048)]
SKINNY_M = [1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80, 128, 130]
EPILOGUES = [(False, False), (True, False), (True, True)]
SENTINEL = -8192.0  # bf16-exact; fills the guard row / guard words behind a buffer
GUARD = 1024


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _skinny_guarded(X, W, bias, resid, f32, ws, ws_bytes):
    """Y [M][N] of one launch into a NaN-filled buffer followed by a guard row, which must survive."""
    M, K = X.shape
    N = W.shape[0]
    buf = torch.full((M + 1, N), math.nan, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda")
    buf[M] = SENTINEL
    rc = lib().slam_op_gemm_skinny(ptr(X), ptr(W), ptr(buf), int(f32), ptr(bias), ptr(resid), M, N, K, ptr(ws), ws_bytes, stream())
    assert rc == 0, rc
    sync()
    assert bool((buf[M] == SENTINEL).all()), ("guard row overwritten", M, N, K, f32)
    return buf[:M]


def _ws(nbytes):
    """A workspace of exactly nbytes followed by guard words (None for 0 bytes)."""
    if nbytes == 0:
        return None
    assert nbytes % 4 == 0
    w = torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return w


def _ws_guard_ok(w, nbytes):
    return w is None or bool((w[nbytes // 4:] == SENTINEL).all())


def _dev_case(N, K):
    """One integer case at the largest M; smaller M are its leading rows."""
    c = R.skinny_int_case(max(SKINNY_M), N, K, seed=7 * N + K)
    d = {k: c[k].cuda() for k in ("X", "W", "bias", "resid")}
    return c, d


def _exact_dev(c, M, use_bias, use_res):
    sub = dict(xw=c["xw"][:M], bias_i=c["bias_i"], resid_i=c["resid_i"][:M])
    ex = R.skinny_exact(sub, use_bias, use_res)
    return ex.float().cuda(), ex.to(torch.bfloat16).cuda()


def _check_exact(c, d, M, use_bias, use_res, f32, ws, ws_bytes, tag):
    N, K = d["W"].shape
    ex32, ex16 = _exact_dev(c, M, use_bias, use_res)
    X = d["X"][:M]
    b = d["bias"] if use_bias else None
    rs = d["resid"][:M].contiguous() if use_res else None
    Y = _skinny_guarded(X, d["W"], b, rs, f32, ws, ws_bytes)
    want = ex32 if f32 else ex16
    if not torch.equal(_bits(Y), _bits(want)):
        bad = (_bits(Y) != _bits(want)).nonzero()
        raise AssertionError((tag, "M N K", M, N, K, "bias resid f32", use_bias, use_res, f32, "wrong elements", len(bad),
                              "first (m, n)", bad[0].tolist(), "got", float(Y[tuple(bad[0])]), "want", float(want[tuple(bad[0])])))
    Y2 = _skinny_guarded(X, d["W"], b, rs, f32, ws, ws_bytes)
    assert torch.equal(_bits(Y), _bits(Y2)), (tag, M, N, K, "not bit-identical run to run")


@pytest.mark.parametrize("nk", SKINNY_NK, ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_gemm_skinny_exact(nk):
    """fp32 output bit-equal to the exact integer result, bf16 output bit-equal to its one rounding after bias and residual."""
    N, K = nk
    c, d = _dev_case(N, K)
    for M in SKINNY_M:
        nws = lib().slam_op_gemm_skinny_workspace(M, N, K)
        ws = _ws(nws)
        for use_bias, use_res in EPILOGUES:
            for f32 in (True, False):
                _check_exact(c, d, M, use_bias, use_res, f32, ws, nws, "full workspace")
        assert _ws_guard_ok(ws, nws), ("wrote past the workspace", M, N, K)


@pytest.mark.parametrize("nk", SKINNY_NK[-3:], ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_gemm_skinny_workspace_plans(nk):
    """Fewer splits when the partials would not fit, one split when not even two fit or there is no workspace: all exact."""
    N, K = nk
    c, d = _dev_case(N, K)
    for M in (3, 33, 65):
        per = M * N * 4
        full = lib().slam_op_gemm_skinny_workspace(M, N, K)
        assert full % per == 0 and full // per >= 2, (M, N, K, full)  # the full plan splits K, or the rest checks nothing
        for tag, nbytes, alloc in (("full", full, full), ("two splits", 2 * per, 2 * per), ("three splits", 3 * per, 3 * per),
                                   ("one split", per, per), ("no workspace", 0, 0)):
            ws = _ws(alloc)
            for use_bias, use_res in ((False, False), (True, True)):
                for f32 in (True, False):
                    _check_exact(c, d, M, use_bias, use_res, f32, ws, nbytes, tag)
            assert _ws_guard_ok(ws, alloc), ("wrote past the workspace", tag, M, N, K)


@pytest.mark.parametrize("nk", [(1152, 896), (502, 896)], ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_gemm_skinny_new_row_tiles_vs_fp64(nk):
    """The operands of test_gemm_skinny_vs_torch at M 17 .. 130, against fp64, at its bars."""
    N, K = nk
    g = torch.Generator(device="cuda").manual_seed(1)
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.03).to(torch.bfloat16)
    bias = (torch.randn(N, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    worst = {True: 0.0, False: 0.0}
    for M in (17, 33, 49, 65, 130):
        X = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        resid = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
        ref = X.double() @ W.double().t()
        nws = lib().slam_op_gemm_skinny_workspace(M, N, K)
        ws = _ws(nws)
        for use_bias, use_res in EPILOGUES:
            r = ref + (bias.double() if use_bias else 0) + (resid.double() if use_res else 0)
            for f32 in (False, True):
                Y = _skinny_guarded(X, W, bias if use_bias else None, resid if use_res else None, f32, ws, nws)
                e = rel_err(Y, r)
                worst[f32] = max(worst[f32], e)
                assert torch.isfinite(Y.float()).all()
                assert e <= (1e-5 if f32 else 5e-3), (N, K, M, use_bias, use_res, f32, e)
        assert _ws_guard_ok(ws, nws)
    print(f"[parity] gemm_skinny {N}x{K} M 17..130 vs fp64: worst rel_rms fp32 {worst[True]:.3e} bf16 {worst[False]:.3e}")


# ---- attn_decode -----------------------------------------------------------------------------------------------------------
_REFS = {}


def _ref(key, make):
    """(case, reference) computed once per key and left unchanged."""
    if key not in _REFS:
        case = make()
        _REFS[key] = (case, R.case_ref(case))
    return _REFS[key]


def _attn_run(case, kv_bound, ws_bytes):
    """One slam_op_attn_decode into fresh copies of the caches; returns rc, o, k cache, v cache, guard intact."""
    c = case
    B, nH, nKV, hd = c["B"], c["nH"], c["nKV"], c["hd"]
    kc, vc = c["kc"].cuda(), c["vc"].cuda()
    qkv, bias, lens = c["qkv"].cuda(), c["bias"].cuda(), c["lens"].cuda()  # named: they must outlive the launch
    o = torch.full((B, nH * hd), SENTINEL, dtype=torch.bfloat16, device="cuda")
    ws = torch.full((ws_bytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib().slam_op_attn_decode(ptr(qkv), ptr(bias), ptr(lens), ptr(kc), ptr(vc), ptr(o), ptr(ws), ws_bytes, B, nH, nKV,
                                   hd, c["cap"], kv_bound, c["theta"], stream())
    sync()
    return rc, o.cpu(), kc.cpu(), vc.cpu(), bool((ws[ws_bytes:] == 0xA5).all())


def _attn_check(name, case, ref, kv_bound, ws_bytes=None, check_k=False):
    c = case
    B, nH, nKV, hd = c["B"], c["nH"], c["nKV"], c["hd"]
    G = nH // nKV
    o_ref, k_new, v_new = ref
    if ws_bytes is None:
        ws_bytes = lib().slam_op_attn_decode_workspace(B, nH, nKV, hd, kv_bound)
        assert ws_bytes == R.attn_op_workspace(B, nH, nKV, hd, kv_bound), "the restated workspace formula is out of date"
    chunk = R.attn_decode_chunk(B, nH, nKV, hd, kv_bound, ws_bytes - R.attn_op_head(B, hd))
    assert chunk > 0
    rc, o, k1, v1, guard = _attn_run(c, kv_bound, ws_bytes)
    assert rc == 0, (name, rc)
    assert guard, (name, "wrote past the workspace")
    rc2, o2, k2, v2, _ = _attn_run(c, kv_bound, ws_bytes)
    assert rc2 == 0
    assert torch.isfinite(o.float()).all(), (name, "non-finite output: a NaN cache row was read, or an empty split leaked")
    assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(k1), _bits(k2)) and torch.equal(_bits(v1), _bits(v2)), \
        (name, "not bit-identical run to run")
    # per (row, head) relative L2 error
    got = o.double().view(B, nH, hd)
    err = (got - o_ref).norm(dim=-1) / o_ref.norm(dim=-1)
    worst = float(err.max())
    wb, wh = divmod(int(err.argmax()), nH)
    print(f"[parity] attn_decode {name} hd={hd} G={G} nKV={nKV} B={B} chunk={chunk} splits={-(-kv_bound // chunk)}: "
          f"worst per-head rel_l2={worst:.3e} at row {wb} (len {int(c['lens'][wb])}) head {wh}")
    assert worst <= R.ATTN_TOL, (name, "row", wb, "len", int(c["lens"][wb]), "head", wh, worst)
    want_k, want_v = c["kc"].clone(), c["vc"].clone()
    for b in range(B):
        pos = int(c["lens"][b])
        if pos == 0:  # one key: p = 1, l = 1, empty splits add exact zeros
            assert torch.equal(_bits(o[b].view(nKV, G, hd)), _bits(v_new[b][:, None, :].expand(nKV, G, hd).contiguous())), \
                (name, b, "a row with one key must return its V exactly")
        assert torch.equal(_bits(v1[b, :, pos]), _bits(v_new[b])), (name, b, "appended V")
        ek = rel_err(k1[b, :, pos].float(), k_new[b].float())
        assert ek <= 4e-3, (name, b, "appended K", ek)
        if check_k:
            assert float(k_new[b].float().abs().max()) > 0.1  # a gaussian new token: the comparison above means something
        want_k[b, :, pos] = k1[b, :, pos]
        want_v[b, :, pos] = v1[b, :, pos]
    # every other cache element untouched (as integers: NaN != NaN)
    assert torch.equal(_bits(k1), _bits(want_k)) and torch.equal(_bits(v1), _bits(want_v)), \
        (name, "cache rows other than lens[b] changed")
    return worst


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: f"hd{i[0]}-g{i[1]}-kv{i[2]}")
def test_attn_decode_every_instantiation_ragged(inst):
    hd, G, nKV = inst
    B = len(R.RAGGED_LENS)
    chunk = R.attn_decode_chunk(B, G * nKV, nKV, hd, R.RAGGED_BOUND)
    case, ref = _ref(("ragged", hd, G, nKV, chunk), lambda: R.ragged_case(hd, G, nKV, chunk))
    _attn_check("ragged", case, ref, R.RAGGED_BOUND)
    # the same instantiation with a gaussian new token, so that the appended (rotated) K is compared too
    lens = [5, 64, 130]
    plain = R.needle_case(3, G * nKV, nKV, hd, lens, 64, seed=hd + G, new_token_needle=False)
    _attn_check("gaussian-new-token", plain, R.case_ref(plain), max(lens) + 1, check_k=True)


@pytest.mark.parametrize("ws_bound", R.LIMITED_BOUNDS)
@pytest.mark.parametrize("inst", R.LIMITED, ids=lambda i: f"hd{i[0]}-g{i[1]}")
def test_attn_decode_workspace_limited_plans(inst, ws_bound):
    hd, G = inst
    nKV, B = 2, len(R.RAGGED_LENS)
    chunk = R.limited_chunk(hd, G, ws_bound)
    ws_bytes = lib().slam_op_attn_decode_workspace(B, G * nKV, nKV, hd, ws_bound)
    assert ws_bytes == R.attn_op_workspace(B, G * nKV, nKV, hd, ws_bound)
    case, ref = _ref(("ragged", hd, G, nKV, chunk), lambda: R.ragged_case(hd, G, nKV, chunk))
    _attn_check(f"ws-for-{ws_bound}", case, ref, R.RAGGED_BOUND, ws_bytes=ws_bytes)


@pytest.mark.parametrize("inst", R.LIMITED, ids=lambda i: f"hd{i[0]}-g{i[1]}")
def test_attn_decode_refuses_a_workspace_without_room(inst):
    hd, G = inst
    nKV, B = 2, len(R.RAGGED_LENS)
    chunk = R.attn_decode_chunk(B, G * nKV, nKV, hd, R.RAGGED_BOUND)
    case, _ = _ref(("ragged", hd, G, nKV, chunk), lambda: R.ragged_case(hd, G, nKV, chunk))
    head = R.attn_op_head(B, hd)
    one_split = B * G * nKV * (hd + 2) * 4
    for ws_bytes in (head, head + one_split - 4):  # nothing behind the header; not quite one split
        rc, o, k1, v1, guard = _attn_run(case, R.RAGGED_BOUND, ws_bytes)
        assert rc != 0, ws_bytes
        assert guard and bool((o == SENTINEL).all()), "o written by a refused call"
        assert torch.equal(_bits(k1), _bits(case["kc"])) and torch.equal(_bits(v1), _bits(case["vc"]))


@pytest.mark.parametrize("name", list(R.MANY_ROWS))
def test_attn_decode_many_rows(name):
    m = R.MANY_ROWS[name]
    case, ref = _ref(("many", name), lambda: R.many_rows_case(name))
    chunk = R.attn_decode_chunk(m["B"], m["nH"], m["nKV"], m["hd"], m["kv_bound"])
    if name == "b64-mha":
        assert m["B"] * m["nKV"] > 512 and chunk >= m["kv_bound"]  # one split
    _attn_check(name, case, ref, m["kv_bound"])


# ---- prefill + decode at real batch sizes --------------------------------------------------------------------------------
LEN_CYCLE = [1, 2, 62, 63, 64, 65, 127, 128, 129, 200]


@pytest.mark.parametrize("B", [33, 70])
def test_prefill_decode_large_batch_nan_cache(B):
    """B = 33: skinny row tile 3. B = 70: fp32 projections in two 64-row chunks, bf16 projections on gemm_nt. The cache starts
    as NaN, so a read of a row that prefill or an earlier step did not write poisons the logits."""
    cfg = O.TINY
    T, NEW, cap, max_tokens = 200, 4, 256, 16384
    assert B * (T + NEW) <= max_tokens
    sd = O.init_weights(cfg, seed=11, bias_std=0.02, norm_jitter=0.1)
    m = _mk(cfg, sd, max_tokens=max_tokens)
    sd_bf = {k: v.float() for k, v in m.state_dict(torch.bfloat16).items()}
    g = torch.Generator().manual_seed(B)
    lens = [LEN_CYCLE[b % len(LEN_CYCLE)] for b in range(B)]
    rows = [[1] + torch.randint(2, cfg.vocab, (n - 1,), generator=g).tolist() for n in lens]
    given = torch.randint(2, cfg.vocab, (B, NEW), generator=g)
    ids = torch.zeros(B, T, dtype=torch.long)
    full = torch.zeros(B, T + NEW, dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.tensor(r)
        full[b, :len(r)] = torch.tensor(r)
        full[b, len(r):len(r) + NEW] = given[b]
    # the engine's split plan: more than one split at every step, or the test would not reach the merge across splits
    splits = []
    for k in range(NEW):
        chunk = R.attn_decode_chunk(B, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, T + k + 1, max_tokens * cfg.vocab * 2)
        splits.append(-(-(T + k + 1) // chunk))
    assert min(splits) > 1, splits
    dev = m.device
    ids_d, given_d = ids.to(dev).contiguous(), given.to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    cache = torch.full((m.engine.kv_cache_bytes(B, cap),), 0xFF, dtype=torch.uint8, device=dev)  # every bf16 a NaN
    m.engine.bind_kv_cache(cache, B, cap)
    logits = torch.empty(B, cfg.vocab, dtype=torch.float32, device=dev)
    steps = []
    m.engine.prefill(ids_d, lens_d, B, T, logits)
    steps.append(logits.clone())
    for k in range(NEW):
        m.engine.decode_step(given_d[:, k].contiguous(), lens_d, B, logits)
        steps.append(logits.clone())
    sync()
    assert lens_d.tolist() == [n + NEW for n in lens]
    dec = torch.stack(steps, 1).cpu()  # [B][NEW + 1][V]: step k predicts the token after prompt + given[:k]
    assert torch.isfinite(dec).all(), "non-finite logits: a never-written cache row was read"
    fwd = m(input_ids=full).logits.float().cpu()
    worst_f = worst_o = 0.0
    for b, n in enumerate(lens):
        for k in range(NEW + 1):
            e = rel_err(dec[b, k], fwd[b, n - 1 + k])
            worst_f = max(worst_f, e)
            assert e <= LOGITS_TOL, (B, "row", b, "len", n, "step", k, "decode vs forward", e)
    for n in (1, 64, 200):  # the fp32 oracle on three rows
        b = lens.index(n)
        ref = O.model_forward(cfg, sd_bf, full[b:b + 1, :n + NEW])
        for k in range(NEW + 1):
            e = rel_err(dec[b, k], ref[0, n - 1 + k])
            worst_o = max(worst_o, e)
            assert e <= LOGITS_TOL, (B, "row", b, "len", n, "step", k, "decode vs oracle", e)
    print(f"[parity] prefill+decode B={B} T={T} steps={NEW} attention splits per step {splits}: worst per-(row, step) logits "
          f"rel_rms vs forward {worst_f:.3e}, vs fp32 oracle {worst_o:.3e}")
