"""-m gpu: decoding from FP8 weights (slam_quantize_decode_w8, UnitLM.quantize_decode_weights). Everything here is bit-exact.

 * the quantise op against tests/fp8_ref.py: codes (through the dequantise op), the matrix rewritten in place and the
   exponents, on rows made of every tie point between adjacent codes, its bf16 neighbours, the subnormal range, zeros of both
   signs, the exponent thresholds and clamps, random and outlier rows;
 * the private code order read out through the real load path: one-hot X rows return the columns of Wdq;
 * slam_op_gemm_skinny_w8(X, q, e) == slam_op_gemm_skinny(X, Wdq): every row tile, the row tail, split-K with the reduce
   launch, K ranges that start or end in the middle of a 64-deep code block, NaN-poisoned outputs / workspaces / guards;
 * the engine: prefill + decode steps, extend_logits, an extend above 64 rows with the codes valid against the same calls
   after the codes were dropped, the launch counter, parameters and state_dict against fp8_ref;
 * generate (greedy, engine sampler, a quantised draft under assistant_model), invalidation, refusals."""
import math

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import fp8_ref as R
from tests.gpu_util import lib, ptr, stream, sync

pytestmark = pytest.mark.gpu

GUARD = 1024
NAN_CODE = 0x7F  # the guard bytes behind a code array decode to NaN: an over-read that reaches an MFMA poisons the output


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype])


def _guarded(t: torch.Tensor, fill):
    """t on the device at the very end of its allocation's payload, `fill` in GUARD elements on both sides."""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 2 * GUARD,), fill, dtype=t.dtype, device="cuda")
    buf[GUARD:GUARD + flat.numel()] = flat.cuda()
    return buf, buf[GUARD:GUARD + flat.numel()].view(t.shape)


def _guards_hold(buf, n, fill):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool(g.isnan().all()) if isinstance(fill, float) and math.isnan(fill) else bool((g == fill).all())


class W8:
    """One matrix on the device in the op's storage: codes + exponents in one slam_op_w8_bytes allocation between guards."""

    def __init__(self, W: torch.Tensor):
        self.N, self.K = W.shape
        N, K = self.N, self.K
        self.nbytes, self.eoff = lib().slam_op_w8_bytes(N, K), lib().slam_op_w8_exps_offset(N, K)
        assert self.nbytes >= self.eoff + N and self.eoff >= N * K and self.eoff % 256 == 0
        self.buf = torch.full((self.nbytes + 2 * GUARD,), NAN_CODE, dtype=torch.uint8, device="cuda")
        self.codes = self.buf[GUARD:GUARD + N * K]
        self.exps = self.buf[GUARD + self.eoff:GUARD + self.eoff + N]
        self.wbuf, self.W = _guarded(W, math.nan)
        assert self.codes.data_ptr() % 16 == 0 and self.W.data_ptr() % 16 == 0
        assert lib().slam_op_quantize_rows_fp8(ptr(self.W), ptr(self.codes), ptr(self.exps), N, K, stream()) == 0
        sync()

    def untouched_ok(self):
        b, N, K = self.buf, self.N, self.K
        rest = torch.cat([b[:GUARD], b[GUARD + N * K:GUARD + self.eoff], b[GUARD + self.eoff + N:]])
        return bool((rest == NAN_CODE).all()) and _guards_hold(self.wbuf, N * K, math.nan)

    def dequantized(self):
        buf, out = _guarded(torch.zeros(self.N, self.K, dtype=torch.bfloat16), math.nan)
        assert lib().slam_op_dequantize_rows_fp8(ptr(self.codes), ptr(self.exps), ptr(out), self.N, self.K, stream()) == 0
        sync()
        assert _guards_hold(buf, self.N * self.K, math.nan)
        return out


def _value_class_rows(N, K):
    """Rows whose column 0 anchors the exponent (448 2^e: the other columns are then scaled by exactly 2^-e) and whose other
    columns walk through every tie point between adjacent codes, one bf16 ulp either side, and the subnormal range, in both
    signs; then a zero row, a row of negative zeros, threshold / clamp rows, an outlier row, random rows."""
    g = R.e4m3_value(np.arange(0x7F))
    ties = (g[:-1] + g[1:]) / 2
    tb = R.bf16_bits(torch.from_numpy(ties.astype(np.float32)).to(torch.bfloat16))
    near = np.concatenate([R.bits_to_bf16(tb + d).double().numpy() for d in (-1, 0, 1)])
    sub = np.arange(0, 129) * 2.0 ** -13
    pool = np.concatenate([near, g, sub])
    pool = np.concatenate([pool, -pool])
    gen = torch.Generator().manual_seed(N * 1000 + K)
    W = (torch.randn(N, K, generator=gen) * 0.02).double()
    per = K - 1
    n_special = -(-len(pool) // per)
    assert n_special + 8 <= N
    pool = np.concatenate([pool, np.zeros(n_special * per - len(pool))])
    for r in range(n_special):
        e = (0, 5, -20)[r % 3]
        W[r, 0] = 448.0 * 2.0 ** e * (-1 if r % 2 else 1)
        W[r, 1:] = torch.from_numpy(pool[r * per:(r + 1) * per] * 2.0 ** e)
    r = n_special
    W[r] = 0.0
    W[r + 1] = -0.0
    W[r + 2, :3] = torch.tensor([2.0 ** -120, -2.0 ** -125, 2.0 ** -133], dtype=torch.float64)  # the lower clamp
    W[r + 2, 3:] = 0.0
    W[r + 3, :2] = torch.tensor([1.875 * 2.0 ** 127, -2.0 ** 111], dtype=torch.float64)         # e = 120
    W[r + 4, 0] = 30.0                                                                        # an outlier among N(0, 0.02)
    W[r + 5, 0] = 449.0          # the next bf16 above 448 is 450; 449 rounds to 448 (ties to even) - still e = 0
    W[r + 6, 0] = 450.0          # e = 1
    W[r + 7, K - 1] = -224.0     # 1.75 * 2^7: e = -1, at the row's far end
    return W.to(torch.bfloat16)


@pytest.mark.parametrize("K", [64, 192])
def test_quantize_op_matches_the_restatement(K):
    N = 70
    W = _value_class_rows(N, K)
    codes, e, Wdq = R.quantize(W)
    assert set(e.tolist()) >= {-100, -20, -1, 0, 1, 5, 120}
    q = W8(W)
    assert q.untouched_ok(), "the quantise op wrote outside codes, exponents or the matrix"
    assert np.array_equal(q.exps.cpu().numpy().view(np.int8), e)
    assert torch.equal(_bits(q.W.cpu()), _bits(Wdq)), "the matrix rewritten in place"
    assert torch.equal(_bits(q.dequantized().cpu()), _bits(Wdq)), "dequantize(codes, exponents)"
    stored = q.codes.cpu().numpy().reshape(N, K)
    assert not np.isin(stored, (0x7F, 0xFF)).any()
    assert np.array_equal(stored[:, R.code_pos(np.arange(K))], codes), "codes in the engine's order"
    # quantising again changes nothing but, at most, the representation
    q2 = W8(q.W.cpu())
    assert torch.equal(_bits(q2.W.cpu()), _bits(Wdq))


def _skinny(fn, X, wargs, f32, bias, resid, N, nws):
    """One launch into NaN between NaN guards, with a NaN workspace of exactly nws bytes between NaN guards."""
    M, K = X.shape
    ybuf, Y = _guarded(torch.zeros(M, N, dtype=torch.float32 if f32 else torch.bfloat16), math.nan)
    Y.fill_(math.nan)
    wsbuf, ws = (None, None) if nws == 0 else _guarded(torch.zeros(nws // 4, dtype=torch.float32), math.nan)
    if ws is not None:
        ws.fill_(math.nan)
    rc = fn(ptr(X), *[ptr(w) for w in wargs], ptr(Y), int(f32), ptr(bias), ptr(resid), M, N, K, ptr(ws), nws, stream())
    assert rc == 0, rc
    sync()
    assert _guards_hold(ybuf, M * N, math.nan), "wrote outside the output"
    assert wsbuf is None or _guards_hold(wsbuf, nws // 4, math.nan), "wrote outside the workspace"
    return Y


@pytest.mark.parametrize("K", [64, 192])
def test_code_order_read_out_through_the_kernel(K):
    """X = one-hot rows: every output is a single product 1 * Wdq[n][k], so the fp32 result IS column k of Wdq - whatever the
    order of the codes in memory, the kernel's own loads must undo it."""
    N = 70
    q = W8(_value_class_rows(N, K))
    Wdq = q.W.float()
    for c in range(K // 64):
        X = torch.zeros(64, K, dtype=torch.bfloat16)
        X[torch.arange(64), 64 * c + torch.arange(64)] = 1.0
        xbuf, Xd = _guarded(X, math.nan)
        nws = lib().slam_op_gemm_skinny_workspace(64, N, K)
        Y = _skinny(lib().slam_op_gemm_skinny_w8, Xd, (q.codes, q.exps), True, None, None, N, nws)
        assert torch.equal(Y, Wdq[:, 64 * c:64 * c + 64].t()), (K, c)  # == : a product of -0 comes back as +0


_CASES = {}


def _gemm_case(N, K):
    if (N, K) not in _CASES:
        g = torch.Generator().manual_seed(N * 7 + K)
        W = torch.randn(N, K, generator=g) * 0.05
        W[::7, ::13] *= 40  # outliers: the rows differ in their exponent
        W[1] = 0
        q = W8(W.to(torch.bfloat16))
        X = torch.randn(130, K, generator=g).to(torch.bfloat16)
        bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).cuda()
        resid = torch.randn(130, N, generator=g).to(torch.bfloat16)
        _CASES[(N, K)] = (q, X, bias, resid)
    return _CASES[(N, K)]


@pytest.mark.parametrize("K", [64, 192, 4096])
@pytest.mark.parametrize("N", [16, 40, 200])
def test_gemm_skinny_w8_is_gemm_skinny_on_wdq(N, K):
    q, X, bias, resid = _gemm_case(N, K)
    assert len(set(q.exps.tolist())) >= 3
    per = lambda M: M * N * 4  # noqa: E731
    full = lambda M: lib().slam_op_gemm_skinny_workspace(M, N, K)  # noqa: E731
    if (N, K) == (200, 4096):
        assert full(1) == 32 * per(1) and full(64) == 32 * per(64)  # 32 splits: the partial path and the reduce launch run
    runs = [(M, False, True, full(M)) for M in (1, 16, 17, 64)] + [(M, True, False, full(M)) for M in (1, 64, 130)]
    # fewer splits than the plan wants: K ranges of an odd number of 32-deep steps, which start or end inside a code block
    if K == 192:
        runs += [(17, False, True, 2 * per(17)), (3, True, False, 2 * per(3))]        # 3 + 3 steps
    if K == 4096:
        runs += [(5, True, False, 26 * per(5)), (33, False, True, 10 * per(33))]      # 5 and 13 steps per split
    for M, f32, epi, nws in runs:
        xbuf, Xd = _guarded(X[:M], math.nan)  # X, codes and exponents end where their guards begin: an over-read is NaN
        b = bias if epi else None
        rbuf, r = _guarded(resid[:M, :N].contiguous(), math.nan) if epi else (None, None)
        got = _skinny(lib().slam_op_gemm_skinny_w8, Xd, (q.codes, q.exps), f32, b, r, N, nws)
        want = _skinny(lib().slam_op_gemm_skinny, Xd, (q.W,), f32, b, r, N, nws)
        assert not bool(want.isnan().any())
        assert torch.equal(_bits(got), _bits(want)), (M, N, K, f32, nws, int((_bits(got) != _bits(want)).sum()))
    assert q.untouched_ok()


# ---- engine ---------------------------------------------------------------------------------------------------------------
BASE = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=64, intermediate_size=256,
            rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
VOCAB = 502
MODELS = {"qwen2": (dict(BASE), False), "qwen3": (dict(BASE, model_type="qwen3"), False),
          "untied_head": (dict(BASE, tie_word_embeddings=False), True), "tied_head": (dict(BASE), True)}
QUANTISED = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")


def _model(base, seed=3, grads=False, max_tokens=512):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    return UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(base), vocab_size=VOCAB, max_tokens=max_tokens), seed=seed,
                  allocate_grads=grads)


def _trace(m, B):
    """Logits of a prefill + 6 decode steps, an extend_logits of 5 columns and an extend of more than 64 rows; the number of
    FP8 launches of each decode step."""
    g = torch.Generator().manual_seed(11 + B)
    dev, eng = m.device, m.engine
    T0, T1, T2 = 9, 5, 70 // B + 1
    assert B * T1 <= 64 < B * T2
    cap = 128
    cache = torch.empty(eng.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    eng.bind_kv_cache(cache, B, cap)
    ids = torch.randint(2, VOCAB, (B, T0), generator=g).to(dev)
    lens = torch.tensor([T0 - (b % 3) for b in range(B)], dtype=torch.int32, device=dev)
    out, per_step = [], []
    logits = torch.full((B, VOCAB), math.nan, dtype=torch.float32, device=dev)
    eng.prefill(ids, lens, B, T0, logits)
    out.append(logits.clone())
    for _ in range(6):
        tok = torch.randint(2, VOCAB, (B,), generator=g).to(dev)
        c0 = eng.decode_w8_launches()
        eng.decode_step(tok, lens, B, logits)
        per_step.append(eng.decode_w8_launches() - c0)
        out.append(logits.clone())
    allg = torch.full((B, T1, VOCAB), math.nan, dtype=torch.float32, device=dev)
    chunk = torch.randint(2, VOCAB, (B, T1), generator=g).to(dev)
    eng.extend_logits(chunk, torch.full((B,), T1, dtype=torch.int32, device=dev), lens, B, T1, allg)
    out.append(allg)
    big = torch.randint(2, VOCAB, (B, T2), generator=g).to(dev)
    eng.extend(big, torch.full((B,), T2, dtype=torch.int32, device=dev), lens, B, T2, logits)
    out.append(logits.clone())
    sync()
    assert all(bool(torch.isfinite(t).all()) for t in out)
    return out, per_step


@pytest.mark.parametrize("tag", list(MODELS))
def test_engine_same_bits_with_and_without_codes(tag):
    base, head = MODELS[tag]
    m = _model(base)
    L = base["num_hidden_layers"]
    orig = m.state_dict(torch.float32)
    assert m.decode_weights is None and m.engine.decode_w8_state() == 0
    info = m.quantize_decode_weights(include_head=head)
    assert m.decode_weights == "fp8_e4m3" and m.engine.decode_w8_state() == 2
    assert info["dtype"] == "fp8_e4m3" and info["include_head"] is head
    assert set(info["rel_rms"]) == {"wqkv", "wo", "wgu", "wd"} | ({"head"} if head else set())
    assert all(0.01 < v < 0.05 for v in info["rel_rms"].values()), info  # three mantissa bits: 1.8 % .. 3.6 % of a value
    H, I, QKV = 128, 256, 256
    elems = L * (QKV * H + H * H + 2 * I * H + H * I) + (VOCAB * H if head else 0)
    rows = L * (QKV + H + 2 * I + H) + (VOCAB if head else 0)
    assert info["bf16_bytes"] == 2 * elems and info["fp8_bytes"] == elems + rows

    # the parameters (bf16 image and fp32 master) are fp8_ref of the original weights, row by row; the rest did not move
    head_key = "lm.lm_head.weight" if not base["tie_word_embeddings"] else "lm.model.embed_tokens.weight"
    sd16, sd32 = m.state_dict(torch.bfloat16), m.state_dict(torch.float32)
    touched = 0
    for k, w in orig.items():
        if k.endswith(QUANTISED) or (head and k == head_key):
            want = R.quantize(w.to(torch.bfloat16))[2]
            want32 = want.float()
            touched += 1
        else:
            want, want32 = w.to(torch.bfloat16), w  # the master keeps the fp32 values of what was not touched
        assert torch.equal(_bits(sd16[k]), _bits(want)), k
        assert torch.equal(_bits(sd32[k]), _bits(want32)), k
    assert touched == 7 * L + (1 if head else 0)

    per = 4 * L + (1 if head else 0)
    got = {}
    for B in (1, 3):
        got[B], steps = _trace(m, B)
        assert steps == [per] * 6, steps
    assert m.engine.decode_w8_launches() > 2 * 6 * per  # the extend passes of up to 64 rows took the FP8 stream too
    m.drop_decode_weights()
    assert m.decode_weights is None and m.engine.decode_w8_state() == 0 and m.engine.decode_w8_launches() == 0
    for B in (1, 3):
        want, steps = _trace(m, B)
        assert steps == [0] * 6
        for i, (a, b) in enumerate(zip(got[B], want)):
            assert torch.equal(_bits(a), _bits(b)), (tag, B, i)
    # quantising the quantised model changes no parameter
    before = m.flat_params.clone()
    m.quantize_decode_weights(include_head=head)
    assert m.decode_weights == "fp8_e4m3" and torch.equal(_bits(before), _bits(m.flat_params))


def _prompts():
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(2, VOCAB, (3, 12), generator=g)
    am = torch.ones_like(ids)
    am[1, :4] = 0  # left-padded, as the reference calls generate
    ids[1, :4] = 0
    return ids, am


GEN = [dict(do_sample=False), dict(do_sample=True, sampler="engine", top_k=25, temperature=0.8, seed=1234)]


@pytest.mark.parametrize("kw", GEN, ids=["greedy", "engine_sampler"])
def test_generate_same_tokens_with_and_without_codes(kw):
    m = _model(MODELS["untied_head"][0])
    ids, am = _prompts()
    m.quantize_decode_weights(include_head=True)
    a = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=24, eos_token_id=[], pad_token_id=0, **kw).cpu()
    n = m.engine.decode_w8_launches()
    assert n >= 23 * (4 * 2 + 1), n  # no EOS: 23 decode steps behind the prefill, 4 projections a layer + the head
    m.drop_decode_weights()
    b = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=24, eos_token_id=[], pad_token_id=0, **kw).cpu()
    assert m.engine.decode_w8_launches() == 0
    assert torch.equal(a, b)


@pytest.mark.parametrize("kw", GEN, ids=["greedy", "engine_sampler"])
def test_quantised_draft_under_assistant_model(kw):
    m = _model(BASE)
    d = _model(dict(BASE, num_hidden_layers=1), seed=5)
    ids, am = _prompts()
    d.quantize_decode_weights()
    args = dict(input_ids=ids, attention_mask=am, max_new_tokens=24, eos_token_id=1, pad_token_id=0, assistant_model=d,
                num_assistant_tokens=4, **kw)
    a = m.generate(**args).cpu()
    assert d.decode_weights == "fp8_e4m3" and d.engine.decode_w8_launches() >= 4 * 4 and m.engine.decode_w8_launches() == 0
    d.drop_decode_weights()
    b = m.generate(**args).cpu()
    assert d.engine.decode_w8_launches() == 0 and torch.equal(a, b)
    # and the quantised target verifies the draft's proposals through the FP8 stream (K + 1 <= 64 rows per pass)
    m.quantize_decode_weights()
    c = m.generate(**args).cpu()
    assert m.engine.decode_w8_launches() > 0
    m.drop_decode_weights()
    assert torch.equal(c, m.generate(**args).cpu())


def test_parameter_writes_drop_the_codes():
    m = _model(BASE, grads=True)
    orig = m.state_dict(torch.float32)
    m.quantize_decode_weights()
    assert m.decode_weights == "fp8_e4m3"
    m.load_state_dict(orig)
    assert m.decode_weights is None and m.engine.decode_w8_state() == 1
    n0 = m.engine.decode_w8_launches()
    got, steps = _trace(m, 3)
    assert steps == [0] * 6 and m.engine.decode_w8_launches() == n0
    fresh = _model(BASE)
    fresh.load_state_dict(orig)
    want, _ = _trace(fresh, 3)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_bits(a), _bits(b)), ("after load_state_dict", i)

    # one AdamW step: the parameters move, the codes are stale, decode reads the new bf16 parameters
    m.quantize_decode_weights()
    assert m.engine.decode_w8_state() == 2
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(2, VOCAB, (2, 32), generator=g).to(m.device)
    m.zero_grad()
    m(ids, labels=ids)
    m.backward()
    n = m.engine.n_params
    mom, var = (torch.zeros(n, dtype=torch.float32, device=m.device) for _ in range(2))
    norm = torch.zeros(1, dtype=torch.float32, device=m.device)
    m.engine.grad_norm(1.0, norm)
    m.engine.adamw_step(m.flat_master, mom, var, norm, 1e-2, 0.9, 0.95, 1e-8, 0.0, 1)
    m.engine.join()
    assert m.decode_weights is None and m.engine.decode_w8_state() == 1
    n0 = m.engine.decode_w8_launches()
    got, steps = _trace(m, 3)
    assert steps == [0] * 6 and m.engine.decode_w8_launches() == n0
    moved = m.state_dict(torch.float32)
    assert any(not torch.equal(moved[k], orig[k]) for k in orig if k.endswith("o_proj.weight"))
    fresh.load_state_dict(moved)
    want, _ = _trace(fresh, 3)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_bits(a), _bits(b)), ("after AdamW", i)
    # quantising again brings the codes back
    m.quantize_decode_weights()
    _, steps = _trace(m, 1)
    assert steps == [8] * 6


def test_refusals():
    m = _model(BASE)
    with pytest.raises(ValueError, match="dtype"):
        m.quantize_decode_weights(dtype="int8")
    assert m.engine.decode_w8_state() == 0
    W = m.flat_params
    off = m.engine.tensors["layers.1.wd"].offset
    keep = W[off + 5].clone()
    W[off + 5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        m.quantize_decode_weights()
    assert m.engine.decode_w8_state() == 0
    W[off + 5] = keep
    odd = _model(dict(BASE, intermediate_size=160))  # the down projection's K = 160 is no multiple of 64
    with pytest.raises(ValueError, match="multiples of 64"):
        odd.quantize_decode_weights()
    assert odd.engine.decode_w8_state() == 0 and odd.decode_weights is None
    with pytest.raises(E.EngineError, match="multiples of 64"):
        odd.engine.bind_decode_w8(torch.empty(1 << 20, dtype=torch.uint8, device=odd.device))
    ids, am = _prompts()
    assert odd.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, eos_token_id=1, pad_token_id=0).shape[0] == 3
    from slamkit_amd.model import UnitLM, UnitLMConfig
    opt = UnitLM(UnitLMConfig(base_model_name="local-opt", vocab_size=VOCAB, max_tokens=256, base_config=dict(
        model_type="opt", num_hidden_layers=2, hidden_size=128, num_attention_heads=2, ffn_dim=256, max_position_embeddings=64)),
        allocate_grads=False)
    with pytest.raises(ValueError, match="OPT"):
        opt.quantize_decode_weights()
    with pytest.raises(E.EngineError, match="OPT"):
        opt.engine.bind_decode_w8(torch.empty(1 << 20, dtype=torch.uint8, device=opt.device))
    assert opt.engine.decode_w8_state() == 0
