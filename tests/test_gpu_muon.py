"""optim = "muon" on the GPU: the two batched product kernels to the bit on integer operands, the prepare and apply launches
to the bit against the fp32 restatement of tests/muon_ref.py, the Newton-Schulz door within the measured bar of the float64
restatement, slam_muon_step against the three doors chained, the four test bodies under the trainer's update against an AdamW
run fed the same gradients, and the trainer itself (loss, checkpoints, DPO)."""
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import adafactor_ref as A
from tests import muon_ref as R
from tests.gpu_util import lib, ptr, stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
GUARD = 0x7FC1   # a NaN pattern no kernel produces


def ibits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def to_bf16_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(BF16).to(DEV)


# =============================================================================================== (a) the product kernels
def _strided(mats, stride, front=64):
    """[batch] float arrays -> one bf16 device buffer: `front` guard elements, the matrices at `stride`, every gap a guard."""
    n = mats[0].size
    buf = torch.full((front + len(mats) * stride + front,), GUARD, dtype=torch.int16)
    for i, a in enumerate(mats):
        buf[front + i * stride: front + i * stride + n] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(BF16).view(torch.int16).reshape(-1)
    return buf.to(DEV).view(BF16)


def _check_strided(buf, want, stride, front=64):
    """Every matrix equals `want[i]` to the bit and every guard element is untouched."""
    got = ibits(buf).cpu()
    n = want[0].size
    guard = torch.tensor(GUARD, dtype=torch.int32).to(torch.int16)
    mask = torch.ones(got.numel(), dtype=torch.bool)
    for i, w in enumerate(want):
        lo = front + i * stride
        mask[lo:lo + n] = False
        wb = torch.from_numpy(R.bf16_bits(w)).reshape(-1)
        bad = int((got[lo:lo + n] != wb).sum())
        assert bad == 0, f"matrix {i}: {bad} of {n} elements differ"
    assert bool((got[mask] == guard).all()), "a guard element was written"


@pytest.mark.parametrize("n,m", [(64, 128), (72, 200), (384, 384)])
def test_product_kernels_are_exact_on_integers(n, m):
    """Small-integer operands and power-of-two alpha / beta: every fp32 sum is exact in any order, so the stored bf16 value is the
    one rounding of the exact result. Batch of 3 at strides beyond n m, guard bands around every output; C = C^T to the bit."""
    rng = np.random.default_rng(n * 1000 + m)
    batch, alpha, beta = 3, 0.5, 2.0
    X = [rng.integers(-3, 4, (n, m)).astype(np.float32) for _ in range(batch)]
    Rs = [rng.integers(-8, 9, (n, n)).astype(np.float32) for _ in range(batch)]
    Rs = [np.tril(r) + np.tril(r, -1).T for r in Rs]
    Ps = [rng.integers(-3, 4, (n, n)).astype(np.float32) for _ in range(batch)]
    Rm = [rng.integers(-8, 9, (n, m)).astype(np.float32) for _ in range(batch)]
    sx, sc, sp = n * m + 72, n * n + 136, n * n + 8
    xb, rb, pb, rmb = _strided(X, sx), _strided(Rs, sc), _strided(Ps, sp), _strided(Rm, sx)
    off = lambda t: t[64:]   # noqa: E731 - the first matrix behind the front guard
    # A = X X^T
    cb = _strided([np.zeros((n, n), np.float32)] * batch, sc)
    E.muon_syrk(off(xb), None, off(cb), batch, n, m, sx, 0, sc, 1.0, 0.0)
    torch.cuda.synchronize()
    _check_strided(cb, [x.astype(np.float64) @ x.T for x in X], sc)
    # C = beta R + alpha X X^T
    E.muon_syrk(off(xb), off(rb), off(cb), batch, n, m, sx, sc, sc, alpha, beta)
    torch.cuda.synchronize()
    want = [beta * r + alpha * (x.astype(np.float64) @ x.T) for x, r in zip(X, Rs)]
    _check_strided(cb, want, sc)
    for i in range(batch):
        c = ibits(cb)[64 + i * sc: 64 + i * sc + n * n].view(n, n)
        assert torch.equal(c, c.t()), "C is not symmetric to the bit"
    # Y = beta R + alpha P X
    yb = _strided([np.zeros((n, m), np.float32)] * batch, sx)
    E.muon_mm(off(pb), off(xb), off(rmb), off(yb), batch, n, m, sp, sx, sx, sx, alpha, beta)
    torch.cuda.synchronize()
    _check_strided(yb, [beta * r + alpha * (p.astype(np.float64) @ x) for p, x, r in zip(Ps, X, Rm)], sx)
    E.muon_mm(off(pb), off(xb), None, off(yb), batch, n, m, sp, sx, 0, sx, 2.0, 0.0)
    torch.cuda.synchronize()
    _check_strided(yb, [2.0 * (p.astype(np.float64) @ x) for p, x in zip(Ps, X)], sx)
    _check_strided(xb, X, sx), _check_strided(pb, Ps, sp)      # the inputs are what they were


# =============================================================================================== (b) - (e) a synthetic table
# plain 72 x 200 | transposed 320 x 192 | gate / up interleaved, 64 x 72 each | a gap | the rest of the buffer is never Muon's
SYN = [(0, 72, 200, 0), (14400, 320, 192, 0), (75840, 64, 72, 1), (75840, 64, 72, 2)]
SYN_END = 75840 + 128 * 72


class Syn:
    """The TINY body with the synthetic table set and a guarded workspace bound."""

    def __init__(self, g16):
        from tests.test_gpu_adafactor import body
        self.b = body(g16)
        self.m, self.eng, self.n, self.g16 = self.b.m, self.b.eng, self.b.n, g16
        assert SYN_END + 4096 < self.n
        self.n_mom, self.ws_bytes = self.eng.muon_set_segments(SYN)
        assert self.n_mom == sum(r * c for _, r, c, _ in SYN)
        self.ws_all = torch.full((self.ws_bytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        pad = (-self.ws_all.data_ptr()) % 256
        self.ws = self.ws_all[pad:pad + self.ws_bytes]
        self.ws_guard = self.ws_all[pad + self.ws_bytes:]
        self.eng.muon_bind_workspace(self.ws)
        self.classes = self.eng.muon_classes()
        assert [(c.rows, c.cols, c.n, c.m, c.count) for c in self.classes] == [(72, 200, 72, 200, 1), (320, 192, 192, 320, 1), (64, 72, 64, 72, 2)]
        self.idx = [R.seg_rows(e) for e in SYN]
        cov = np.zeros(self.n, dtype=bool)
        for i in self.idx:
            cov[i.reshape(-1)] = True
        self.cov = cov
        self.mom_off = np.cumsum([0] + [r * c for _, r, c, _ in SYN])

    def close(self):
        self.eng.muon_bind_workspace(None)
        self.eng.muon_set_segments(None)
        self.eng.set_option("adamw_sr", 0)

    def packed_view(self, ci, k):
        """bf16 view [n][m] of matrix k of class ci in the workspace."""
        c = self.classes[ci]
        lo = c.x_byte_offset + k * c.n * c.m * 2
        return self.ws[lo:lo + c.n * c.m * 2].view(BF16).view(c.n, c.m)

    def seg_place(self, si):
        """(class index, index in class) of table row si."""
        return [(0, 0), (1, 0), (2, 0), (2, 1)][si]

    def set_grads(self, g):
        """g: float32 [n] of bf16-exact values, NaN outside the table."""
        t = torch.from_numpy(g)
        if self.g16:
            self.m.flat_grads16.copy_(t.to(BF16))
            self.m.flat_grads.fill_(NAN)
        else:
            self.m.flat_grads.copy_(t)


@pytest.fixture(scope="module", params=[False, True], ids=["g32", "g16"])
def syn(request):
    s = Syn(request.param)
    yield s
    s.close()


def _inputs(s, seed):
    rng = np.random.default_rng(seed)
    g = np.full(s.n, np.nan, np.float32)
    g[s.cov] = R.bf16(rng.standard_normal(int(s.cov.sum())).astype(np.float32) * 0.01)
    mom = (rng.standard_normal(s.n_mom) * 0.01).astype(np.float32)
    p = np.full(s.n, np.nan, np.float32)
    p[s.cov] = (rng.standard_normal(int(s.cov.sum())) * 0.05).astype(np.float32)
    return g, mom, p


def test_prepare_is_the_fp32_restatement(syn):
    """Momentum buffer and packed bf16(U) to the bit - plain, transposed and both interleaved patterns, clip coefficient 0.375,
    from the fp32 buffer and from a bf16 image of the same values, Nesterov on and off; the partials add up to the sum of squares
    (fp32 sums of at most 4096 non-negative terms in a fixed order: within 4096 * 2^-24 relative of the float64 sum)."""
    s = syn
    for nesterov in (True, False):
        g, mom0, _ = _inputs(s, 3)
        s.set_grads(g)
        mom = torch.full((s.n_mom + 64,), NAN, dtype=F32, device=DEV)
        mom[:s.n_mom] = torch.from_numpy(mom0)
        norm_out = torch.tensor([3.0, 0.375], dtype=F32, device=DEV)
        s.eng.op_muon_prepare(mom[:s.n_mom], norm_out, momentum=0.95, nesterov=nesterov, zero_grad=False)
        torch.cuda.synchronize()
        assert bool(torch.isnan(mom[s.n_mom:]).all()) and bool((s.ws_guard == 0xA5).all())
        got_mom = mom[:s.n_mom].cpu().numpy()
        for si, (ent, idx) in enumerate(zip(SYN, s.idx)):
            lo, hi = s.mom_off[si], s.mom_off[si + 1]
            bn, x = R.prepare_f32(g[idx], mom0[lo:hi].reshape(idx.shape), 0.375, 0.95, nesterov)
            assert np.array_equal(got_mom[lo:hi].view(np.int32), bn.reshape(-1).view(np.int32)), f"segment {si}: momentum bits"
            ci, k = s.seg_place(si)
            got = ibits(s.packed_view(ci, k)).cpu().numpy()
            assert np.array_equal(got, R.bf16_bits(R.packed(x))), f"segment {si}: packed bf16(U) bits"
            c = s.classes[ci]
            part = s.ws[c.part_byte_offset + k * c.parts * 4: c.part_byte_offset + (k + 1) * c.parts * 4].view(F32).cpu().numpy().astype(np.float64)
            want = float((x.astype(np.float64) ** 2).sum())
            assert abs(part.sum() - want) <= 4096 * 2.0 ** -24 * want, (si, part.sum(), want)


@pytest.mark.parametrize("shape", [(128, 896), (320, 192), (384, 384), (72, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_schulz_within_the_measured_bar(shape):
    """slam_op_muon_ns on two Gaussian matrices of the shape (packed: transposed when rows > cols) against the float64 restatement,
    each within max(4 s, 2^-8) measured on that very input; a second run gives the same bits."""
    xs = [R.bf16(np.random.default_rng(100 * i + shape[0]).standard_normal(shape).astype(np.float32)) for i in range(2)]
    n, m = min(shape), max(shape)
    stride = n * m + 64
    ws = torch.empty(E.muon_ns_workspace_bytes(2, n, m) + 256, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:]
    runs = []
    for rep in range(2):
        buf = _strided([R.packed(x) for x in xs], stride)
        E.muon_ns(buf[64:], 2, n, m, stride, ws)
        torch.cuda.synchronize()
        runs.append(ibits(buf).cpu().clone())
    assert torch.equal(runs[0], runs[1]), "two runs, different bits"
    guard = torch.tensor(GUARD, dtype=torch.int32).to(torch.int16)
    assert bool((runs[0][:64] == guard).all()) and bool((runs[0][64 + n * m: 64 + stride] == guard).all())
    for i, x in enumerate(xs):
        b, sdist, o = R.bar(x)
        got = runs[0][64 + i * stride: 64 + i * stride + n * m].view(BF16).float().numpy().reshape(n, m)
        d = R.rel_dist(got, R.packed(o))
        print(f"[muon] ns {shape} matrix {i}: distance {d:.3e}, s {sdist:.3e}, bar {b:.3e}")
        assert d <= b, (d, b)


@pytest.mark.parametrize("master", [True, False], ids=["f32-master", "bf16-only"])
def test_apply_is_the_fp32_restatement(syn, master):
    """Given the packed O, the stored parameters to the bit: both adjust_lr modes and none, wd 0 and 0.01, and - bf16-only - the
    stochastic rounding, whose expected bits come from slam_op_sr_round_bf16 at the elements' flat indices."""
    s = syn
    rng = np.random.default_rng(5)
    lr = 1e-3
    for adjust, wd, sr in (("match_rms_adamw", 0.0, False), ("original", 0.01, False), (None, 0.01, False), ("match_rms_adamw", 0.01, True)):
        if sr and master:
            continue
        _, _, p0 = _inputs(s, 9)
        if not master:
            p0 = np.where(s.cov, R.bf16(np.nan_to_num(p0)), np.nan).astype(np.float32)
        o_all = to_bf16_dev(rng.standard_normal(s.n_mom).astype(np.float32) * 0.3)      # packed, class order = table order here
        mt = torch.from_numpy(p0).to(DEV) if master else None
        s.m.flat_params.copy_(torch.full((s.n,), NAN, dtype=BF16) if master else torch.from_numpy(p0).to(BF16))
        s.eng.set_option("adamw_sr", int(sr))
        s.eng.set_option("adamw_sr_seed", 77)
        s.eng.op_muon_apply(mt, o_all, lr, 4, weight_decay=wd, adjust_lr=adjust)
        torch.cuda.synchronize()
        s.eng.set_option("adamw_sr", 0)
        want = np.full(s.n, np.nan, np.float32)
        o_np = o_all.float().cpu().numpy()
        for si, (ent, idx) in enumerate(zip(SYN, s.idx)):
            _, rows, cols, _ = ent
            o = o_np[s.mom_off[si]:s.mom_off[si + 1]].reshape(min(rows, cols), max(rows, cols))
            o = o.T if rows > cols else o
            want[idx] = R.apply_f32(p0[idx], o, lr, wd, adjust, rows, cols)
        w = mt if master else s.m.flat_params
        cov = torch.from_numpy(s.cov).to(DEV)
        assert bool(torch.isnan(w[~cov]).all()) and bool(torch.isnan(s.m.flat_params[~cov]).all()), "an uncovered element was written"
        if master:
            assert np.array_equal(mt.cpu().numpy().view(np.int32)[s.cov], want.view(np.int32)[s.cov]), (adjust, wd)
            assert torch.equal(ibits(s.m.flat_params)[cov], ibits(mt.to(BF16))[cov])
        elif sr:
            y = torch.empty(s.n, dtype=BF16, device=DEV)
            x = torch.from_numpy(np.nan_to_num(want)).to(DEV)
            assert lib().slam_op_sr_round_bf16(ptr(x), ptr(y), s.n, 0, 77, 4, 0, stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(ibits(s.m.flat_params)[cov], ibits(y)[cov]), "stochastic rounding bits"
            assert not torch.equal(ibits(y)[cov], ibits(x.to(BF16))[cov])      # and it is not round-to-nearest
        else:
            assert np.array_equal(ibits(s.m.flat_params).cpu().numpy()[s.cov], R.bf16_bits(want)[s.cov]), (adjust, wd)


@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep-grads", "zero-grads"])
@pytest.mark.parametrize("master", [True, False], ids=["f32-master", "bf16-only"])
def test_step_equals_the_three_doors_chained(syn, master, zero_grad):
    s = syn
    g, mom0, p0 = _inputs(s, 21)
    if not master:
        p0 = np.where(s.cov, R.bf16(np.nan_to_num(p0)), np.nan).astype(np.float32)
    norm_out = torch.tensor([3.0, 0.375], dtype=F32, device=DEV)
    cov = torch.from_numpy(s.cov).to(DEV)
    ws_ns = torch.empty(max(E.muon_ns_workspace_bytes(c.count, c.n, c.m) for c in s.classes) + 256, dtype=torch.uint8, device=DEV)
    ws_ns = ws_ns[(-ws_ns.data_ptr()) % 256:]

    def run(chained):
        s.set_grads(g)
        mom = torch.from_numpy(mom0).to(DEV)
        mt = torch.from_numpy(p0).to(DEV) if master else None
        s.m.flat_params.copy_(torch.full((s.n,), NAN, dtype=BF16) if master else torch.from_numpy(p0).to(BF16))
        g_before = ibits(s.m.flat_grads).clone()
        if chained:
            s.eng.op_muon_prepare(mom, norm_out, momentum=0.95, nesterov=True, zero_grad=zero_grad)
            for c in s.classes:
                x = s.ws[c.x_byte_offset: c.x_byte_offset + c.count * c.n * c.m * 2].view(BF16)
                part = s.ws[c.part_byte_offset: c.part_byte_offset + c.count * c.parts * 4].view(F32)
                E.muon_ns(x, c.count, c.n, c.m, c.n * c.m, ws_ns, partials=part, parts=c.parts)
            s.eng.op_muon_apply(mt, None, 1e-3, 2, weight_decay=0.01, adjust_lr="match_rms_adamw")
        else:
            s.eng.muon_step(mt, mom, norm_out, 1e-3, 2, weight_decay=0.01, zero_grad=zero_grad)
        torch.cuda.synchronize()
        w = mt if master else s.m.flat_params
        assert bool(torch.isnan(w[~cov]).all()) and bool(torch.isnan(s.m.flat_params[~cov]).all()), "an uncovered element was written"
        assert not bool(torch.isnan(w[cov]).any()) and bool((s.ws_guard == 0xA5).all())
        # zero_grad clears the Muon elements of the fp32 buffer, whichever buffer was read, and nothing else
        gb = ibits(s.m.flat_grads)
        assert torch.equal(gb[~cov], g_before[~cov])
        assert (not bool(gb[cov].any())) if zero_grad else torch.equal(gb[cov], g_before[cov])
        return ibits(w).clone(), ibits(s.m.flat_params).clone(), ibits(mom).clone()

    a, b = run(True), run(False)
    for x, y, what in zip(a, b, ("weights", "bf16 parameters", "momentum")):
        assert torch.equal(x[cov] if x.numel() == s.n else x, y[cov] if y.numel() == s.n else y), what
    # and the step moved the weights by about lr_adj per element (an orthogonalised update has entries of order 1 / sqrt(m))
    w = (a[0].view(F32) if master else a[0].view(BF16).float())[cov].cpu().numpy()
    assert 0 < float(np.abs(w - np.nan_to_num(p0)[s.cov]).max()) < 0.05


def test_step_refusals_on_the_device():
    eng = _tiny_model(None, max_tokens=64).engine          # an engine of its own: the table it sets and clears is nobody else's
    mom = torch.zeros(4096, dtype=F32, device=DEV)
    with pytest.raises(E.EngineError, match="segment table"):
        eng.muon_step(None, mom, None, 1e-3, 1)
    n_mom, ws_bytes = eng.muon_set_segments([(0, 64, 64, 0)])
    assert (n_mom, ws_bytes > 0) == (4096, True)
    with pytest.raises(E.EngineError, match="workspace"):
        eng.muon_step(None, mom, None, 1e-3, 1)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:]
    with pytest.raises(E.EngineError, match="too small"):
        eng.muon_bind_workspace(ws[:ws_bytes - 256])
    eng.muon_bind_workspace(ws[:ws_bytes])
    eng.set_option("overlap_adamw", 1)
    with pytest.raises(E.EngineError, match="overlap_adamw"):
        eng.muon_step(None, mom, None, 1e-3, 1)
    eng.set_option("overlap_adamw", 0)
    for kw, word in ((dict(ns_steps=0), "ns_steps"), (dict(ns_steps=17), "ns_steps")):
        with pytest.raises(E.EngineError, match=word):
            eng.muon_step(None, mom, None, 1e-3, 1, **kw)
    with pytest.raises(E.EngineError, match="NULL"):
        eng.muon_step(None, None, None, 1e-3, 1)
    eng.muon_set_segments(None)
    with pytest.raises(E.EngineError, match="segment table"):   # the workspace went with the table
        eng.muon_step(None, mom, None, 1e-3, 1)


# =============================================================================================== (f) the model level
@pytest.mark.parametrize("fam", list(A.FAMILIES))
def test_model_under_muon_against_adamw_and_the_restatement(fam):
    """Three updates of the trainer under optim = "muon" and under "adamw_torch", both fed the same gradients: every non-Muon
    element - fp32 master, bf16 parameter, both moments - has the AdamW run's bits; every Muon matrix lies within the accumulated
    lr_adj * bar * |O_ref| (+ 2^-22 |p| a step for the fp32 roundings of the apply) of the restatement driven by the gradients
    read back from the engine, its momentum buffer has the restatement's bits; the transposed images match the parameters."""
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    base, vocab = A.FAMILIES[fam]

    def make(optim):
        torch.manual_seed(3)
        m = UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(base), vocab_size=vocab, max_tokens=64))
        a = SLAMTrainingArguments(optim=optim, logging_steps=0, max_grad_norm=0.5, weight_decay=0.01, output_dir="/tmp/unused")
        return m, SLAMTrainer(model=m, args=a)

    mm, tm = make("muon")
    ma, ta = make("adamw_torch")
    ma._weights.copy_(mm._weights)
    ma.sync_params_from_master()
    mm.sync_params_from_master()
    n = mm.engine.n_params
    segs = mm.hf_muon_segments()
    idx = [R.seg_rows(s.muon_entry) for s in segs]
    cov = np.zeros(n, dtype=bool)
    for i in idx:
        cov[i.reshape(-1)] = True
    covd = torch.from_numpy(cov).to(DEV)
    p_ref = [mm._weights.cpu().numpy()[i].astype(np.float32) for i in idx]
    bufs = [np.zeros(i.shape, np.float32) for i in idx]
    budget = [0.0] * len(segs)
    lr = 1e-3
    gen = torch.Generator().manual_seed(17)
    for t in range(3):
        g = (torch.randn(n, generator=gen) * 0.02).to(DEV)
        for m in (mm, ma):
            m.engine.set_option("grad_norm_partials", 0)
            m.flat_grads.copy_(g)
        g_back = mm.flat_grads.cpu().numpy()
        tm._clip_and_update(lr, zero_grad=True)
        ta._clip_and_update(lr, zero_grad=True)
        torch.cuda.synchronize()
        cs = float(tm.norm_out[1])
        assert cs == float(ta.norm_out[1]) and 0 < cs < 1
        assert not bool(mm.flat_grads.any())                                   # Muon's elements and the AdamW runs: all cleared
        for k, (s, i) in enumerate(zip(segs, idx)):
            bufs[k], x = R.prepare_f32(g_back[i], bufs[k], np.float32(cs), 0.95, True)
            b, sdist, o = R.bar(x)
            p_ref[k] = R.apply_f32(p_ref[k], o, lr, 0.01, "match_rms_adamw", s.rows, s.cols)
            budget[k] += lr * R.lr_ratio("match_rms_adamw", s.rows, s.cols) * b * float(np.linalg.norm(o)) + 2.0 ** -22 * float(np.linalg.norm(p_ref[k]))
    # the non-Muon elements: AdamW's bits
    assert torch.equal(ibits(mm._weights)[~covd], ibits(ma._weights)[~covd])
    assert torch.equal(ibits(mm.flat_params)[~covd], ibits(ma.flat_params)[~covd])
    for off, cnt, so in tm._adamw_runs:
        assert torch.equal(ibits(tm.exp_avg[so:so + cnt]), ibits(ta.exp_avg[off:off + cnt]))
        assert torch.equal(ibits(tm.exp_avg_sq[so:so + cnt]), ibits(ta.exp_avg_sq[off:off + cnt]))
    assert tm.exp_avg.numel() == n - int(cov.sum()) and float(tm.exp_avg.abs().max()) > 0
    # the Muon matrices
    w = mm._weights.cpu().numpy()
    mom = tm.muon_momentum.cpu().numpy()
    lo = 0
    for k, (s, i) in enumerate(zip(segs, idx)):
        assert np.array_equal(mom[lo:lo + i.size].view(np.int32), bufs[k].reshape(-1).view(np.int32)), f"{s.name}: momentum bits"
        lo += i.size
        d = float(np.linalg.norm(w[i].astype(np.float64) - p_ref[k]))
        print(f"[muon] {fam} {s.name}: |p - p_ref| {d:.3e}, budget {budget[k]:.3e}")
        assert d <= budget[k], (s.name, d, budget[k])
    assert torch.equal(ibits(mm.flat_params), ibits(mm._weights.to(BF16)))
    if mm.flat_params_t is not None:
        # fresh already: an explicit refresh changes no bit; and a layer matrix's image is its transpose
        before = ibits(mm.flat_params_t).clone()
        mm.engine.refresh_transposed()
        torch.cuda.synchronize()
        assert torch.equal(ibits(mm.flat_params_t), before), "the step left a stale transposed image"
        for name, tz in mm.engine.tensors.items():
            if tz.cols > 1 and name.startswith("layers."):
                a, z = tz.offset, tz.offset + tz.rows * tz.cols
                assert torch.equal(ibits(mm.flat_params_t[a:z].view(tz.cols, tz.rows).t().contiguous()), ibits(mm.flat_params[a:z].view(tz.rows, tz.cols))), name


# =============================================================================================== (g) the trainer
def _tiny_model(sd, max_tokens=1024):
    from tests.test_gpu_model import _mk
    return _mk(O.TINY, sd, max_tokens=max_tokens)


def _rows(n, seed, k=40):
    g = torch.Generator().manual_seed(seed)
    return [{"input_ids": [1] + torch.randint(2, 502, (k,), generator=g).tolist(), "attention_mask": [1] * (k + 1)} for _ in range(n)]


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
def test_trainer_loss_goes_down_under_muon(osd):
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    sd = O.init_weights(O.TINY, seed=5, bias_std=0.02, norm_jitter=0.05)
    ds, coll = TokenDataset(_rows(8, 0)), DataCollatorForLanguageModeling(pad_token_id=0)
    a = SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=30, num_train_epochs=30, warmup_steps=2, warmup_ratio=0.0,
                              learning_rate=1e-3, logging_steps=1, max_grad_norm=0.5, weight_decay=0.01, seed=7, output_dir="/tmp/unused",
                              optim="muon", optim_state_dtype=osd)
    m = _tiny_model(sd)
    tr = SLAMTrainer(model=m, args=a, data_collator=coll, train_dataset=ds)
    n_mu = sum(s.rows * s.cols for s in m.hf_muon_segments())
    assert tr.muon_momentum.numel() == n_mu and tr.exp_avg.numel() == m.engine.n_params - n_mu
    assert tr.optimizer_state_bytes[0] == 4 * n_mu + 2 * tr.exp_avg.numel() * tr.exp_avg.element_size()
    state = tr.train()
    losses = [r["loss"] for r in state.log_history if "loss" in r]
    print("muon", osd, [round(x, 3) for x in losses])
    assert state.global_step == 30 and tr.opt_step == 30 and all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses


def test_checkpoint_resume_under_muon(tmp_path):
    """Three steps + checkpoint + resume = the bits of six uninterrupted steps; optimizer.pt holds the kind, the momentum buffer
    and the compact moments; the other kinds refuse it before anything is overwritten."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    sd = O.init_weights(O.TINY, seed=9)
    ds, coll = TokenDataset(_rows(16, 1)), DataCollatorForLanguageModeling(pad_token_id=0)

    def run(max_steps, out, resume=None, save_steps=0, optim="muon"):
        m = _tiny_model(sd)
        a = SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=max_steps, warmup_steps=1, warmup_ratio=0.0, logging_steps=0,
                                  save_steps=save_steps, output_dir=str(out), num_train_epochs=4, optim=optim, weight_decay=0.01)
        tr = SLAMTrainer(model=m, args=a, data_collator=coll, train_dataset=ds)
        tr.train(resume_from_checkpoint=resume)
        return m, tr

    m_full, tr_full = run(6, tmp_path / "a", save_steps=3)
    ck = str(tmp_path / "a" / "checkpoint-3")
    st = torch.load(os.path.join(ck, "optimizer.pt"))
    assert st["optim"] == "muon" and st["opt_step"] == 3 and st["muon_momentum"].numel() == tr_full.muon_momentum.numel()
    assert st["exp_avg"].numel() == tr_full.exp_avg.numel() < m_full.engine.n_params
    m_res, tr2 = run(6, tmp_path / "b", resume=ck)
    assert tr2.state.global_step == 6 and tr2.opt_step == 6
    assert torch.equal(ibits(m_full.flat_params), ibits(m_res.flat_params)) and torch.equal(m_full._weights, m_res._weights)
    assert torch.equal(ibits(tr_full.muon_momentum), ibits(tr2.muon_momentum)) and torch.equal(ibits(tr_full.exp_avg_sq), ibits(tr2.exp_avg_sq))
    for kind in ("adamw_torch", "adafactor"):
        with pytest.raises(ValueError, match="Muon checkpoint"):
            run(6, tmp_path / "c", resume=ck, optim=kind)


def test_dpo_step_under_muon():
    from slamkit_amd.tokeniser import UnitTokeniser
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer
    from tests.test_gpu_dpo import _model, _pairs
    pol = _model(O.init_weights(O.TINY, seed=11, bias_std=0.02), 16 * 256)
    ref = _model(O.init_weights(O.TINY, seed=12, bias_std=0.02), 16 * 256)
    before = pol._weights.clone()
    args = DPOConfig(per_device_train_batch_size=4, beta=0.1, logging_steps=1, max_steps=1, output_dir="/tmp/unused", learning_rate=5e-5,
                     warmup_steps=0, warmup_ratio=0.0, optim="muon")
    tr = SLAMDPOTrainer(model=pol, ref_model=ref, args=args, train_dataset=_pairs(4), processing_class=UnitTokeniser(None, load_fe=False))
    st = tr.train()
    torch.cuda.synchronize()
    assert st.global_step == 1 and tr.opt_step == 1
    assert bool(torch.isfinite(pol._weights).all()) and float((pol._weights != before).float().mean()) > 0.5
    assert float(tr.muon_momentum.abs().max()) > 0
