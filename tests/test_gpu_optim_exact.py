"""-m gpu: the optimizer kernels of slamkit_amd/csrc/optimizer.hip through the engine's entry points, held PER ELEMENT to one step
of torch.optim.AdamW in float64 at the rounding bound (tests/optim_exact_ref.py has the reference, the designed inputs, the rule
and the derivation of DELTA_OPT = 2^-20; nothing here widens it):

    fp32 outputs:  |got - ref| <= DELTA_OPT S          bf16 outputs:  bf16_rne(ref - DELTA_OPT S) <= got <= bf16_rne(ref + DELTA_OPT S)

and to bits wherever a statement is exact: the bf16 working copy is the rounded master, every transposed image is the transpose of
the parameters, zero_grad clears the fp32 gradient buffer over exactly the updated elements and leaves the bf16 image alone, a
ranged update leaves every element outside its range alone (the neighbours hold NaN payloads no kernel produces), a second launch
gives the same bits. The gradient norm runs on integer-valued buffers whose chunk sums and norm are exact, the clip coefficient
against its fp32 formula, the conversions on the rounding edges of fp32 -> bf16.

Two bodies, built once per module with and without a final = 2 backward (bf16-kept gradients): O.TINY (widths that are multiples
of 128: the 64 x 128 tile kernels and the all-bf16 x8 tile) and a two-layer body of hidden 192 / intermediate 320 (multiples of
64 only: the 64 x 64 tiles). Which kernel each case reaches and what the runs measured: profiles/optim_exact.md."""
import functools

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import optim_exact_ref as X
from tests import row_exact_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
B192 = O.OracleConfig(n_layers=2, hidden=192, n_heads=3, n_kv_heads=1, head_dim=64, intermediate=320)
CFG = {"tiny": O.TINY, "b192": B192}
MODES = (0, 1, 2)
CLIP_OF_SET = (X.CLIPS[1], 1.0, None, X.CLIPS[1])     # the clip coefficient a hyper-parameter set runs with (None: no norm_out)
WORST = {}                                             # (array, mode) -> worst |got - ref| / S of the fp32 outputs, in 2^-24


def band(dtype):
    b = R.BAND_BITS[dtype]
    return b if dtype == F32 else b - 0x10000 * (b >= 0x8000)


def fill_band(t):
    R.bits(t).fill_(band(t.dtype))


def is_band(t):
    return R.bits(t) == band(t.dtype)


def same_bits(name, a, b):
    bad = R.bits(a) != R.bits(b)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {a.numel()} elements differ in bits, first at flat {int(bad.reshape(-1).nonzero()[0])}"


def same_bits_or_nan(name, a, b):
    bad = (R.bits(a) != R.bits(b)) & ~(torch.isnan(a) & torch.isnan(b))
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {a.numel()} elements differ, first at flat {int(bad.reshape(-1).nonzero()[0])}"


class Body:
    """One model: its layout, the designed inputs per state mode on the device, and one AdamW step in every form."""

    def __init__(self, kind, g16):
        from tests.test_gpu_model import _mk
        cfg = CFG[kind]
        self.kind, self.g16 = kind, g16
        self.m = m = _mk(cfg, None, max_tokens=64)
        self.eng = eng = m.engine
        self.n = n = eng.n_params
        assert m.flat_params_t is not None
        self.layout = X.Layout([(t.name, t.offset, t.rows, t.cols) for t in eng.tensors.values()], n)
        widths = {c for c in self.layout.cols if c > 1}
        assert all(c % 128 == 0 for c in widths) if kind == "tiny" else all(c % 64 == 0 and c % 128 == 64 for c in widths), widths
        if g16:  # where the optimizer reads gradients follows the last backward: a real one that kept its final values in bf16 only
            eng.set_option("grad_norm_partials", 0)    # slam_grad_norm reads the buffer, like the chunk entry points
            ids = torch.randint(2, cfg.vocab, (1, 64), generator=torch.Generator().manual_seed(1))
            ids[:, 0] = 1
            eng.set_option("grad_overwrite_next", 1)
            m(input_ids=ids, labels=ids, return_logits=False)
            m.backward(1.0, final=2)
            torch.cuda.synchronize()
            assert m.flat_grads16 is not None

    @functools.lru_cache(maxsize=None)
    def design(self, mode, nonfinite=True):
        d = X.design(self.layout.ranges, mode, self.g16, seed=mode, nonfinite=nonfinite)
        X.check_design(self.layout.ranges, d)
        return {k: v.to(DEV) for k, v in d.items()}

    def wd_elements(self, flags, wd):
        w = torch.zeros(self.n, dtype=F64)
        for (lo, hi), f in zip(self.layout.ranges, flags):
            w[lo:hi] = wd if f else 0.0
        return w.to(DEV)

    def step(self, mode, hp, path, clip, flags=None, sr=False, zero_grad=True, ranges=None):
        """One launch of the step from the designed state -> the buffers afterwards (clones) and the bits the gradient buffers held
        before. ranges: [(offset, count)] through slam_adamw_range*, everything outside them holding the band's NaN payload."""
        m, eng, n, d = self.m, self.eng, self.n, self.design(mode)
        inside = torch.ones(n, dtype=torch.bool, device=DEV)
        if ranges is not None:
            inside.zero_()
            for o, c in ranges:
                assert not bool(inside[o:o + c].any())
                inside[o:o + c] = True
        md, pd = (F32 if mode == 0 else BF16), (BF16 if mode == 2 else F32)

        def banded(x64, dtype):
            t = x64.to(dtype)
            return torch.where(inside, R.bits(t), torch.full_like(R.bits(t), band(dtype))).view(dtype)
        eng.set_decay_mask(flags)
        eng.set_option("adamw_sr", int(sr))
        eng.set_option("adamw_sr_seed", 1234)
        eng.set_option("fuse_adamw_t", 1 if path in ("fused", "overlap_fused") else 0)
        eng.set_option("overlap_adamw", 1 if path.startswith("overlap") else 0)
        p0 = banded(d["p"], pd)
        master = p0 if mode != 2 else None
        if mode == 2:
            m.flat_params.copy_(p0)
        else:
            fill_band(m.flat_params)
        fill_band(m.flat_params_t)
        ea, eq = banded(d["m"], md), banded(d["v"], md)
        if self.g16:
            m.flat_grads16.copy_(banded(d["g"], BF16))
            fill_band(m.flat_grads)                   # NaN: an update that reads the wrong buffer shows
        else:
            m.flat_grads.copy_(banded(d["g"], F32))
        before = {"grads": m.flat_grads.clone(), "grads16": m.flat_grads16.clone() if self.g16 else None}
        norm_out = None if clip is None else torch.tensor([3.0, clip], dtype=F32, device=DEV)
        args = (norm_out, *hp)
        try:
            if ranges is not None:
                for o, c in ranges:
                    eng.adamw_range(o, c, master, ea, eq, *args, zero_grad=zero_grad)
            elif mode == 2:
                eng.adamw_step_bf16(ea, eq, *args, zero_grad=zero_grad)
            else:
                eng.adamw_step(master, ea, eq, *args, zero_grad=zero_grad)
            eng.join()
            torch.cuda.synchronize()
        finally:
            eng.set_option("overlap_adamw", 0)
            eng.set_option("adamw_sr", 0)
            eng.set_option("fuse_adamw_t", 1)
            eng.set_decay_mask(None)
        out = {"params": m.flat_params.clone(), "params_t": m.flat_params_t.clone(), "m": ea, "v": eq, "grads": m.flat_grads.clone()}
        if mode != 2:
            out["master"] = master
        if self.g16:
            out["grads16"] = m.flat_grads16.clone()
        return out, before, inside

    def case(self, mode, hp, path, flags=None, sr=False, zero_grad=True, ranges=None, clip="of the set"):
        """The step twice (same bits), then every statement of the module docstring about it."""
        clip = CLIP_OF_SET[X.HYPERS.index(hp)] if clip == "of the set" else clip
        tag = (f"{self.kind} mode {mode} {'g16' if self.g16 else 'g32'} set {X.HYPERS.index(hp)} {path}"
               + (" masked" if flags else "") + (" sr" if sr else "") + (f" zero_grad {int(zero_grad)}" if ranges else ""))
        out, before, inside = self.step(mode, hp, path, clip, flags, sr, zero_grad, ranges)
        again, _, _ = self.step(mode, hp, path, clip, flags, sr, zero_grad, ranges)
        for k in out:
            same_bits(f"{tag} {k}: run 1 vs run 2", out[k], again[k])
        d, h = self.design(mode), X.hyper(*hp)
        wd = None if flags is None else self.wd_elements(flags, h["wd"])
        ref = X.adam_ref(d["p"], d["m"], d["v"], d["g"], 1.0 if clip is None else clip, h, lerp=mode == 2, wd=wd)
        if mode == 2 and ranges is None and flags is None:   # the conditions of the designed inputs, on the reference of this very case
            X.check_reference(tag, d, ref, cancel_moves=(clip is not None and clip != 1.0) or hp[1] != .9)
        sel = None if ranges is None else inside.nonzero().reshape(-1)
        cls = d["cls"] if sel is None else d["cls"][sel]
        form = "range" if ranges is not None else "flat" if path in ("flat", "overlap_flat") else "fused"
        for k, arr in (("p", "params" if mode == 2 else "master"), ("m", "m"), ("v", "v")):
            got, (r, S) = out[arr], ref[k]
            if sel is not None:
                assert bool(is_band(got[~inside]).all()), f"{tag} {arr}: an element outside the updated ranges changed"
                got, r, S = got[sel], r[sel], S[sel]
            st = {}
            X.check(f"{tag} {arr}", got, r, S, cls, self.layout, form, sr=sr and got.dtype == BF16, stats=st, index=sel)
            if "worst" in st:
                WORST[(arr, mode)] = max(WORST.get((arr, mode), 0.0), st["worst"])
        if mode != 2:   # the working copy is the round-to-nearest-even of the master the kernel stored (SR leaves it alone)
            want = R.bf16_rne(out["master"].double())
            want = torch.where(inside, want, out["params"])
            same_bits_or_nan(f"{tag}: working copy vs RNE(master)", out["params"], want)
            assert bool(is_band(out["params"][~inside]).all())
        if ranges is None:   # every transposed image is the transpose of the parameters (the flat path refreshes them)
            for name, lo, hi, cols in zip(self.layout.names, self.layout.lo, self.layout.hi, self.layout.cols):
                if cols > 1:
                    rows = (hi - lo) // cols
                    same_bits(f"{tag}: transposed image of {name}", out["params_t"][lo:hi].view(cols, rows).t().contiguous(),
                              out["params"][lo:hi].view(rows, cols))
        # zero_grad: the fp32 buffer is cleared over exactly the updated elements, whichever buffer was read; nothing else moves
        want = torch.where(inside, torch.zeros_like(before["grads"]), before["grads"]) if zero_grad else before["grads"]
        same_bits(f"{tag}: fp32 gradient buffer after zero_grad = {int(zero_grad)}", out["grads"], want)
        if self.g16:
            same_bits(f"{tag}: the bf16 gradient image", out["grads16"], before["grads16"])
        return out


_bodies = {}


def body(kind, g16):
    if (kind, g16) not in _bodies:
        _bodies[(kind, g16)] = Body(kind, g16)
    return _bodies[(kind, g16)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    if WORST:
        print("\n[optim-exact] worst |got - ref| / S of the fp32 outputs in units of 2^-24 (the rule allows 16): "
              + ", ".join(f"{a} mode {m} {w:.2f}" for (a, m), w in sorted(WORST.items())))
    Body.design.cache_clear()
    _bodies.clear()
    torch.cuda.empty_cache()


G = [False, True]
GID = ["g32", "g16"]


# =============================================================================================== AdamW, every form
@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,hp", [("tiny", h) for h in X.HYPERS] + [("b192", X.HYPERS[0]), ("b192", X.HYPERS[3])],
                         ids=[f"tiny-set{i}" for i in range(4)] + ["b192-set0", "b192-set3"])
def test_fused_walk(kind, hp, mode, g16):
    """fuse_adamw_t = 1: every matrix through its tile kernel (64 x 128 and the all-bf16 x8 tile on TINY, 64 x 64 on the 192 body),
    the vectors between them through the strided kernel."""
    body(kind, g16).case(mode, hp, "fused")


@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hp", X.HYPERS, ids=[f"set{i}" for i in range(4)])
def test_flat(hp, mode, g16):
    """fuse_adamw_t = 0: the 8-wide bf16-state kernel (mode 2) or one instance of the strided kernel (modes 0 and 1: the path the
    refactor of profiles/adamw_refactor.md put the fp32 state on), then the separate transpose pass."""
    body("tiny", g16).case(mode, hp, "flat")


def _cut(b):
    """a range of 64 around the first bound between a no-decay and a decayed tensor under the HF flags"""
    flags = b.m.hf_decay_flags()
    i = next(i for i in range(1, len(flags)) if flags[i] != flags[i - 1])
    return b.layout.lo[i] - 24, 64


@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep", "zero"])
@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("mode", MODES)
def test_ranges(mode, g16, zero_grad):
    """slam_adamw_range*: (0, 8), 8 elements that end the buffer, a range that starts and ends inside a block, two adjacent ranges in
    reverse order, a range that cuts a no-decay bound (HF flags set); every element outside keeps the NaN payload it held, in p,
    master, m, v and both gradient buffers; zero_grad clears the fp32 buffer over the ranges and nothing else."""
    b = body("tiny", g16)
    n = b.n
    ranges = [(0, 8), (n - 8, 8), (2048 + 8, 2048 + 16), (8192 + 512, 256), (8192 + 256, 256), _cut(b)]
    b.case(mode, X.HYPERS[3], "flat", flags=b.m.hf_decay_flags(), zero_grad=zero_grad, ranges=ranges)
    b.case(mode, X.HYPERS[1], "flat", zero_grad=zero_grad, ranges=ranges[:5])


@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["flat", "fused", "ranges"])
@pytest.mark.parametrize("which", ["alternating", "hf"])
def test_decay_mask(which, path, mode, g16):
    """slam_set_decay_mask: alternating flags over the tensor list (a bound at every tensor, so the flags differ across the layers
    of a batch) and HF's flags; the reference takes wd per tensor. Set 3: lr wd = 0.01 shows in every storage type."""
    b = body("tiny", g16)
    flags = [i % 2 == 0 for i in range(len(b.layout.names))] if which == "alternating" else b.m.hf_decay_flags()
    assert any(flags) and not all(flags)
    if path == "ranges":
        cut = (b.n // 2) // 8 * 8 + 8
        b.case(mode, X.HYPERS[3], "flat", flags=flags, ranges=[(cut, b.n - cut), (0, cut)], zero_grad=False)
    else:
        b.case(mode, X.HYPERS[3], path, flags=flags)


@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kind,path", [("tiny", "flat"), ("tiny", "fused"), ("b192", "fused")])
def test_stochastic_rounding_stays_between_the_neighbours(kind, path, mode, g16):
    """adamw_sr = 1: every stochastically rounded value (m and v; p too where it is the state) is one of the bf16 neighbours of
    the interval; the master stays under the fp32 rule and its working copy is its round-to-nearest."""
    body(kind, g16).case(mode, X.HYPERS[1], path, sr=True)


@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("path", ["overlap_flat", "overlap_fused"])
def test_overlapped_step(path, g16):
    """overlap_adamw = 1 (fp32 state): the per-layer chunks on the engine's side stream, read after slam_join"""
    body("tiny", g16).case(0, X.HYPERS[1], path)


def test_underflow_class_as_stored():
    """What the kernels store for v' below 2^-126 (|g| = 2^-70, m = v = 0; the rule accepts anything up to 2^-120 there): printed
    for profiles/optim_exact.md, and held to be one of the two fp32 neighbours of the reference (0 or the denormal)."""
    b = body("tiny", False)
    for mode in MODES:
        out = b.case(mode, X.HYPERS[0], "flat", clip=1.0)
        d = b.design(mode)
        u = d["cls"] == X.UNDER
        v = out["v"][u].double()
        ref = X.adam_ref(d["p"], d["m"], d["v"], d["g"], 1.0, X.hyper(*X.HYPERS[0]), lerp=mode == 2)["v"][0][u]
        vals = sorted(set(v.unique().tolist()))
        print(f"[optim-exact] underflow class mode {mode}: reference v' = {float(ref[0]):.4e}, stored {vals}")
        assert bool(((v == 0) | (v == 2.0 ** -149)).all()) if mode == 0 else bool((v == 0).all()), vals


# =============================================================================================== gradient norm and clip
def _norm_both_ways(b, max_norm):
    """{norm, coefficient} and the chunk sums through slam_grad_sumsq_chunks + slam_grad_norm_from_chunks, and through
    slam_grad_norm; the two must agree in bits."""
    eng = b.eng
    chunk, nchunks = eng.grad_chunk_info()
    cs = torch.full((nchunks,), float("nan"), dtype=F32, device=DEV)
    a, c = torch.full((2,), float("nan"), device=DEV), torch.full((2,), float("nan"), device=DEV)
    eng.grad_sumsq_chunks(0, b.n, cs)
    eng.grad_norm_from_chunks(cs, max_norm, a)
    eng.grad_norm(max_norm, c)
    torch.cuda.synchronize()
    same_bits_or_nan("slam_grad_norm vs the chunk entry points", a, c)
    return a.cpu().numpy(), cs.cpu()


def _set_grads(b, g32):
    """g32: fp32 values that are exact in bf16 -> the buffer the engine reads (the fp32 one NaN when that is the bf16 image)"""
    if b.g16:
        b.m.flat_grads16.copy_(g32.to(BF16))
        assert torch.equal(b.m.flat_grads16.float().nan_to_num(7.0), g32.to(DEV).nan_to_num(7.0))
        b.m.flat_grads.fill_(float("nan"))
    else:
        b.m.flat_grads.copy_(g32)


def _chunk_sums_exact(sq_int, unit, chunk):
    """integer squares (in units of `unit`) -> the exact chunk sums"""
    n = sq_int.numel()
    pad = (-n) % chunk
    s = torch.cat([sq_int, torch.zeros(pad, dtype=torch.int64)]).view(-1, chunk).sum(1)
    assert int(s.max()) < 2 ** 24
    return (s.double() * unit).to(F32)


@pytest.mark.parametrize("g16", G, ids=GID)
def test_norm_of_integer_buffers_is_exact(g16):
    b = body("tiny", g16)
    n = b.n
    chunk, nchunks = b.eng.grad_chunk_info()
    assert chunk == X.GRAD_CHUNK and n % chunk != 0 and n % 4 == 0, (n, chunk)
    tail = (nchunks - 1) * chunk
    i = torch.arange(n)
    # all ones: every chunk sum is an integer, the norm is f32(sqrt(n))
    _set_grads(b, torch.ones(n))
    out, cs = _norm_both_ways(b, 1.0)
    same_bits("chunk sums of ones", cs, _chunk_sums_exact(torch.ones(n, dtype=torch.int64), 1.0, chunk))
    assert out[0] == np.float32(np.sqrt(np.float64(n))), (out[0], n)
    assert X.ulp_apart(out[1], X.clip_coef(out[0], 1.0)) <= 1
    # 2^((i % 3) - 1): squares 1/4, 1, 4 - exact in any order of summation
    _set_grads(b, torch.pow(2.0, ((i % 3) - 1).float()))
    out, cs = _norm_both_ways(b, 1.0)
    sq = torch.tensor([1, 4, 16])[i % 3]
    same_bits("chunk sums of 2^((i % 3) - 1)", cs, _chunk_sums_exact(sq, 0.25, chunk))
    assert out[0] == np.float32(np.sqrt(np.float64(int(sq.sum())) / 4.0)), out[0]
    # one 3.0, zeros elsewhere: the norm is exactly 3.0 wherever the element lies
    for at in (0, chunk - 1, chunk, n - 1, tail, n - 4, 16 * chunk - 1, 16 * chunk):
        g = torch.zeros(n)
        g[at] = 3.0
        _set_grads(b, g)
        out, cs = _norm_both_ways(b, 0.0)
        want = torch.zeros(nchunks)
        want[at // chunk] = 9.0
        same_bits(f"chunk sums with one 3.0 at {at}", cs, want)
        assert out[0] == np.float32(3.0) and out[1] == np.float32(1.0), (at, out)


def test_chunk_sums_are_the_same_bits_from_either_buffer():
    """bf16-representable designed values through the fp32 and the bf16 instantiation: the chunk sums are bit-equal, as the comment
    in optimizer.hip promises."""
    a, b = body("tiny", False), body("tiny", True)
    g = X.design(a.layout.ranges, 2, True, seed=9, nonfinite=False)["g"].float()
    _set_grads(a, g)
    _set_grads(b, g)
    oa, ca = _norm_both_ways(a, 0.5)
    ob, cb = _norm_both_ways(b, 0.5)
    same_bits("chunk sums fp32 buffer vs bf16 image", ca, cb)
    assert oa.tobytes() == ob.tobytes()


@pytest.mark.parametrize("g16", G, ids=GID)
def test_norm_zero_nonfinite_and_the_coefficient(g16):
    b = body("tiny", g16)
    n = b.n
    _set_grads(b, torch.zeros(n))
    for mx in (1.0, 0.0, -1.0):
        out, cs = _norm_both_ways(b, mx)
        assert out[0] == 0.0 and out[1] == 1.0 and float(cs.abs().max()) == 0.0, (mx, out)
    for val, norm, coef in ((float("inf"), np.inf, 0.0), (float("-inf"), np.inf, 0.0)):
        g = torch.ones(n)
        g[n // 2 + 3] = val
        _set_grads(b, g)
        out, _ = _norm_both_ways(b, 1.0)
        assert out[0] == norm and out[1] == coef, out
    g = torch.ones(n)
    g[n - 2] = float("nan")
    _set_grads(b, g)
    out, _ = _norm_both_ways(b, 1.0)
    assert np.isnan(out[0]) and np.isnan(out[1]), out
    # the coefficient at norms just below, at and above max_norm: one element x, the norm is |x| up to the rounding of x^2
    equal = True
    for x in (1.0 - 2.0 ** -8, 1.0, 1.0 + 2.0 ** -7, 0.5, 2.0, float(torch.tensor(1e-3).to(BF16)), float(torch.tensor(3e4).to(BF16))):
        for mx in (1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), float(np.nextafter(np.float32(1.0), np.float32(2.0))), 1.0 + 2e-6):
            g = torch.zeros(n)
            g[4097] = x
            _set_grads(b, g)
            out, _ = _norm_both_ways(b, mx)
            want = X.clip_coef(out[0], mx)
            assert abs(float(out[0]) - x) <= 2.0 ** -23 * x
            assert X.ulp_apart(out[1], want) <= 1 and out[1] <= 1.0, (x, mx, out, want)
            equal = equal and out[1] == want
    print(f"[optim-exact] clip coefficient {'bit-equal to' if equal else 'within one ulp of, not always bit-equal to,'} its fp32 formula ({'bf16' if g16 else 'fp32'} buffer)")


@pytest.mark.parametrize("g16", G, ids=GID)
def test_norm_of_designed_gradients_and_sharded_fill(g16):
    """|norm - ref| <= 2e-6 ref against float64 on the designed gradients without the non-finite class (the bar of
    tests/test_gpu_final_grads.py); and a sharded fill - one chunk-aligned range per call, in any order, the tail range last or
    first - equals the whole fill bit for bit."""
    b = body("tiny", g16)
    n = b.n
    g = X.design(b.layout.ranges, 2 if g16 else 0, g16, seed=3, nonfinite=False)["g"]
    _set_grads(b, g.float())
    out, cs = _norm_both_ways(b, 0.5)
    ref = float(g.norm())
    print(f"[optim-exact] designed gradients ({'bf16' if g16 else 'fp32'} buffer): norm {out[0]:.9e} fp64 {ref:.9e} rel err {abs(float(out[0]) - ref) / ref:.3e}")
    assert abs(float(out[0]) - ref) <= 2e-6 * ref
    chunk, nchunks = b.eng.grad_chunk_info()
    cuts = [0, chunk, 17 * chunk, 48 * chunk, (nchunks - 1) * chunk, n]
    pieces = [(lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for order in (pieces, pieces[::-1], pieces[2:] + pieces[:2]):
        sh = torch.full((nchunks,), float("nan"), dtype=F32, device=DEV)
        for o, c in order:
            b.eng.grad_sumsq_chunks(o, c, sh)
        torch.cuda.synchronize()
        same_bits("sharded fill vs whole fill", sh.cpu(), cs)


# =============================================================================================== the rounding behind every store
def _edges():
    """fp32 bit patterns at the rounding edges of fp32 -> bf16"""
    e = []
    for hi in (0x3F80, 0x3F81, 0x0001, 0x0002, 0x007F, 0x0080, 0x7F7E, 0x4049):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):   # ties onto even (hi even) and odd (hi odd), one ulp either side
            e.append((hi << 16) | lo)
    e += [0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x00000000]
    e += [x | 0x80000000 for x in e]
    nan = [0x7FC00000, 0x7FC00001, 0x7F800001, 0x7F80FFFF, 0x7FBFFFFF, 0xFFC00000, 0xFF800001, 0x7FFFFFFF]
    inf = [0x7F800000, 0xFF800000]
    return torch.tensor(e + nan + inf, dtype=torch.int64)


def test_conversions_round_to_nearest_even_on_the_edges():
    """slam_cast_params and slam_pack_grads_bf16 (pack_bf16x2, the rounding behind every optimizer store) on exact ties onto even
    and odd neighbours, one fp32 ulp either side of a tie, 0x7F7FFFFF (rounds to inf), -0.0, fp32 denormals and NaN payloads:
    bit for bit bf16_rne; a NaN only has to stay a NaN."""
    b = body("tiny", False)
    n = b.n
    e = _edges()
    bits32 = e[torch.arange(n) % e.numel()]
    x = torch.where(bits32 >= 2 ** 31, bits32 - 2 ** 32, bits32).to(torch.int32).view(F32).to(DEV)
    want = R.bf16_rne(x.double())
    assert int(torch.isnan(x).sum()) >= 8 and int(torch.isinf(want.float()).sum()) > int(torch.isinf(x).sum())
    fill_band(b.m.flat_params)
    b.eng.cast_params(x)
    torch.cuda.synchronize()
    same_bits_or_nan("slam_cast_params", b.m.flat_params, want)
    b.m.flat_grads.copy_(x)
    for off, cnt in ((0, n), (4, 8), (n - 4, 4), (8188, 1 << 14)):
        dst, chk = R.guarded(cnt, BF16, DEV)
        b.eng.pack_grads_bf16(off, cnt, dst)
        torch.cuda.synchronize()
        chk(f"slam_pack_grads_bf16({off}, {cnt})")
        same_bits_or_nan(f"slam_pack_grads_bf16({off}, {cnt})", dst, want[off:off + cnt])
    same_bits("slam_pack_grads_bf16 left the fp32 buffer alone", b.m.flat_grads, x)
