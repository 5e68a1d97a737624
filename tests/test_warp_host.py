"""CPU tier of slam_sample_tokens_warped (min_p, typical_p, epsilon_cutoff, eta_cutoff behind the device sampler's top-p): the
symbol is declared, exported and bound; it refuses bad arguments before anything reaches the device (fake pointers, as in
test_sampling_host.py); tests/warp_ref.py and UnitLM's torch `_warp` against what transformers' own warpers keep
(tests/golden/warp_hf.npz, make_golden_warp.py); the cap on what the GPU test's 1e-5 band may excuse; the arguments of generate
on a model object that never touches a GPU."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import warp_cases as WC
from tests import warp_ref as W
from tests.test_spec_host import _host_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_hf.npz")
E_INVAL = -1
BAND = 1e-5


def test_symbol_declared_exported_and_bound():
    lib = E.load_library()
    n = "slam_sample_tokens_warped"
    assert n in E.header_symbols() and hasattr(lib, n) and n in lib._slam_signatures
    assert callable(E.sample_tokens_warped)
    assert C.sizeof(E.SlamWarpDesc) == 16 and C.sizeof(E.SlamSampleDesc) == 40
    off = E.SlamWarpDesc()
    assert (off.min_p, off.typical_p, off.epsilon_cutoff, off.eta_cutoff) == (0.0, 1.0, 0.0, 0.0) and not off.active
    assert E.SlamWarpDesc(min_p=0.1).active and E.SlamWarpDesc(typical_p=0.9).active
    assert E.SlamWarpDesc(epsilon_cutoff=1e-3).active and E.SlamWarpDesc(eta_cutoff=1e-3).active


def test_refusals_before_any_launch():
    lib = E.load_library()
    fake, nxt, ws, eos = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22), C.c_void_p(1 << 23)
    B, V = 8, 502
    nws = lib.slam_sample_workspace_bytes(B, V, 25)

    def call(logits=fake, B=B, V=V, use_desc=True, eos_ids=None, nxt=nxt, ws=ws, nws=nws, group=1, out_col=0, warp=(), **kw):
        d = dict(do_sample=1, top_k=25, temperature=0.8, top_p=1.0, seed=11, step=0, pad_id=0, n_eos=0)
        d.update(kw)
        w = C.byref(E.SlamWarpDesc(*warp)) if warp is not None else None
        return lib.slam_sample_tokens_warped(logits, B, V, None, C.byref(E.SlamSampleDesc(**d)) if use_desc else None, None,
                                             eos_ids, None, nxt, None, 0, ws, nws, None, group, out_col, w, None)

    nan = float("nan")
    # the warp description, under sampling and under greedy (which ignores it beyond the range check)
    for ds in (1, 0):
        for v in (-0.1, 1.0001, nan):
            assert call(warp=(v, 1.0, 0.0, 0.0), do_sample=ds) == E_INVAL, v
        for v in (0.0, -0.5, 1.0001, nan):
            assert call(warp=(0.0, v, 0.0, 0.0), do_sample=ds) == E_INVAL, v
        for v in (-1e-3, 1.0, 1.5, nan):
            assert call(warp=(0.0, 1.0, v, 0.0), do_sample=ds) == E_INVAL, v
            assert call(warp=(0.0, 1.0, 0.0, v), do_sample=ds) == E_INVAL, v
    # slam_sample_tokens_at's list holds with a valid description on, with one off and with none
    for warp in ((0.1, 0.9, 1e-3, 1e-3), (0.0, 1.0, 0.0, 0.0), None):
        assert call(warp=warp, logits=None) == E_INVAL
        assert call(warp=warp, use_desc=False) == E_INVAL
        assert call(warp=warp, nxt=None) == E_INVAL
        for b in (0, -1):
            assert call(warp=warp, B=b) == E_INVAL
        assert call(warp=warp, V=0) == E_INVAL
        for k in (0, 257):
            assert call(warp=warp, top_k=k) == E_INVAL
        assert call(warp=warp, do_sample=2) == E_INVAL
        for t in (0.0, nan):
            assert call(warp=warp, temperature=t) == E_INVAL
        for p in (0.0, 1.0001, nan):
            assert call(warp=warp, top_p=p) == E_INVAL
        for n in (-1, 17):
            assert call(warp=warp, n_eos=n, eos_ids=eos) == E_INVAL
        assert call(warp=warp, n_eos=1) == E_INVAL
        assert call(warp=warp, nws=nws - 1) == E_INVAL
        assert call(warp=warp, ws=None) == E_INVAL
        assert call(warp=warp, top_k=26) == E_INVAL  # the workspace was sized for 25: it is slam_sample_tokens_at's
        for g in (0, -1, 3):
            assert call(warp=warp, group=g) == E_INVAL
        assert call(warp=warp, out_col=-1) == E_INVAL


# ---- against transformers' own warpers -------------------------------------------------------------------------------------------
def _golden():
    g = np.load(GOLDEN)
    logits, config = g["logits"], g["config"]
    kept = np.unpackbits(g["kept"], axis=-1)[..., :logits.shape[1]].astype(bool)
    assert logits.shape == (256, 502) and config.shape == (80, 8) and kept.shape == (80, 64, 502)
    return logits, config, kept


def test_golden_covers_the_grid():
    _, config, kept = _golden()
    assert {tuple(c[:3]) for c in config} == {(t, k, p) for t in (0.8, 1.0) for k in (0, 2, 25, 256) for p in (1.0, 0.9)}
    assert {tuple(c[3:7]) for c in config} == {(0.1, 1, 0, 0), (0, 0.9, 0, 0), (0, 1, 3e-3, 0), (0, 1, 0, 3e-3),
                                               (0.05, 0.95, 1e-3, 2e-3)}
    assert kept.any(-1).all()


def test_restatement_keeps_what_hf_keeps():
    """fp32 and fp64 restatements against HF's kept mask on every golden row (top_k >= 1: the contract's range) whose fp64 margin
    exceeds the band."""
    logits, config, kept = _golden()
    judged = total = 0
    for c, (t, k, p, *warp, first) in enumerate(config):
        if k == 0:
            continue
        for r in range(kept.shape[1]):
            x = logits[(int(first) + r) % len(logits)]
            m64, margin = W.kept_mask(x, None, int(k), t, p, warp, fp64=True)
            total += 1
            if margin <= BAND:
                continue
            judged += 1
            assert (m64 == kept[c, r]).all(), (c, r, margin)
            assert (W.kept_mask(x, None, int(k), t, p, warp)[0] == kept[c, r]).all(), (c, r, margin)
    print(f"{judged} of {total} rows judged")
    assert judged >= 0.9 * total


def test_torch_warp_keeps_what_hf_keeps():
    """UnitLM's `_warp` (the torch sampler's chain) on CPU tensors, top_k = 0 included, under the same condition; for top_k = 0
    the margin is that of the chain on all V candidates, which is what the restatement computes for top_k = V."""
    from slamkit_amd.model.unit_lm import _warp
    logits, config, kept = _golden()
    judged = total = 0
    for c, (t, k, p, *warp, first) in enumerate(config):
        rows = (int(first) + np.arange(kept.shape[1])) % len(logits)
        got = torch.isfinite(_warp(torch.from_numpy(logits[rows]), float(t), int(k), float(p), *[float(v) for v in warp])).numpy()
        for r, x in enumerate(logits[rows]):
            margin = W.kept_mask(x, None, int(k) or len(x), t, p, warp, fp64=True)[1]
            total += 1
            if margin <= BAND:
                continue
            judged += 1
            assert (got[r] == kept[c, r]).all(), (c, r, margin)
    assert judged >= 0.9 * total
    x = torch.from_numpy(logits[:4])
    assert torch.equal(_warp(x, 0.8, 25, 0.9), _warp(x, 0.8, 25, 0.9, 0.0, 1.0, 0.0, 0.0))  # off defaults: the positional call


def test_restatement_structure():
    eq = np.full(100, 0.25, dtype=np.float32)
    for warp in WC.WARPS.values():  # all-equal scores: every s and every p ties, nothing may leave
        ids, keep, w, margin = W.chain(eq, None, 25, 0.8, 1.0, warp)
        assert list(ids) == list(range(25)) and keep.all() and (w == 1).all()
    ids, keep, _, _ = W.chain(eq, None, 25, 0.8, 1.0, (1.0, 1.0, 0.0, 0.0))  # min_p = 1 keeps the ties at the top
    assert keep.all()
    x = np.array([5.0, 4.0, 1.0, -30.0, 5.0], dtype=np.float32)
    ids, keep, _, _ = W.chain(x, None, 25, 1.0, 1.0, (1.0, 1.0, 0.0, 0.0))
    assert list(ids[keep]) == [0, 4]
    ids, keep, _, _ = W.chain(x, None, 25, 1.0, 1.0, (0.0, 1.0, 0.9, 0.0))  # epsilon above every p: the top ties stay
    assert list(ids[keep]) == [0, 4]
    ids, keep, _, _ = W.chain(x, None, 1, 1.0, 1.0, (0.0, 0.5, 0.0, 0.0))  # typical_p on k' = 1
    assert list(ids[keep]) == [0]
    # typical_p can drop rank 0: a peaked head over a flat tail has its entropy at the tail's -log p
    x = np.concatenate([[2.0], np.zeros(200)]).astype(np.float32)
    ids, keep, _, _ = W.chain(x, None, 256, 1.0, 1.0, (0.0, 0.5, 0.0, 0.0))
    assert not keep[0] and keep[1:].sum() >= 100
    tok = W.sample_row(x, None, 256, 1.0, 1.0, (0.0, 0.5, 0.0, 0.0), 11, np.arange(8), np.arange(8))
    assert (tok != 0).all()
    assert W.sample_row(np.full(9, -np.inf), None, 25, 1.0, 1.0, WC.WARPS["all"], 11, [0], [0])[0, 0] == -1


@pytest.mark.parametrize("V,B", WC.SHAPES)
def test_band_cap_on_the_gpu_test_inputs(V, B):
    """From the fp64 reference alone: in every configuration of tests/test_gpu_warp.py at most 5 % of the (row, draw) pairs lie
    inside the 1e-5 band."""
    worst = 0.0
    for warp in WC.WARPS:
        for k in WC.TOP_K:
            for p in WC.TOP_P:
                band = WC.reference(V, B, warp, k, p)[1]
                worst = max(worst, float(band.mean()))
                assert band.mean() <= 0.05, (V, B, warp, k, p, float(band.mean()))
    print(f"V {V} B {B}: worst share of draws in the band {worst:.3%}")


# ---- generate's arguments, on a model object that never touches a GPU ---------------------------------------------------------
def test_generate_validates_the_four_arguments():
    m = _host_model()
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), max_new_tokens=4, do_sample=True, top_k=25)
    nan = float("nan")
    for name, bad in (("min_p", (-0.1, 1.5, nan)), ("typical_p", (0.0, -0.2, 1.5, nan)), ("epsilon_cutoff", (-1e-3, 1.0, 2.0, nan)),
                      ("eta_cutoff", (-1e-3, 1.0, 2.0, nan))):
        for v in bad:
            for sampler in (None, "engine"):
                with pytest.raises(ValueError, match=name):
                    m.generate(sampler=sampler, **{name: v}, **kw)
            with pytest.raises(ValueError, match=name):  # the value arrives from generation_config
                m.generate(generation_config=types.SimpleNamespace(**{name: v}), **kw)
        with pytest.raises(ValueError, match=name):  # the explicit argument overrides a valid config
            m.generate(generation_config=types.SimpleNamespace(**{name: 0.5}), **{name: bad[0]}, **kw)
    for typo in ("min_pp", "typical", "epsilon_cutof", "eta_cut_off", "top_h"):
        with pytest.raises(TypeError, match="unsupported arguments"):
            m.generate(**{typo: 0.1}, **kw)
    with pytest.raises(ValueError, match="top_k"):  # the engine sampler's top_k range stays with the warpers on
        m.generate(input_ids=kw["input_ids"], max_new_tokens=4, do_sample=True, top_k=0, min_p=0.1, sampler="engine")
