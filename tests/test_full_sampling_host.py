"""No GPU: generate(sampler="engine_full")'s refusals, the new symbols, the workspace arithmetic, and the cap on the draws that
tests/test_gpu_full_sampling.py may leave out - from the reference alone."""
import os

import pytest
import torch

from slamkit_amd import engine as E
from tests import full_sample_ref as R
from tests.test_spec_host import _host_model


def test_generate_refusals():
    m = _host_model()
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), max_new_tokens=4, sampler="engine_full")
    with pytest.raises(ValueError, match="top_k must be 0.*sampler='engine'"):
        m.generate(do_sample=True, top_k=25, **kw)
    with pytest.raises(ValueError, match="top_k must be 0"):  # the value arrives from generation_config
        m.generate(do_sample=True, generation_config=type("G", (), {"top_k": 50})(), **kw)
    for bad in (dict(typical_p=0.9), dict(eta_cutoff=1e-3)):
        with pytest.raises(ValueError, match="entropy"):
            m.generate(do_sample=True, top_k=0, **bad, **kw)
    with pytest.raises(ValueError, match="engine_full"):
        m.generate(assistant_model=_host_model(), **kw)
    with pytest.raises(ValueError, match="engine_full"):
        m.generate(prompt_lookup_num_tokens=3, **kw)
    with pytest.raises(ValueError, match="temperature"):
        m.generate(do_sample=True, temperature=0.0, **kw)
    with pytest.raises(ValueError, match="engine_full"):  # the engine sampler names the sampler that takes top_k = 0
        m.generate(do_sample=True, top_k=0, **{**kw, "sampler": "engine"})
    with pytest.raises(ValueError, match="engine_full"):
        m.generate(**{**kw, "sampler": "device"})


def test_symbols_and_workspace():
    names = E.header_symbols()
    assert "slam_sample_tokens_full" in names and "slam_sample_full_workspace_bytes" in names
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slam_engine.h")).read()
    assert f"#define SLAM_SAMPLE_FULL_SMALL_MAX {E.SAMPLE_FULL_SMALL_MAX}\n" in hdr
    lib = E.load_library()  # its dynamic symbol table is what exports.map lets through
    assert lib.slam_sample_tokens_full is not None
    small, one_more = E.sample_full_workspace_bytes(8, E.SAMPLE_FULL_SMALL_MAX), E.sample_full_workspace_bytes(8, E.SAMPLE_FULL_SMALL_MAX + 1)
    assert 0 < small < one_more < E.sample_full_workspace_bytes(8, 152167) == 2 * E.sample_full_workspace_bytes(4, 152167)
    for B, V in ((0, 502), (-1, 502), (65536, 502), (8, 0), (8, -5), (8, (1 << 22) + 1)):
        assert E.sample_full_workspace_bytes(B, V) == 0


def test_einval_before_any_launch():
    """Host tensors and stream 0: every refusal comes before anything is launched or dereferenced."""
    x, nxt = torch.zeros(4, 6147), torch.zeros(4, dtype=torch.int64)
    ws = torch.zeros(E.sample_full_workspace_bytes(4, 6147), dtype=torch.uint8)

    def call(desc=None, warp=None, x=x, nxt=nxt, ws=ws, **kw):
        d = E.SlamSampleDesc(do_sample=1, top_k=0, temperature=1.0, top_p=0.9, seed=1, step=0, pad_id=0, n_eos=0)
        for k, v in (desc or {}).items():
            setattr(d, k, v)
        with pytest.raises(E.EngineError, match="invalid argument"):
            E.sample_tokens_full(x, d, nxt, ws, warp, stream=0, **kw)

    for desc in (dict(top_k=1), dict(top_k=1, do_sample=0), dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5),
                 dict(do_sample=2), dict(n_eos=1), dict(n_eos=17)):
        call(desc)
    for warp in (E.SlamWarpDesc(typical_p=0.9), E.SlamWarpDesc(eta_cutoff=1e-3), E.SlamWarpDesc(min_p=1.5),
                 E.SlamWarpDesc(epsilon_cutoff=1.0), E.SlamWarpDesc(min_p=float("nan"))):
        call(warp=warp)
    call(nxt=None)
    call(ws=ws[:-8])
    call(ws=ws[1:])
    call(group=3)
    call(out_col=-1)
    call(x=torch.zeros(4, 0))


@pytest.mark.parametrize("V,B", [(502, 5), (E.SAMPLE_FULL_SMALL_MAX, 5), (E.SAMPLE_FULL_SMALL_MAX + 1, 5), (6147, 5), (152167, 2)])
def test_the_band_leaves_out_at_most_two_percent(V, B):
    x, bn = R.logits(V, B), R.banned(V)
    for setting in R.SETTINGS:
        tok, near = R.sample_rows(x, bn, setting, R.ROW_IDS[:B], range(R.STEPS))
        assert near.mean() <= 0.02, (V, setting, float(near.mean()))
        assert bn[tok[tok >= 0]].sum() == 0 and (tok[B - 1] == -1).all() == (B == 5)  # no banned id; the empty row has no token
