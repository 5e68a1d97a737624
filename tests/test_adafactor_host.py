"""CPU checks of Adafactor (optim = "adafactor"): UnitLM.hf_param_segments() against HF's parameter lists, the float64
restatement of tests/adafactor_ref.py against transformers' own Adafactor in float64 (tests/golden/adafactor_hf_<family>.npz,
written by make_golden_adafactor.py), the acceptance bound of the GPU tests shown to hold for an fp32 emulation of the kernels'
summation orders on the GPU tests' own inputs - zero violations, no element left out -, and every refusal that needs no GPU: the
segment table's argument checks, a step without a table, the trainer's and the arguments' ValueErrors, the checkpoint kinds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import UnitLM, UnitLMConfig
from tests import adafactor_ref as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMS = list(A.FAMILIES)


def host_model(fam):
    """A UnitLM without a GPU: the key map only needs the engine's tensor table."""
    base, vocab = A.FAMILIES[fam]
    cfg = UnitLMConfig(base_model_name="local", base_config=dict(base), vocab_size=vocab)
    m = UnitLM.__new__(UnitLM)
    m.config = cfg
    m.engine = E.Engine(cfg.engine_desc(), *cfg.engine_arch(), flags=cfg.engine_flags())
    m._build_key_map()
    return m


def fixture(fam):
    return np.load(os.path.join(GOLDEN, f"adafactor_hf_{fam}.npz"))


def flat_case(fam):
    """The fixture's run over the engine's flat layout -> (model, segments, table, per-segment wd, p0 [n], [g_t [n]], fixture)"""
    m, fx = host_model(fam), fixture(fam)
    segs = m.hf_param_segments()
    names = [str(x) for x in fx["names"]]
    shapes = {n: tuple(fx[f"p64_{i}"].shape) for i, n in enumerate(names)}
    inputs = A.hf_inputs([(n, shapes[n]) for n in names])
    decay = dict(zip(names, fx["decay"]))
    n = m.engine.n_params
    table = [s.entry for s in segs]
    p0, gs = np.zeros(n), [np.zeros(n) for _ in range(A.HF_STEPS)]
    for s in segs:
        idx = A.seg_index(s.entry)
        p0[idx] = inputs[s.name][0].reshape(idx.shape)
        for t in range(A.HF_STEPS):
            gs[t][idx] = inputs[s.name][1][t].reshape(idx.shape)
    wd = [A.HF_WD if decay[s.name] else 0.0 for s in segs]
    return m, segs, table, wd, p0, gs, fx


# ------------------------------------------------------------------------------------------------ the segments
@pytest.mark.parametrize("fam", FAMS)
def test_segments_are_hfs_parameter_list(fam):
    m, fx = host_model(fam), fixture(fam)
    segs = m.hf_param_segments()
    want = {str(n): tuple(fx[f"p64_{i}"].shape) for i, n in enumerate(fx["names"])}
    assert {s.name: s.shape for s in segs} == want and len(segs) == len(want)   # names and shapes, exactly; a tied head once
    n = m.engine.n_params
    cov = A.covered([s.entry for s in segs], n)                                   # disjoint (asserted inside) and in range
    padded = [m.engine.tensors[k] for k in ("embed", "lm_head") if k in m.engine.tensors]
    # only the pad rows of the token table (and of an untied head) are left out
    assert int((~cov).sum()) == sum(t.numel - m.config.vocab_size * t.cols for t in padded)
    for s in segs:
        assert s.factored == (len(s.shape) == 2) and s.offset % 8 == 0 and s.cols % 8 == 0
        assert (s.rows, s.cols) == (s.shape if s.factored else (1, s.shape[0]))
        assert s.pattern == (1 if "gate_proj" in s.name else 2 if "up_proj" in s.name else 0)
    if fam == "qwen3":
        assert sum("q_norm" in s.name or "k_norm" in s.name for s in segs) == 2
    if fam == "opt":
        assert any("embed_positions" in s.name and s.factored for s in segs) and sum(s.name.endswith("layer_norm.bias") for s in segs) == 3
    if fam == "qwen2_untied":
        assert any(s.name == "lm.lm_head.weight" for s in segs)
    # HF's decay class is one per engine tensor: what lets the step honour slam_set_decay_mask per segment
    flags = dict(zip(m.engine.tensors, m.hf_decay_flags()))
    starts = sorted((t.offset, name) for name, t in m.engine.tensors.items())
    for s, d in zip(segs, [bool(fx["decay"][list(fx["names"]).index(s.name)]) for s in segs]):
        owner = [name for off, name in starts if off <= s.offset][-1]
        assert flags[owner] == d, s.name
    m.engine.close()


# ------------------------------------------------------------------------------------------------ the restatement against HF
@pytest.mark.parametrize("fam", FAMS)
def test_restatement_equals_hf_float64(fam):
    m, segs, table, wd, p, gs, fx = flat_case(fam)
    offs, n_state = A.state_offsets(table)
    state = np.zeros(n_state)
    for t in range(A.HF_STEPS):
        p, state = A.step_f64(p, gs[t], state, table, t + 1, A.HF_LR, cs=A.HF_CS, wd=wd)
    names = [str(x) for x in fx["names"]]
    for s, so in zip(segs, offs):
        i = names.index(s.name)
        # 1e-12 relative to the operands of the final subtraction (|p0| <= 2^-4 here), not to a result in which they cancel
        np.testing.assert_allclose(p[A.seg_index(s.entry)].reshape(s.shape), fx[f"p64_{i}"], rtol=1e-12, atol=1e-12 * 2.0 ** -4, err_msg=s.name)
        if s.factored:
            np.testing.assert_allclose(state[so:so + s.rows], fx[f"row64_{i}"], rtol=1e-12, atol=0, err_msg=s.name)
            np.testing.assert_allclose(state[so + s.rows:so + s.rows + s.cols], fx[f"col64_{i}"], rtol=1e-12, atol=0, err_msg=s.name)
        else:
            np.testing.assert_allclose(state[so:so + s.cols], fx[f"v64_{i}"], rtol=1e-12, atol=0, err_msg=s.name)
    m.engine.close()


# ------------------------------------------------------------------------------------------------ the bound, derived on the host
def _state_violations(got, ref, rel):
    return int((~(np.abs(got.astype(np.float64) - ref) <= rel * np.abs(ref))).sum())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32-master", "bf16-only"])
def test_emulation_meets_the_bound_on_the_synthetic_case(bf16):
    """The inputs of tests/test_gpu_adafactor.py case (a): three steps, each from the stored parameters, every element compared."""
    table, names, n, _ = A.synthetic_table()
    cov = A.covered(table, n)
    _, n_state = A.state_offsets(table)
    p0, gs = A.synthetic_inputs(n, bf16_values=bf16)
    p_st, s32, s64 = p0.astype(np.float32), np.zeros(n_state, np.float32), np.zeros(n_state)
    for t in range(3):
        ref, s64, terms = A.step_f64(p_st.astype(np.float64), gs[t], s64, table, t + 1, A.SYN_LR, cs=A.SYN_CS, wd=A.SYN_WD, want_terms=True)
        got, s32 = A.step_f32_emulated(p_st, gs[t], s32, table, t + 1, A.SYN_LR, cs=A.SYN_CS, wd=A.SYN_WD)
        b, rel = A.bounds(table, t + 1, n, terms, ref)
        assert bool((b[cov] > 0).all())
        if bf16:
            got = A.bf16_rne(got.astype(np.float64)).astype(np.float32)
            assert A.violations_bf16(got, ref, b, cov) == 0, f"step {t + 1}"
        else:
            assert A.violations_f32(got, ref, b, cov) == 0, f"step {t + 1}"
        assert _state_violations(s32, s64, rel) == 0, f"state, step {t + 1}"
        assert np.array_equal(got[~cov], p_st[~cov])
        p_st = got
    # the clip bites on some segments and not on others, and the bound is a rounding bound: far below the update it bounds
    assert (terms[2] > 1.0).any() and (terms[2] == 1.0).any()
    assert float(np.median(b[cov] / np.maximum(terms[0][cov], 1e-300))) < 1e-3


@pytest.mark.parametrize("fam", FAMS)
def test_emulation_meets_the_accumulated_bound_on_the_hf_case(fam):
    """The inputs of case (f): three steps of the emulation's own trajectory against the float64 one, the bounds added up."""
    m, segs, table, wd, p64, gs, fx = flat_case(fam)
    n = m.engine.n_params
    cov = A.covered(table, n)
    _, n_state = A.state_offsets(table)
    p32, s32, s64, total = p64.astype(np.float32), np.zeros(n_state, np.float32), np.zeros(n_state), np.zeros(n)
    for t in range(A.HF_STEPS):
        p64, s64, terms = A.step_f64(p64, gs[t], s64, table, t + 1, A.HF_LR, cs=A.HF_CS, wd=wd, want_terms=True)
        p32, s32 = A.step_f32_emulated(p32, gs[t], s32, table, t + 1, A.HF_LR, cs=A.HF_CS, wd=wd)
        total += A.bounds(table, t + 1, n, terms, p64)[0]
    assert A.violations_f32(p32, p64, total, cov) == 0
    m.engine.close()


def test_bf16_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 0.0, 0.3])
    assert A.bf16_rne(x).tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0]      # ties to even
    lo, hi = A.bf16_floor_ceil(x)
    assert (lo <= x).all() and (x <= hi).all() and (A.bf16_rne(lo) == lo).all() and (A.bf16_rne(hi) == hi).all()
    assert lo[0] == hi[0] == 1.0 and hi[1] == 1.0 + 2.0 ** -7 and lo[3] == -1.0 - 2.0 ** -7


# ------------------------------------------------------------------------------------------------ ABI refusals without a GPU
def _eng():
    return E.Engine(E.SlamModelDesc(2, 64, 1, 1, 64, 128, 502, 0, 1e-6, 10000.0))


def _set(eng, rows):
    buf = (E.SlamAdafactorSegment * len(rows))(*[E.SlamAdafactorSegment(*r) for r in rows])
    return eng.lib.slam_adafactor_set_segments(eng.h, buf, len(rows)), (eng.lib.slam_last_error(eng.h) or b"").decode()


def test_segment_table_argument_checks():
    eng = _eng()
    n = eng.n_params
    for rows, word in (([(0, 64, 64, 1, 0), (64 * 63, 8, 64, 1, 0)], "overlap"),          # the second starts inside the first
                       ([(0, 64, 64, 1, 1), (64 * 64, 32, 64, 1, 0)], "overlap"),          # a contiguous block over the second phase-0 group
                       ([(n - 64, 2, 64, 1, 0)], "out of range"),
                       ([(0, 64, 64, 1, 2)], None),                                        # phase 32: rows 32 .. 63 and 96 .. 127 - in range
                       ([(n - 64 * 64, 64, 64, 1, 1)], "out of range"),                    # the groups of a pattern span twice the rows
                       ([(-8, 1, 8, 0, 0)], "out of range"),
                       ([(4, 1, 8, 0, 0)], "misaligned"), ([(0, 8, 12, 1, 0)], "misaligned"),
                       ([(0, 0, 8, 1, 0)], "positive"), ([(0, 2, 8, 0, 0)], "vector"), ([(0, 48, 8, 1, 1)], "groups of 32"),
                       ([(0, 8, 8, 1, 3)], "pattern"), ([(0, 8, 8, 2, 0)], "factored")):
        rc, msg = _set(eng, rows)
        if word is None:
            assert rc != -1, msg   # a valid table passes the checks (what follows is the upload, which needs a device)
        else:
            assert rc == -1 and word in msg, (rows, rc, msg)
    assert eng.lib.slam_adafactor_set_segments(eng.h, None, 3) == -1
    assert eng.lib.slam_adafactor_set_segments(None, None, 0) == -1
    assert eng.lib.slam_adafactor_set_segments(eng.h, None, 0) == 0    # clearing an empty table
    eng.close()


def test_step_and_sizes_without_a_table_are_refused():
    eng = _eng()
    lib = eng.lib
    one = C.c_void_p(8)  # never dereferenced: every refusal comes before a launch
    rc = lib.slam_adafactor_step(eng.h, None, one, None, 1e-3, 1e-30, 1.0, -0.8, 0.0, 1, 0, None)
    assert rc == -2 and b"segment table" in lib.slam_last_error(eng.h)       # SLAM_ESTATE
    a, b = C.c_int64(0), C.c_size_t(0)
    assert lib.slam_adafactor_sizes(eng.h, C.byref(a), C.byref(b)) == -2
    assert lib.slam_adafactor_bind_workspace(eng.h, one, 1 << 20) == -2
    assert lib.slam_adafactor_bind_workspace(eng.h, None, 0) == 0             # NULL unbinds
    assert lib.slam_adafactor_step(None, None, one, None, 1e-3, 1e-30, 1.0, -0.8, 0.0, 1, 0, None) == -1
    with pytest.raises(E.EngineError, match="segment table"):
        eng.adafactor_sizes()
    eng.close()


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "slam_engine.h")).read()
    lib = E.load_library()
    for name in ("slam_adafactor_set_segments", "slam_adafactor_sizes", "slam_adafactor_bind_workspace", "slam_adafactor_step"):
        assert name in E.header_symbols() and name in lib._slam_signatures and hasattr(lib, name)
    assert re.search(r"int slam_adafactor_step\(SlamEngine\* h, float\* master_f32, float\* state_f32, const float\* norm_out, double lr, "
                     r"double eps1,\s+double clip_threshold, double decay_rate, double weight_decay, int32_t step, int32_t zero_grad,\s+"
                     r"slam_stream_t stream\);", hdr)
    assert C.sizeof(E.SlamAdafactorSegment) == 24
    assert list(lib.slam_adafactor_step.argtypes) == [C.c_void_p] * 4 + [C.c_double] * 5 + [C.c_int32] * 2 + [C.c_void_p]


# ------------------------------------------------------------------------------------------------ arguments, trainer, checkpoints
class _Recorder:
    def __init__(self, inner):
        self.inner, self.calls = inner, []
        self.n_params = inner.n_params

    def __getattr__(self, k):
        if k.startswith("adafactor"):
            def rec(*a, **kw):
                self.calls.append(k)
                return (16, 64) if k == "adafactor_set_segments" else None
            return rec
        return getattr(self.inner, k)


def _stub_trainer(**kw):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import StubLM
    model = StubLM()
    model.engine = _Recorder(model.engine)
    model.hf_param_segments = lambda: []
    model._weights, model.sync_params_from_master = model.flat_master, lambda: None   # what a checkpoint touches
    return SLAMTrainer(model=model, args=SLAMTrainingArguments(logging_steps=0, **kw)), model


def test_optim_argument():
    from slamkit_amd.trainer import DPOConfig, SLAMTrainingArguments
    assert SLAMTrainingArguments().optim == "adamw_torch" and DPOConfig(optim="adafactor").optim == "adafactor"
    for ok in ("adamw_torch", "adamw_torch_fused", "adafactor"):
        assert SLAMTrainingArguments(optim=ok).optim == ok
    with pytest.raises(ValueError, match="adamw_torch.*adamw_torch_fused.*adafactor"):
        SLAMTrainingArguments(optim="adamw_8bit")


def test_adamw_names_make_no_adafactor_call():
    for name in ("adamw_torch", "adamw_torch_fused"):
        tr, model = _stub_trainer(optim=name)
        assert model.engine.calls == [] and tr.exp_avg is not None and tr.exp_avg_sq is not None and not hasattr(tr, "adafactor_state")


def test_trainer_under_adafactor_and_its_refusals():
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import StubLM
    tr, model = _stub_trainer(optim="adafactor")
    assert model.engine.calls == ["adafactor_set_segments", "adafactor_bind_workspace"]   # the table once, then the workspace
    assert tr.exp_avg is None and tr.exp_avg_sq is None and tr.adafactor_state.numel() == 16
    for kw, word in ((dict(optim_state_dtype="float32_bf16_moments"), "moments"), (dict(ddp_algo="rs_ag"), "rs_ag"),
                     (dict(overlap_optimizer=True), "overlap_optimizer")):
        with pytest.raises(ValueError, match=word):
            _stub_trainer(optim="adafactor", **kw)
    args = SLAMTrainingArguments(logging_steps=0)
    args.optim = "sgd"   # a field set after construction gets past the arguments' own check: the trainer checks again
    with pytest.raises(ValueError, match="optim must be"):
        SLAMTrainer(model=StubLM(), args=args)
    args.optim = "adafactor"
    with pytest.raises(ValueError, match="hf_param_segments"):
        SLAMTrainer(model=StubLM(), args=args)   # a model that cannot name its HF tensors


def test_checkpoint_kind_mismatch_is_an_error(tmp_path):
    import torch
    from slamkit_amd.trainer.slam_trainer import check_checkpoint_optim
    adam = {"master": 0, "exp_avg": 0, "exp_avg_sq": 0, "opt_step": 3}
    fact = {"master": 0, "optim": "adafactor", "adafactor_state": 0, "opt_step": 3}
    check_checkpoint_optim(adam, False)
    check_checkpoint_optim(fact, True)
    with pytest.raises(ValueError, match="AdamW checkpoint"):
        check_checkpoint_optim(adam, True)
    with pytest.raises(ValueError, match="Adafactor checkpoint"):
        check_checkpoint_optim(fact, False)
    # through the trainer: an AdamW run's optimizer.pt under optim = "adafactor", before anything is overwritten
    tr, model = _stub_trainer(optim="adamw_torch", output_dir=str(tmp_path))
    tr.save_checkpoint()
    path = tr._ckpt_dir(0)
    assert set(torch.load(os.path.join(path, "optimizer.pt"))) == {"master", "exp_avg", "exp_avg_sq", "opt_step"}  # AdamW's file is what it was
    tr2, model2 = _stub_trainer(optim="adafactor", output_dir=str(tmp_path))
    before = model2.flat_master.clone()
    with pytest.raises(ValueError, match="AdamW checkpoint"):
        tr2._load_checkpoint(path)
    assert torch.equal(model2.flat_master, before)
    tr2.save_checkpoint()
    st = torch.load(os.path.join(path, "optimizer.pt"))
    assert st["optim"] == "adafactor" and st["adafactor_state"].numel() == 16 and "exp_avg" not in st
    with pytest.raises(ValueError, match="Adafactor checkpoint"):
        tr._load_checkpoint(path)


def test_cli_override_reaches_the_arguments():
    from slamkit_amd.trainer import SLAMTrainingArguments
    from slamkit_amd.utils.config import load_config, to_container
    cfg = load_config("train", ["training_args.optim=adafactor"])
    known = SLAMTrainingArguments.__dataclass_fields__
    args = SLAMTrainingArguments(**{k: v for k, v in to_container(cfg.training_args).items() if k in known})
    assert args.optim == "adafactor"
    assert load_config("train", []).training_args.get("optim") is None   # the shipped recipes stay as they are
