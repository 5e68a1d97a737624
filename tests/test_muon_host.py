"""optim = "muon" without a GPU: the arguments and their refusals, the C ABI (declared, exported, bound; table validation before
anything reaches the device), the pinned Muon segment lists, the trainer's call order on a recorder stub, tests/muon_ref.py
against torch.optim.Muon itself, and the tolerance of the orthogonalised update: measured per input (muon_ref.bar) and shown to
tell the rule from three near misses."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import adafactor_ref as A
from tests import muon_ref as R
from tests.test_adafactor_host import host_model

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slam_engine.h")
MUON_SYMBOLS = ("slam_muon_set_segments", "slam_muon_sizes", "slam_muon_bind_workspace", "slam_muon_class_count",
                "slam_muon_class_info", "slam_muon_step", "slam_op_muon_prepare", "slam_op_muon_ns_workspace", "slam_op_muon_ns",
                "slam_op_muon_apply", "slam_op_muon_syrk", "slam_op_muon_mm")
NS_SHAPES = [(128, 896), (320, 192), (384, 384), (72, 200)]   # the GPU tier's slam_op_muon_ns shapes


def gaussian(shape, seed=0):
    return R.bf16(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------ arguments
def test_muon_arguments_and_their_refusals():
    from slamkit_amd.trainer import DPOConfig, SLAMTrainingArguments
    a = SLAMTrainingArguments(optim="muon")
    assert (a.optim, a.muon_momentum, a.muon_nesterov, a.muon_ns_steps, a.muon_adjust_lr) == ("muon", 0.95, True, 5, "match_rms_adamw")
    assert SLAMTrainingArguments().optim == "adamw_torch" and DPOConfig(optim="muon").optim == "muon"
    for adj in ("match_rms_adamw", "original", None):
        assert SLAMTrainingArguments(optim="muon", muon_adjust_lr=adj).muon_adjust_lr == adj
    with pytest.raises(ValueError, match="adamw_torch.*adamw_torch_fused.*adafactor.*muon"):
        SLAMTrainingArguments(optim="lion")
    for kw, word in ((dict(muon_ns_steps=0), "muon_ns_steps"), (dict(muon_ns_steps=17), "muon_ns_steps"),
                     (dict(muon_momentum=1.0), "muon_momentum"), (dict(muon_momentum=-0.1), "muon_momentum"),
                     (dict(muon_adjust_lr="rms"), "muon_adjust_lr")):
        with pytest.raises(ValueError, match=word):
            SLAMTrainingArguments(optim="muon", **kw)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(HDR).read()
    lib = E.load_library()
    for name in MUON_SYMBOLS:
        assert name in E.header_symbols() and name in lib._slam_signatures and hasattr(lib, name), name
    assert re.search(r"int slam_muon_step\(SlamEngine\* h, float\* master_f32, float\* momentum_f32, const float\* norm_out, double lr, "
                     r"double weight_decay,\s+double momentum, int32_t nesterov, int32_t ns_steps, double a, double b, double c, "
                     r"double eps, int32_t adjust_lr,\s+int32_t step, int32_t zero_grad, slam_stream_t stream\);", hdr)
    assert C.sizeof(E.SlamMuonSegment) == 24 and C.sizeof(E.SlamMuonClass) == 40
    assert list(lib.slam_muon_step.argtypes) == ([C.c_void_p] * 4 + [C.c_double] * 3 + [C.c_int32] * 2 + [C.c_double] * 4 +
                                                 [C.c_int32] * 3 + [C.c_void_p])
    assert E.MUON_ADJUST_LR == {None: 0, "original": 1, "match_rms_adamw": 2}


def test_table_validation_and_refusals_before_the_device():
    """Every bad table is SLAM_EINVAL with a message naming the segment, decided on the host; so are the step's refusals."""
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(2, 64, 4, 2, 64, 128, 502, 0, 1e-6, 10000.0))
    n = eng.n_params

    def refused(rows, word, code=-1):
        buf = (E.SlamMuonSegment * len(rows))(*[E.SlamMuonSegment(*r, 0) for r in rows])
        assert lib.slam_muon_set_segments(eng.h, buf, len(rows)) == code
        assert word in lib.slam_last_error(eng.h).decode(), lib.slam_last_error(eng.h)

    refused([(0, 0, 64, 0)], "positive")
    refused([(0, 1, 64, 0)], "not a matrix")
    refused([(0, 64, 1, 0)], "not a matrix")
    refused([(0, 64, 64, 3)], "pattern")
    refused([(0, 48, 64, 1)], "groups of 32")
    refused([(4, 64, 64, 0)], "misaligned")
    refused([(0, 64, 60, 0)], "misaligned")
    refused([(0, 12, 64, 0)], "misaligned")
    refused([(n - 64, 64, 64, 0)], "out of range")
    refused([(0, 64, 64, 0), (64 * 32, 64, 64, 0)], "overlap")
    refused([(0, 64, 64, 1), (64 * 64, 32, 64, 0)], "overlap")      # the second 32-row group of the first starts at row 64
    seg = (E.SlamMuonSegment * 1)(E.SlamMuonSegment(0, 64, 64, 0, 0))
    assert lib.slam_muon_set_segments(eng.h, seg, 0) == -1 and lib.slam_muon_set_segments(eng.h, None, 2) == -1
    assert lib.slam_muon_set_segments(eng.h, None, 0) == 0                                     # clearing an empty table
    assert lib.slam_muon_set_segments(None, seg, 1) == -1
    # sizes / workspace / step without a table: SLAM_ESTATE, with the reason
    with pytest.raises(E.EngineError, match="segment table"):
        eng.muon_sizes()
    one = C.c_void_p(256)    # never dereferenced: every call below is refused on the host
    assert lib.slam_muon_bind_workspace(eng.h, one, 1 << 20) == -2 and lib.slam_muon_bind_workspace(eng.h, None, 0) == 0
    step = lambda mom, ns, adj=2, st=1, mu=0.95: lib.slam_muon_step(eng.h, None, mom, None, 1e-3, 0.0, mu, 1, ns, R.A, R.B, R.C, R.EPS,
                                                                     adj, st, 0, None)
    for call, word in ((lambda: step(one, 0), "ns_steps"), (lambda: step(one, 17), "ns_steps"), (lambda: step(None, 5), "momentum_f32 is NULL"),
                       (lambda: step(one, 5, adj=3), "adjust_lr"), (lambda: step(one, 5, st=0), "step counts"),
                       (lambda: step(one, 5, mu=1.0), "momentum must")):
        assert call() == -1 and word in lib.slam_last_error(eng.h).decode(), (word, lib.slam_last_error(eng.h))
    assert step(one, 5) == -2 and "segment table" in lib.slam_last_error(eng.h).decode()
    eng.set_option("overlap_adamw", 1)
    assert step(one, 5) == -2 and "overlap_adamw" in lib.slam_last_error(eng.h).decode()
    eng.set_option("overlap_adamw", 0)
    assert lib.slam_muon_step(None, None, one, None, 1e-3, 0.0, 0.95, 1, 5, R.A, R.B, R.C, R.EPS, 2, 1, 0, None) == -1
    assert lib.slam_op_muon_prepare(eng.h, one, None, 0.95, 1, 0, None) == -2
    assert lib.slam_op_muon_apply(eng.h, None, None, 1e-3, 0.0, 2, 1, None) == -2
    assert lib.slam_muon_class_count(eng.h) == 0
    # the batch doors refuse shapes that are no multiples of 8, n > m and a short workspace before any launch
    assert E.muon_ns_workspace_bytes(3, 72, 200) > 3 * 72 * 200 * 2 and E.muon_ns_workspace_bytes(1, 70, 200) == 0
    assert lib.slam_op_muon_ns(one, 1, 200, 72, 200 * 72, None, 0, 5, R.A, R.B, R.C, R.EPS, one, 1 << 30, None) == -1
    assert lib.slam_op_muon_ns(one, 1, 72, 200, 72 * 200, None, 0, 5, R.A, R.B, R.C, R.EPS, one, 16, None) == -3
    assert lib.slam_op_muon_syrk(one, None, one, 1, 70, 200, 70 * 200, 0, 70 * 70, 1.0, 0.0, None) == -1
    assert lib.slam_op_muon_mm(one, one, None, one, 1, 72, 200, 72 * 72, 72 * 200 + 4, 0, 72 * 200, 1.0, 0.0, None) == -1
    eng.close()


# ------------------------------------------------------------------------------------------------ the segment lists
def _expected_muon(fam):
    """The Muon matrices of the one-layer test bodies, pinned: (HF name, rows, cols, pattern) in key-map order."""
    if fam == "opt":
        p = "lm.model.decoder.layers.0."
        return [(p + "self_attn.q_proj.weight", 64, 64, 0), (p + "self_attn.k_proj.weight", 64, 64, 0),
                (p + "self_attn.v_proj.weight", 64, 64, 0), (p + "self_attn.out_proj.weight", 64, 64, 0),
                (p + "fc1.weight", 64, 64, 0), (p + "fc2.weight", 64, 64, 0)]
    p = "lm.model.layers.0."
    return [(p + "self_attn.q_proj.weight", 64, 64, 0), (p + "self_attn.k_proj.weight", 64, 64, 0),
            (p + "self_attn.v_proj.weight", 64, 64, 0), (p + "self_attn.o_proj.weight", 64, 64, 0),
            (p + "mlp.gate_proj.weight", 64, 64, 1), (p + "mlp.up_proj.weight", 64, 64, 2), (p + "mlp.down_proj.weight", 64, 64, 0)]


@pytest.mark.parametrize("fam", list(A.FAMILIES))
def test_muon_segments_are_pinned(fam):
    m = host_model(fam)
    segs = m.hf_muon_segments()
    assert sorted((s.name, s.rows, s.cols, s.pattern) for s in segs) == sorted(_expected_muon(fam))
    every = {s.name: s for s in m.hf_param_segments()}
    assert all(every[s.name] == s for s in segs)                        # a subset of hf_param_segments, entries unchanged
    rest = [n for n in every if n not in {s.name for s in segs}]
    assert all(("embed" in n or "lm_head" in n or "norm" in n or n.endswith(".bias")) for n in rest), rest
    assert any("embed_tokens" in n for n in rest) and (fam != "qwen2_untied" or "lm.lm_head.weight" in rest)
    if fam == "qwen3":
        assert sum("q_norm" in n or "k_norm" in n for n in rest) == 2
    if fam == "opt":
        assert any("embed_positions" in n for n in rest)
    # the AdamW runs: the exact complement, in order, with compact state offsets
    from slamkit_amd.trainer.slam_trainer import muon_adamw_runs
    n = m.engine.n_params
    cov = np.zeros(n, dtype=bool)
    for s in segs:
        cov[R.seg_rows(s.muon_entry).reshape(-1)] = True
    runs = muon_adamw_runs([s.muon_entry for s in segs], n)
    got = np.zeros(n, dtype=bool)
    so = 0
    for off, cnt, state in runs:
        assert cnt > 0 and off % 8 == 0 and cnt % 8 == 0 and state == so and not got[off:off + cnt].any()
        got[off:off + cnt] = True
        so += cnt
    assert bool((got == ~cov).all()) and so == n - int(cov.sum())
    assert all(a[0] + a[1] < b[0] for a, b in zip(runs, runs[1:]))     # maximal runs: a Muon matrix between any two
    m.engine.close()


# ------------------------------------------------------------------------------------------------ the trainer on a recorder
class _Recorder:
    def __init__(self, inner):
        self.inner, self.calls = inner, []
        self.n_params = inner.n_params

    def __getattr__(self, k):
        if k.startswith("muon") or k.startswith("adafactor") or k in ("adamw_range", "refresh_transposed", "grad_norm", "adamw_step"):
            def rec(*a, **kw):
                self.calls.append(k if k != "adamw_range" else (k, a[0], a[1], kw.get("state_offset")))
                return (32, 512) if k == "muon_set_segments" else (16, 64) if k == "adafactor_set_segments" else None
            return rec
        return getattr(self.inner, k)


class _Seg:
    def __init__(self, entry):
        self.muon_entry = entry


def _stub_trainer(**kw):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import StubLM
    model = StubLM()
    model.engine = _Recorder(model.engine)
    model.hf_muon_segments = lambda: [_Seg((64, 8, 8, 0)), _Seg((256, 8, 8, 0))]
    model.hf_param_segments = lambda: []
    model._weights, model.sync_params_from_master = model.flat_master, lambda: None
    return SLAMTrainer(model=model, args=SLAMTrainingArguments(logging_steps=0, **kw)), model


def test_trainer_call_order_under_muon_and_no_new_call_elsewhere():
    for name in ("adamw_torch", "adamw_torch_fused", "adafactor"):
        tr, model = _stub_trainer(optim=name)
        assert not [c for c in model.engine.calls if str(c).startswith("muon")] and not hasattr(tr, "muon_momentum")
    tr, model = _stub_trainer(optim="muon")
    n = model.engine.n_params
    assert model.engine.calls == ["muon_set_segments", "muon_bind_workspace"]       # the table once, then the workspace
    assert tr.muon_momentum.numel() == 32 and tr.muon_momentum.dtype == torch.float32
    assert tr.exp_avg.numel() == tr.exp_avg_sq.numel() == n - 128                    # moments for AdamW's elements only
    assert tr.optimizer_state_bytes == (4 * 32 + 2 * 4 * (n - 128), 512)
    del model.engine.calls[:]
    tr._clip_and_update(1e-3, zero_grad=True)
    assert tr.opt_step == 1
    assert model.engine.calls == ["grad_norm", "muon_step", ("adamw_range", 0, 64, 0), ("adamw_range", 128, 128, 64),
                                  ("adamw_range", 320, n - 320, 192), "refresh_transposed"]
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import StubLM
    for kw, word in ((dict(optim_state_dtype="float32_bf16_moments"), "moments"), (dict(ddp_algo="rs_ag"), "rs_ag"),
                     (dict(overlap_optimizer=True), "overlap_optimizer")):
        with pytest.raises(ValueError, match=word):
            _stub_trainer(optim="muon", **kw)
    args = SLAMTrainingArguments(logging_steps=0, optim="muon")
    with pytest.raises(ValueError, match="hf_muon_segments"):
        SLAMTrainer(model=StubLM(), args=args)
    args.muon_ns_steps = 40   # a field set after construction gets past the arguments' own check: the trainer checks again
    with pytest.raises(ValueError, match="muon_ns_steps"):
        _stub_trainer_with(args)


def _stub_trainer_with(args):
    from slamkit_amd.trainer import SLAMTrainer
    from tests.test_trainer_dp_gloo import StubLM
    model = StubLM()
    model.engine = _Recorder(model.engine)
    model.hf_muon_segments = lambda: [_Seg((64, 8, 8, 0))]
    return SLAMTrainer(model=model, args=args)


def test_checkpoint_kinds(tmp_path):
    from slamkit_amd.trainer.slam_trainer import check_checkpoint_optim
    adam = {"master": 0, "exp_avg": 0, "exp_avg_sq": 0, "opt_step": 3}
    fact = {"master": 0, "optim": "adafactor", "adafactor_state": 0, "opt_step": 3}
    muon = {"master": 0, "optim": "muon", "muon_momentum": 0, "exp_avg": 0, "exp_avg_sq": 0, "opt_step": 3}
    check_checkpoint_optim(adam, False), check_checkpoint_optim(fact, True), check_checkpoint_optim(muon, "muon")   # the existing calls
    for st, kind, word in ((muon, False, "Muon checkpoint"), (muon, True, "Muon checkpoint"), (adam, "muon", "AdamW checkpoint"),
                           (fact, "muon", "Adafactor checkpoint"), (adam, True, "AdamW checkpoint"), (fact, False, "Adafactor checkpoint")):
        with pytest.raises(ValueError, match=word):
            check_checkpoint_optim(st, kind)
    # through the trainer: optimizer.pt carries the kind, the momentum buffer and the compact moments; the other kinds refuse it
    tr, model = _stub_trainer(optim="muon", output_dir=str(tmp_path))
    tr.save_checkpoint()
    path = tr._ckpt_dir(0)
    st = torch.load(os.path.join(path, "optimizer.pt"))
    assert set(st) == {"master", "optim", "muon_momentum", "exp_avg", "exp_avg_sq", "opt_step"} and st["optim"] == "muon"
    assert st["muon_momentum"].numel() == 32 and st["exp_avg"].numel() == model.engine.n_params - 128
    tr._load_checkpoint(path)
    tr2, model2 = _stub_trainer(optim="adamw_torch", output_dir=str(tmp_path))
    before = model2.flat_master.clone()
    with pytest.raises(ValueError, match="Muon checkpoint"):
        tr2._load_checkpoint(path)
    assert torch.equal(model2.flat_master, before)                      # before anything is overwritten
    tr2.save_checkpoint()
    with pytest.raises(ValueError, match="AdamW checkpoint"):
        tr._load_checkpoint(path)


# ------------------------------------------------------------------------------------------------ muon_ref against torch
@pytest.mark.skipif(not hasattr(torch.optim, "Muon"), reason="this torch has no torch.optim.Muon")
@pytest.mark.parametrize("shape", [(72, 200), (200, 72)], ids=["wide", "tall"])
@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "plain"])
@pytest.mark.parametrize("adjust", ["match_rms_adamw", "original"])
def test_restatement_against_torch_muon(shape, nesterov, adjust):
    """Three consecutive steps of torch.optim.Muon (CPU, fp32 parameter) and of the restatement from the same gradients. Per step
    the two orthogonalised updates differ by summation order only: the parameters stay within the accumulated lr_adj * bar * |O|
    (plus the fp32 roundings of the apply and of torch's lerp form of the momentum, 2^-22 |p| a step)."""
    rng = np.random.default_rng(11)
    lr, wd = 2.0 ** -6, 0.125
    p0 = R.bf16(rng.standard_normal(shape).astype(np.float32) * 0.05)
    gs = [rng.standard_normal(shape).astype(np.float32) for _ in range(3)]
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Muon([pt], lr=lr, weight_decay=wd, momentum=0.95, nesterov=nesterov, adjust_lr_fn=adjust)
    p, buf, budget = p0.copy(), np.zeros(shape, np.float32), 0.0
    for g in gs:
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        bnew, x = R.prepare_f32(g, buf, 1.0, 0.95, nesterov)
        b, s, o = R.bar(x)
        p, buf = R.apply_f32(p, o, lr, wd, adjust, *shape), bnew
        budget += lr * R.lr_ratio(adjust, *shape) * b * float(np.linalg.norm(o)) + 2.0 ** -22 * float(np.linalg.norm(p))
    tb = opt.state[pt]["momentum_buffer"].numpy()
    assert np.abs(tb - buf).max() <= 2.0 ** -22 * np.abs(buf).max()            # lerp's form of the same blend
    d = float(np.linalg.norm(pt.detach().numpy().astype(np.float64) - p))
    print(f"[muon] torch vs restatement {shape} {adjust} nesterov={nesterov}: |dp| {d:.3e} budget {budget:.3e}")
    assert d <= budget


# ------------------------------------------------------------------------------------------------ the bar
@pytest.mark.parametrize("shape", NS_SHAPES + [(64, 64), (256, 512), (512, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_bar_discriminates(shape):
    """max(4 s, 2^-8) at every shape the GPU tier compares an orthogonalised matrix at: the float32-permuted restatement passes
    it by construction; one iteration fewer, b and c swapped, and no normalisation each land ABOVE it (a diverged result counts)."""
    x = gaussian(shape, seed=shape[0] * 7 + shape[1])
    b, s, o = R.bar(x)
    print(f"[muon] {shape}: s = {s:.3e}, bar = {b:.3e}")
    assert 2.0 ** -8 <= b < 0.05 and s <= b / 4
    with np.errstate(all="ignore"):
        misses = {"ns_steps - 1": R.orthogonalize(x, 4), "b and c swapped": R.orthogonalize(x, 5, (R.A, R.C, R.B)),
                  "no normalisation": R.orthogonalize(x, 5, normalise=False)}
        for what, got in misses.items():
            d = R.rel_dist(got, o)
            assert not d <= b, (what, d, b)
    # the result is an approximate orthogonalisation: no singular value above the band torch documents (about 0.5 .. 1.5), most
    # inside it (a square Gaussian has singular values near 0 that five iterations do not lift)
    sv = np.linalg.svd(o.astype(np.float64), compute_uv=False)
    assert sv.max() < 1.6 and 0.5 < np.median(sv) < 1.3
