"""SLAMTrainer and its optimizer object without a GPU, on a recorder over the stub model of test_trainer_dp_gloo.py: the exact
engine calls at construction and in one step for every optimizer kind and state precision (and for the sharded step behind a
forced one-rank ShardedGradReducer), the layout of optimizer.pt and its round trip, and the trainer's forwarding attributes.
Every expected list and layout below was taken from a run of the commit before the optimizer classes existed, where the trainer
made these calls itself: they pin the behaviour, not the code that now produces it."""
import os
import weakref

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import test_trainer_dp_gloo as base
from tests import test_trainer_rs_ag_gloo as rs

N = 2 * base.V * base.H   # 1184 elements in the stub's flat buffer
F32, BF16 = torch.float32, torch.bfloat16
RECORDED = ("adamw_range", "refresh_transposed", "grad_norm", "adamw_step", "adamw_step_bf16", "grad_sumsq_chunks",
            "grad_norm_from_chunks", "zero_grads")


class _Recorder:
    """tests/test_muon_host.py::_Recorder with more names: a step call is recorded with whether it got an fp32 master, a range
    call with its range and state offset."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []
        self.n_params = inner.n_params

    def __getattr__(self, k):
        if k.startswith("muon") or k.startswith("adafactor") or k in RECORDED:
            def rec(*a, **kw):
                if k == "adamw_range":
                    self.calls.append((k, a[0], a[1], kw.get("state_offset"), "master" if a[2] is not None else None))
                elif k in ("adafactor_step", "muon_step"):
                    self.calls.append((k, "master" if a[0] is not None else None))
                elif k == "grad_sumsq_chunks":
                    self.calls.append((k, a[0], a[1]))
                else:
                    self.calls.append(k)
                return (32, 512) if k == "muon_set_segments" else (16, 64) if k == "adafactor_set_segments" else None
            return rec
        return getattr(self.inner, k)


class _Seg:
    def __init__(self, entry):
        self.muon_entry = entry


def _stub_trainer(model=None, **kw):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    model = model or base.StubLM()
    model.engine = _Recorder(model.engine)
    model.hf_muon_segments = lambda: [_Seg((64, 8, 8, 0)), _Seg((256, 8, 8, 0))]
    model.hf_param_segments = lambda: []
    model._weights, model.sync_params_from_master = model.flat_master, lambda: None   # what a checkpoint touches
    return SLAMTrainer(model=model, args=SLAMTrainingArguments(logging_steps=0, **kw)), model


MUON_RUNS = [(0, 64, 0), (128, 128, 64), (320, N - 320, 192)]
# (optim, optim_state_dtype): (calls at construction, calls of one _clip_and_update)
CALLS = {
    ("adamw_torch", "float32"): ([], ["grad_norm", "adamw_step"]),
    ("adamw_torch", "bfloat16"): ([], ["grad_norm", "adamw_step_bf16"]),
    ("adamw_torch", "float32_bf16_moments"): ([], ["grad_norm", "adamw_step"]),
    ("adafactor", "float32"): (["adafactor_set_segments", "adafactor_bind_workspace"], ["grad_norm", ("adafactor_step", "master")]),
    ("adafactor", "bfloat16"): (["adafactor_set_segments", "adafactor_bind_workspace"], ["grad_norm", ("adafactor_step", None)]),
    ("muon", "float32"): (["muon_set_segments", "muon_bind_workspace"],
                          ["grad_norm", ("muon_step", "master")] + [("adamw_range", o, c, s, "master") for o, c, s in MUON_RUNS]
                          + ["refresh_transposed"]),
    ("muon", "bfloat16"): (["muon_set_segments", "muon_bind_workspace"],
                           ["grad_norm", ("muon_step", None)] + [("adamw_range", o, c, s, None) for o, c, s in MUON_RUNS]
                           + ["refresh_transposed"]),
}
# optimizer.pt per (optim, optim_state_dtype): [(key, dtype, numel)] in the file's order; "optim" and "opt_step" are no tensors
FILES = {
    ("adamw_torch", "float32"): [("master", F32, N), ("exp_avg", F32, N), ("exp_avg_sq", F32, N), ("opt_step", int, None)],
    ("adamw_torch", "bfloat16"): [("master", F32, N), ("exp_avg", BF16, N), ("exp_avg_sq", BF16, N), ("opt_step", int, None)],
    ("adamw_torch", "float32_bf16_moments"): [("master", F32, N), ("exp_avg", BF16, N), ("exp_avg_sq", BF16, N), ("opt_step", int, None)],
    ("adafactor", "float32"): [("master", F32, N), ("optim", str, None), ("adafactor_state", F32, 16), ("opt_step", int, None)],
    ("adafactor", "bfloat16"): [("master", F32, N), ("optim", str, None), ("adafactor_state", F32, 16), ("opt_step", int, None)],
    ("muon", "float32"): [("master", F32, N), ("optim", str, None), ("muon_momentum", F32, 32), ("exp_avg", F32, N - 128),
                          ("exp_avg_sq", F32, N - 128), ("opt_step", int, None)],
    ("muon", "bfloat16"): [("master", F32, N), ("optim", str, None), ("muon_momentum", F32, 32), ("exp_avg", BF16, N - 128),
                           ("exp_avg_sq", BF16, N - 128), ("opt_step", int, None)],
}
STATE_NAMES = ("exp_avg", "exp_avg_sq", "adafactor_state", "muon_momentum")


@pytest.mark.parametrize("optim,osd", list(CALLS), ids=lambda v: str(v))
def test_engine_calls_at_construction_and_in_one_step(optim, osd):
    built, stepped = CALLS[(optim, osd)]
    tr, model = _stub_trainer(optim=optim, optim_state_dtype=osd)
    print(optim, osd, "construction:", model.engine.calls)
    assert model.engine.calls == built
    del model.engine.calls[:]
    tr._clip_and_update(1e-3, zero_grad=True)
    print(optim, osd, "step:", model.engine.calls)
    assert model.engine.calls == stepped and tr.opt_step == 1
    del model.engine.calls[:]
    tr._update(1e-3, zero_grad=False)   # one rank, no forced exchange: the replicated step again
    assert model.engine.calls == stepped and tr.opt_step == 2


def test_adamw_torch_fused_is_the_same_optimizer():
    tr, model = _stub_trainer(optim="adamw_torch_fused")
    tr._clip_and_update(1e-3, zero_grad=True)
    assert model.engine.calls == CALLS[("adamw_torch", "float32")][1]


# ---- the sharded step -------------------------------------------------------------------------------------------------------------
SHARDED_STEP = [("grad_sumsq_chunks", 592, 592), ("grad_sumsq_chunks", 0, 592), "grad_norm_from_chunks",
                ("adamw_range", 592, 592, None, "master"), ("adamw_range", 0, 592, None, "master"), "zero_grads"]
SHARDED_STEP_TAIL = [("grad_sumsq_chunks", 640, 512), ("grad_sumsq_chunks", 0, 640), ("grad_sumsq_chunks", 1152, 32),
                     "grad_norm_from_chunks", ("adamw_range", 640, 512, None, None), ("adamw_range", 0, 640, None, None),
                     ("adamw_range", 1152, 32, None, None)]


def _sharded_worker(port, q):
    """One rank, SLAM_DP_FORCE=1: every collective of the rs_ag step runs on a group of one. The backward's two bucket callbacks
    leave this rank the two halves of the buffer (accumulating backward: the step ends with the zeroing pass); then the same
    step with a replicated tail, bf16 state and a storing first backward."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", SLAM_DP_FORCE="1")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        from slamkit_amd.data import DataCollatorForLanguageModeling
        tr, model = _stub_trainer(rs.ShardStubLM(), ddp_algo="rs_ag", ddp_bucket_layers=1, ddp_comm_dtype="float32",
                                  overwrite_first_grad=False)
        built = list(model.engine.calls)
        del model.engine.calls[:]
        mb = DataCollatorForLanguageModeling(pad_token_id=0)(base.make_rows(4))
        tr.optimizer_step([mb], 1e-3)
        first = (list(model.engine.calls), list(tr.reducer.owned), tr.opt_step, tr._shards_stale)
        rs.CHUNK = 64   # 1184 = 18 x 64 + 32: a replicated tail above the last whole chunk
        tr2, model2 = _stub_trainer(rs.ShardStubLM(), ddp_algo="rs_ag", ddp_bucket_layers=1, optim_state_dtype="bfloat16")
        tr2.optimizer_step([mb], 1e-3)
        q.put((built, first, (list(model2.engine.calls), list(tr2.reducer.owned), tr2.reducer.tail)))
    finally:
        dist.destroy_process_group()


def test_engine_calls_of_the_sharded_step_one_forced_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_sharded_worker, args=(base._free_port(), q))
    p.start()
    built, (calls, owned, opt_step, stale), (tail_calls, tail_owned, tail) = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    print("sharded:", built, calls, owned, tail_calls, tail_owned, tail)
    assert built == [] and owned == [(592, 592), (0, 592)] and opt_step == 1 and stale
    assert calls == SHARDED_STEP
    assert tail_owned == [(640, 512), (0, 640)] and tail == (1152, 32)
    assert tail_calls == SHARDED_STEP_TAIL


# ---- optimizer.pt -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optim,osd", list(FILES), ids=lambda v: str(v))
def test_optimizer_file_layout_and_round_trip(optim, osd, tmp_path):
    tr, model = _stub_trainer(optim=optim, optim_state_dtype=osd, output_dir=str(tmp_path))
    g = torch.Generator().manual_seed(1)
    kept = {}
    for name in STATE_NAMES:
        t = getattr(tr, name, None)
        if t is not None:
            t.copy_(torch.randn(t.numel(), generator=g))
            kept[name] = t.clone()
    tr.opt_step = 5
    tr.save_checkpoint()
    path = tr._ckpt_dir(0)
    st = torch.load(os.path.join(path, "optimizer.pt"))
    layout = [(k, v.dtype, v.numel()) if isinstance(v, torch.Tensor) else (k, type(v), None) for k, v in st.items()]
    print(optim, osd, layout)
    assert layout == FILES[(optim, osd)]
    assert st["opt_step"] == 5 and st.get("optim") == (None if optim == "adamw_torch" else optim)
    assert all(torch.equal(st[k], v) for k, v in kept.items()) and torch.equal(st["master"], model.flat_master)
    # into a fresh trainer of another seed: the master, every state tensor and the step count come back
    tr2, model2 = _stub_trainer(base.StubLM(seed=1), optim=optim, optim_state_dtype=osd, output_dir=str(tmp_path))
    assert not torch.equal(model2.flat_master, model.flat_master)
    tr2._load_checkpoint(path)
    assert tr2.opt_step == 5 and torch.equal(model2.flat_master, model.flat_master)
    assert all(torch.equal(getattr(tr2, k), v) for k, v in kept.items())
    assert [k for k in STATE_NAMES if getattr(tr2, k, None) is not None] == [k for k in STATE_NAMES if k in kept]


def test_a_checkpoint_of_another_size_is_refused_before_anything_is_overwritten(tmp_path):
    for optim, key in (("muon", "muon_momentum"), ("adamw_torch", "exp_avg"), ("adafactor", "adafactor_state")):
        tr, model = _stub_trainer(optim=optim, output_dir=str(tmp_path / optim))
        tr.save_checkpoint()
        path = tr._ckpt_dir(0)
        st = torch.load(os.path.join(path, "optimizer.pt"))
        st[key] = st[key][:-8]
        torch.save(st, os.path.join(path, "optimizer.pt"))
        tr2, model2 = _stub_trainer(base.StubLM(seed=1), optim=optim, output_dir=str(tmp_path / optim))
        before = model2.flat_master.clone()
        with pytest.raises(ValueError, match=f"another model or segment table: {key}"):
            tr2._load_checkpoint(path)
        assert torch.equal(model2.flat_master, before)


# ---- the trainer's attributes -----------------------------------------------------------------------------------------------------
def test_state_attributes_forward_to_the_optimizer():
    tr, _ = _stub_trainer(optim="adamw_torch")
    assert tr.exp_avg is tr.optimizer.state["exp_avg"] and tr.exp_avg_sq is tr.optimizer.state["exp_avg_sq"]
    assert tr.exp_avg.numel() == N and tr.optimizer.kind == "adamw" and tr.optimizer.state_bytes == (2 * 4 * N, 0)
    assert not hasattr(tr, "adafactor_state") and not hasattr(tr, "muon_momentum")
    with pytest.raises(AttributeError):
        del tr.muon_momentum
    refs = [weakref.ref(tr.exp_avg), weakref.ref(tr.exp_avg_sq)]
    tr.exp_avg = tr.exp_avg_sq = None                       # "one optimizer state at a time": the memory must really go
    assert tr.exp_avg is None and tr.optimizer.state["exp_avg"] is None and all(r() is None for r in refs)
    tr, _ = _stub_trainer(optim="adamw_torch", optim_state_dtype="bfloat16")
    refs = [weakref.ref(tr.exp_avg), weakref.ref(tr.exp_avg_sq)]
    del tr.exp_avg, tr.exp_avg_sq
    assert all(r() is None for r in refs) and not hasattr(tr, "exp_avg") and "exp_avg_sq" not in tr.optimizer.state
    new = torch.ones(3)
    tr.exp_avg = new
    assert tr.optimizer.state["exp_avg"] is new
    tr, _ = _stub_trainer(optim="adafactor")
    assert tr.exp_avg is None and tr.exp_avg_sq is None and not hasattr(tr, "muon_momentum")
    assert tr.adafactor_state is tr.optimizer.state["adafactor_state"] and tr.optimizer.state_bytes == (4 * 16, 64)
    tr, _ = _stub_trainer(optim="muon")
    assert tr.muon_momentum is tr.optimizer.state["muon_momentum"] and not hasattr(tr, "adafactor_state")
    assert list(tr.optimizer.state) == ["muon_momentum", "exp_avg", "exp_avg_sq"] and tr.optimizer.adamw_runs == MUON_RUNS


def test_each_refusal_is_written_once():
    """Every kind's refusals come from one function: the shared sentences stand once in the trainer package."""
    import slamkit_amd.trainer as T
    root = os.path.dirname(T.__file__)
    text = "".join(open(os.path.join(root, f)).read() for f in sorted(os.listdir(root)) if f.endswith(".py"))
    for sentence in ("a shard of the flat buffer cuts them", "has no overlapped form", "needs a model that knows its {"):
        assert text.count(sentence) == 1, sentence
    for gone in ("needs a model that knows its decoder", "needs a model that knows its HF parameter tensors"):
        assert gone not in text
