"""CPU tier of label smoothing (SLAMTrainingArguments.label_smoothing_factor, UnitLM.forward(label_smoothing=),
slam_set_label_smoothing): the formula's numpy restatement against HF's own LabelSmoother (golden), the argument / YAML / trainer
plumbing on a stub model, and the ABI surface - declared, exported, bound, refusing bad arguments before anything touches a
device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import label_smoothing_ref as R

NEW_SYMBOLS = ("slam_set_label_smoothing", "slam_op_cross_entropy_smooth")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_smoothing_hf.npz")
U32 = 2.0 ** -24  # unit round-off of float32


def _cases():
    g = np.load(GOLDEN)
    for i in range(int(g["n_cases"])):
        yield (i, g[f"logits_{i}"], g[f"labels_{i}"], float(g[f"eps_{i}"]), int(g[f"num_items_{i}"]) or None,
               float(g[f"loss_{i}"]), g[f"grad_{i}"])


def test_ref_matches_hf_label_smoother_golden():
    """tests/golden/label_smoothing_hf.npz holds HF's LabelSmoother (shift_labels=True) + autograd on float64 copies of fp32
    logits. HF's plain term is float64 there; its smoothing term is not: HF sums the -log p_v of a position with dtype=float32
    and carries that term in float32 until it is added to the plain one. So:
      eps = 0 (plain term alone): loss within 1e-13 relative, gradient within 1e-15 absolute + 1e-13 relative - float64 round-off;
      eps > 0: the smoothing term eps * S / denom (S = sum_t smooth_t, all terms positive) is known to HF only up to the float32
      roundings of: V values and their V - 1 additions per position, N - 1 additions over the N positions, one division, the
      conversion of eps and one product - at most (V + N + 4) * 2^-24 relative to that term; its gradient carries the 4 roundings
      of eps / (denom * V): at most 4 * 2^-24 * eps / denom per element. Those are the bounds, plus the float64 ones above."""
    n_eps0 = 0
    for i, logits, labels, eps, n, loss, grad in _cases():
        assert logits.dtype == np.float32 and (labels == -100).any() and (labels[:, 1:] == 0).any()
        V = logits.shape[-1]
        assert (labels[:, 1:] == V - 1).any()
        r = R.label_smoothing(logits, labels, eps, n)
        N = int(r["valid"].sum())
        smooth_term = eps * r["smooth"].sum() / r["denom"]
        tol_loss = 1e-13 * abs(loss) + smooth_term * (V + N + 4) * U32
        tol_grad = 1e-15 + 1e-13 * np.abs(grad).max() + 4 * U32 * eps / r["denom"]
        dl, dg = abs(float(r["loss"]) - loss), float(np.abs(r["grad"] - grad).max())
        print(f"case {i}: eps {eps} num_items {n}: loss {loss:.12f} |d| {dl:.2e} (bound {tol_loss:.2e}), grad |d| {dg:.2e} (bound {tol_grad:.2e})")
        assert dl <= tol_loss and dg <= tol_grad, i
        assert r["denom"] == (n if n else N)
        n_eps0 += eps == 0.0
    assert n_eps0 >= 2


def test_ref_properties():
    """eps = 0 is the oracle's compute_loss; the gradient is the derivative of the loss (central differences); rows without
    a target are zero; the torch restatement agrees with the numpy one."""
    from oracle.slam_oracle import compute_loss
    _, logits, labels, _, _, _, _ = next(_cases())
    for n in (None, 17):
        x = torch.from_numpy(logits).double().requires_grad_(True)
        ref = compute_loss(x, torch.from_numpy(labels), num_items_in_batch=n)  # .float() inside: an fp32 reference
        ref.backward()
        r0 = R.label_smoothing(logits, labels, 0.0, n)
        assert abs(float(r0["loss"]) - float(ref.detach())) <= 1e-6 * float(ref.detach())
        assert np.abs(r0["grad"][:, :-1] - x.grad.numpy()[:, :-1]).max() <= 1e-6
        r = R.label_smoothing(logits, labels, 0.3, n)
        assert (r["grad"][~r["valid"]] == 0).all() and (r["nll"][~r["valid"]] == 0).all() and (r["smooth"][~r["valid"]] == 0).all()
        assert not r["valid"][:, -1].any()
        assert np.array_equal(r["nll"], r0["nll"])  # the plain per-row term does not depend on eps
        assert abs(r["grad"][r["valid"]].sum(-1)).max() <= 1e-15  # p - (1 - eps) onehot - eps / V sums to 0
        z = logits.astype(np.float64)
        for (b, t, v) in ((0, 0, 0), (1, 3, 36), (0, 4, 11)):
            zp, zm = z.copy(), z.copy()
            zp[b, t, v] += 1e-5
            zm[b, t, v] -= 1e-5
            fd = (R.label_smoothing(zp, labels, 0.3, n)["loss"] - R.label_smoothing(zm, labels, 0.3, n)["loss"]) / 2e-5
            assert abs(fd - r["grad"][b, t, v]) <= 1e-8
        xt = torch.from_numpy(z).requires_grad_(True)
        lt = R.label_smoothing_torch(xt, torch.from_numpy(labels), 0.3, n)
        lt.backward()
        assert abs(float(lt.detach()) - float(r["loss"])) <= 1e-13 * float(r["loss"])
        assert np.abs(xt.grad.numpy() - r["grad"]).max() <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- ABI surface
def test_symbols_declared_exported_and_bound():
    lib = E.load_library()
    names = E.header_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(lib, n) and n in lib._slam_signatures, n
    assert sorted(lib._slam_signatures) == names
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slam_engine.h")).read()
    doc = hdr[hdr.index("Label smoothing of the training loss"):hdr.index("int slam_set_label_smoothing")]
    for word in ("smooth_t = lse - (1 / V) sum_v z_v", "(1 - epsilon) sum_t nll_t + epsilon sum_t smooth_t", "xor butterfly",
                 "wave order", "PLAIN nll_t", "SLAM_ESTATE"):
        assert word in doc, word


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Nothing here reaches a device: every refusal happens before a launch."""
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(2, 256, 4, 2, 64, 512, 502, 0, 1e-6, 10000.0))
    f = lib.slam_set_label_smoothing
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert f(eng.h, bad) == -1, bad
        assert b"[0, 1)" in lib.slam_last_error(eng.h)
    for ok in (0.0, 0.1, 0.999, 0.0):
        assert f(eng.h, ok) == 0, ok
    assert f(None, 0.1) == -1
    with pytest.raises(E.EngineError, match="label smoothing"):
        eng.set_label_smoothing(1.0)
    eng.set_label_smoothing(0.25)
    eng.set_label_smoothing(0)
    one = C.c_void_p(256)  # a non-null address that is never dereferenced
    op = lib.slam_op_cross_entropy_smooth
    assert op(one, one, 0.0, one, one, one, one, 3, 41, 512, 502, 1.0, None) == -1
    assert op(one, one, 0.0, one, one, one, one, 3, 41, 512, 502, -0.5, None) == -1
    assert op(one, one, 0.0, one, one, None, one, 3, 41, 512, 502, 0.1, None) == -1   # smoothing without its row array
    assert op(None, one, 0.0, one, one, one, one, 3, 41, 512, 502, 0.1, None) == -1
    assert op(one, one, 0.0, one, one, one, one, 3, 41, 500, 502, 0.1, None) == -1    # V > Vp
    assert op(one, one, 0.0, one, one, one, one, 3, 41, 516, 502, 0.1, None) == -1    # Vp not a multiple of 8
    eng.close()


# ------------------------------------------------------------------------------------------------------ arguments and trainers
def test_argument_validation_and_yaml():
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer, SLAMTrainingArguments
    from slamkit_amd.utils.config import CONFIG_DIR, load_config, to_container
    assert SLAMTrainingArguments().label_smoothing_factor == 0.0 and DPOConfig().label_smoothing_factor == 0.0
    assert SLAMTrainingArguments(label_smoothing_factor=0.1).label_smoothing_factor == 0.1
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError, match="label_smoothing_factor"):
            SLAMTrainingArguments(label_smoothing_factor=bad)
    # DPO: TRL's label_smoothing is another quantity - a non-zero factor is refused, before anything is built
    with pytest.raises(ValueError, match="label_smoothing_factor"):
        SLAMDPOTrainer(model=None, args=DPOConfig(label_smoothing_factor=0.1))
    # the recipes carry the default, and the train CLI's override reaches the dataclass
    assert "label_smoothing_factor: 0.0" in open(os.path.join(CONFIG_DIR, "training_args", "_recipe_common.yaml")).read()
    for top in ("train", "train_inter_scale", "preference_alignment_train"):
        assert to_container(load_config(top).training_args)["label_smoothing_factor"] == 0.0, top
    ta = to_container(load_config("train", ["training_args.label_smoothing_factor=0.1"]).training_args)
    known = SLAMTrainingArguments.__dataclass_fields__
    assert SLAMTrainingArguments(**{k: v for k, v in ta.items() if k in known}).label_smoothing_factor == 0.1


def _recorder():
    from tests.test_trainer_dp_gloo import StubLM

    class Rec(StubLM):
        def __init__(self):
            super().__init__()
            self.seen = []

        def forward(self, **kw):
            self.seen.append(kw.get("label_smoothing", "absent"))
            kw.pop("label_smoothing", None)
            return super().forward(**kw)

    return Rec()


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_trainer_hands_the_factor_to_forward_in_training_and_evaluation(tmp_path, eps):
    from slamkit_amd.data import DataCollatorForLanguageModeling
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import make_rows
    m = _recorder()
    args = SLAMTrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=2, learning_rate=1e-2, warmup_steps=1,
                                 warmup_ratio=0.0, max_steps=2, gradient_accumulation_steps=2, logging_steps=0, save_steps=0,
                                 label_smoothing_factor=eps, per_device_eval_batch_size=2)
    tr = SLAMTrainer(model=m, args=args, data_collator=DataCollatorForLanguageModeling(pad_token_id=0),
                     train_dataset=make_rows(), eval_dataset=make_rows(6, seed=9))
    want = eps if eps else "absent"  # 0 passes nothing: the calls are what they were
    tr.train()
    assert m.seen == [want] * 4   # 2 steps x 2 micro-batches
    m.seen.clear()
    tr.evaluate()
    assert m.seen == [want] * 3
    # a field set after construction gets past the dataclass check; the trainer checks again
    args.label_smoothing_factor = 1.0
    with pytest.raises(ValueError, match="label_smoothing_factor"):
        SLAMTrainer(model=_recorder(), args=args, data_collator=DataCollatorForLanguageModeling(pad_token_id=0),
                    train_dataset=make_rows())


def test_model_sets_the_engine_value_only_when_it_changes():
    from slamkit_amd.model import UnitLM

    class Eng:
        def __init__(self):
            self.calls = []

        def set_label_smoothing(self, e):
            self.calls.append(e)

    m = object.__new__(UnitLM)
    m.engine, m._smoothing = Eng(), 0.0
    for e in (0.0, 0.1, 0.1, 0.0, 0.0, None, 0.5):
        m._set_label_smoothing(e)
    assert m.engine.calls == [0.1, 0.0, 0.5]
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            m._set_label_smoothing(bad)
    assert m.engine.calls == [0.1, 0.0, 0.5] and m._smoothing == 0.5
