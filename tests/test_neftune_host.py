"""CPU tier of NEFTune (slam_set_neftune, engine option "neftune_call_next"; HF TrainingArguments.neftune_noise_alpha): the
restated scale against the magnitude transformers' own hook uses (tests/golden/neftune_hf.npz), bounds / moments / key structure
of the restated noise, the host-side refusals of the ABI, and how the arguments, the trainer and the CLI carry the field.
Engine creation and every refusal are host-only."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from slamkit_amd import engine as E
from tests import neftune_ref as R

E_INVAL, E_STATE, E_NOMEM = -1, -2, -3
OPT125M = (12, 768, 12, 12, 64, 3072, 502, 1, 1e-5, 10000.0)
SLAM358M = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neftune_hf.npz")
N = 1 << 20


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    assert len(g["alpha"]) >= 12 and int(g["n"]) == N
    return g


# ------------------------------------------------------------------------------------------------------------ the numbers
def test_scale_is_hfs_magnitude(gold):
    """65536 s against the `mag_norm` the hook handed to uniform_: HF takes the square root and the division in fp32 (2^-24
    each); s itself and the recorded fp32 value are rounded once each (2^-24 each): 2^-22 in all."""
    for alpha, T, H, mag in zip(gold["alpha"], gold["T"], gold["H"], gold["mag_norm"]):
        s = R.scale(alpha, int(T), int(H))
        assert s.dtype == np.float32 and s > 0
        rel = abs(65536.0 * float(s) - float(mag)) / float(mag)
        print(f"[neftune] alpha {alpha:g} T {T} H {H}: 65536 s = {65536.0 * float(s):.9g}, HF {float(mag):.9g}, rel {rel:.2e}")
        assert rel <= 2.0 ** -22, (alpha, T, H, rel)


def test_moments_and_bounds(gold):
    """2^20 elements per golden tuple: |n| < mag for every element; mean within 6 standard errors of 0; variance within 6
    standard errors of mag^2 / 3 and of HF's recorded sample variance. Uniform on (-mag, mag): var = mag^2 / 3, fourth moment
    mag^4 / 5, so SE(mean) = mag / sqrt(3 N) and SE(var) = mag^2 sqrt((1/5 - 1/9) / N)."""
    for i, (alpha, T, H) in enumerate(zip(gold["alpha"], gold["T"], gold["H"])):
        T, H = int(T), int(H)
        s = R.scale(alpha, T, H)
        mag = float(alpha) / math.sqrt(T * H)
        # the noise is a function of the flat index: the first 2^20 elements of any [M, H] launch are these
        n = R.noise(N // 8, 8, s, seed=0xA5A5_0000_1234_5678 + i, call=3 + i).astype(np.float64).reshape(-1)
        assert np.abs(n).max() < mag and np.abs(n).max() <= float(np.float32(65535.0) * s)  # the largest level, as fp32 rounds it
        se_mean, se_var = mag / math.sqrt(3.0 * N), mag * mag * math.sqrt((1.0 / 5.0 - 1.0 / 9.0) / N)
        mean, var = n.mean(), n.var()
        print(f"[neftune] alpha {alpha:g} T {T} H {H}: mean {mean / se_mean:+.2f} SE, var {(var - mag * mag / 3) / se_var:+.2f} SE, "
              f"against HF's draw {(var - gold['x_var'][i]) / se_var:+.2f} SE")
        assert abs(mean) <= 6 * se_mean
        assert abs(var - mag * mag / 3.0) <= 6 * se_var
        assert abs(var - float(gold["x_var"][i])) <= 6 * se_var
        # HF's own draw obeys its bounds (its fp32 mag_norm): the recorded file is what it claims to be
        hf_mag = float(gold["mag_norm"][i])
        assert -hf_mag <= gold["x_min"][i] and gold["x_max"][i] <= hf_mag and abs(gold["x_mean"][i]) <= 6 * se_mean


def test_levels_are_odd_symmetric_and_cover_the_range():
    t = R.levels(N // 64, 64, seed=17, call=2)
    assert t.min() >= -65535 and t.max() <= 65535 and (t & 1).all()
    assert t.min() < -65000 and t.max() > 65000
    n = R.noise(4, 8, np.float32(3e-6), 17, 2)
    assert n.dtype == np.float32 and (n == R.levels(4, 8, 17, 2).astype(np.float32) * np.float32(3e-6)).all()


def test_noise_depends_on_seed_call_and_index_alone():
    M, H, s = 37, 72, R.scale(5.0, 16, 72)
    a = R.noise(M, H, s, seed=11, call=5, index0=64)
    assert (a == R.noise(M, H, s, seed=11, call=5, index0=64)).all()
    for other in (dict(seed=12, call=5, index0=64), dict(seed=11 + (1 << 32), call=5, index0=64),  # both halves of the seed
                  dict(seed=11, call=6, index0=64), dict(seed=11, call=5, index0=72)):
        b = R.noise(M, H, s, **other)
        assert (a != b).mean() > 0.99, other
    # the index is the flat one: a launch at index0 = 8 rows further down draws what rows 8.. of this one drew
    assert (R.noise(M - 8, H, s, 11, 5, index0=64 + 8 * H) == a[8:]).all()
    # the high word of the counter is part of it
    assert (R.noise(4, 8, s, 11, 5, index0=1 << 35) != R.noise(4, 8, s, 11, 5, index0=0)).mean() > 0.9
    # never the bits of a dropout site under the same seed and call
    from tests.dropout_ref import r16
    idx = np.arange(4096, dtype=np.int64)
    for site in (0, 1, 2, 47):
        assert (r16(11, 5, site, idx) != r16(11, 5, R.SITE, idx)).mean() > 0.99


def test_embed_restatement_rounds_once():
    g = np.random.default_rng(0)
    E_ = R.bf16_to_f32(R.bf16_bits(g.normal(0, 0.02, (9, 16)).astype(np.float32)))
    P_ = R.bf16_to_f32(R.bf16_bits(g.normal(0, 0.02, (7, 16)).astype(np.float32)))
    ids = np.array([0, 3, 8, -1, 9, 2], dtype=np.int64)  # -1 and 9 read row 0
    assert (R.rows(ids, 9) == [0, 3, 8, 0, 0, 2]).all()
    assert (R.embed(ids, E_, np.float32(0), 1, 1) == R.bf16_bits(E_[R.rows(ids, 9)])).all()  # s = 0: the plain gather
    out = R.embed(ids, E_, np.float32(1e-6), 1, 1, P=P_, T=4, position_ids=np.array([0, 1, 2, 3, 4, 40]))
    assert (R.pos_rows(6, 4, 7, np.array([0, 1, 2, 3, 4, 40])) == [2, 3, 4, 5, 6, 6]).all()
    assert out.shape == (6, 16) and out.dtype == np.uint16
    assert (R.bf16_bits(np.float32([1.0, 1.00390625, 1.01171875])) == [0x3F80, 0x3F80, 0x3F82]).all()  # ties to even


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_symbols_exported_and_bound():
    lib = E.load_library()
    for name in ("slam_set_neftune", "slam_op_embed_noise_fwd"):
        assert name in E.header_symbols() and hasattr(lib, name), name
    assert hasattr(E.Engine, "set_neftune") and hasattr(E.Engine, "arm_neftune")


@pytest.mark.parametrize("desc,arch", [(SLAM358M, (0, 0)), (OPT125M, (1, 2048)), (SLAM358M, (3, 0))], ids=["qwen2", "opt", "qwen3"])
def test_set_neftune_and_option_ranges(desc, arch):
    eng = E.Engine(E.SlamModelDesc(*desc), *arch)
    for bad in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(E.EngineError, match="neftune alpha"):
            eng.set_neftune(bad, 0)
        assert E.load_library().slam_set_neftune(eng.h, C.c_float(bad), 0) == E_INVAL
    for ok in (0.0, 5.0, 15.0, 1e-3):
        eng.set_neftune(ok, seed=(1 << 64) - 1)
    for alpha in (0.0, 5.0):  # the range is checked whether or not the arming is ignored
        eng.set_neftune(alpha, 3)
        for bad in (-1, 1 << 32, 1 << 40):
            with pytest.raises(E.EngineError, match="out of range"):
                eng.arm_neftune(bad)
        eng.arm_neftune(0)
        eng.arm_neftune((1 << 32) - 1)
    assert E.load_library().slam_set_neftune(None, C.c_float(5.0), 0) == E_INVAL
    eng.close()


def test_set_neftune_keeps_the_workspace_bound_and_refusals_stay_refusals():
    """slam_set_neftune adds no buffer: the workspace size does not move and a bound one stays bound. Forwards that are refused
    stay refused with the same codes when armed (that they use the arming up is checked where a forward can run: on the GPU)."""
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*OPT125M), 1, 2048)
    h = eng.h
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below returns before a launch

    def forward(B, T):
        return lib.slam_forward(h, fake, None, None, None, None, B, T, 1.0, None, None, None)

    n0 = lib.slam_workspace_bytes(h, 256)
    assert lib.slam_bind_params(h, fake, None) == 0
    assert lib.slam_bind_workspace(h, fake, n0, 256) == 0
    assert forward(2, 256) == E_NOMEM  # bound: past the state check, refused for its size
    eng.set_neftune(5.0, 9)
    assert lib.slam_workspace_bytes(h, 256) == n0
    assert forward(2, 256) == E_NOMEM  # still bound
    eng.arm_neftune(7)
    assert forward(2, 256) == E_NOMEM
    eng.arm_neftune(7)
    assert lib.slam_forward(h, None, None, None, None, None, 1, 64, 0.0, None, None, None) == E_INVAL
    eng.arm_neftune(7)
    assert lib.slam_forward_unpadded(h, fake, None, fake, 2, 64, 100, fake, 1 << 20, 0.0, None, None, None) == E_INVAL  # M_packed % 64
    eng.set_neftune(0.0, 9)
    assert lib.slam_workspace_bytes(h, 256) == n0 and forward(2, 256) == E_NOMEM
    eng.close()


def test_op_refuses_bad_arguments():
    fn = E.load_library().slam_op_embed_noise_fwd
    ids, Ew, Pw, out = (C.c_void_p((1 + i) << 20) for i in range(4))  # never dereferenced: every call returns before a launch
    s = C.c_float(1e-6)

    def call(ids=ids, E_=Ew, P=None, out=out, M=8, H=64, V=16, T=4, NP=10, s=s, seed=0, call=0, index0=0):
        return fn(ids, None, E_, P, out, None, M, H, V, T, NP, s, seed, call, index0, None)

    assert call(ids=None) == E_INVAL and call(E_=None) == E_INVAL and call(out=None) == E_INVAL
    assert call(M=0) == E_INVAL and call(M=-3) == E_INVAL
    assert call(H=60) == E_INVAL and call(H=0) == E_INVAL  # H % 8
    for bad in (-1e-6, float("inf"), float("nan")):
        assert call(s=C.c_float(bad)) == E_INVAL
    assert call(call=-1) == E_INVAL and call(call=1 << 32) == E_INVAL
    assert call(index0=-8) == E_INVAL and call(index0=4) == E_INVAL and call(index0=(1 << 35) + 1) == E_INVAL
    assert call(P=Pw, T=0) == E_INVAL and call(P=Pw, NP=0) == E_INVAL  # a position table needs its sizes


# ------------------------------------------------------------------------------------------- arguments, trainer and CLI
def test_training_arguments_carry_the_field():
    from slamkit_amd.trainer import SLAMTrainingArguments
    from slamkit_amd.trainer.slam_dpo_trainer import DPOConfig, SLAMDPOTrainer
    assert SLAMTrainingArguments().neftune_noise_alpha is None and DPOConfig().neftune_noise_alpha is None  # HF's default
    assert SLAMTrainingArguments(neftune_noise_alpha=5).neftune_noise_alpha == 5
    assert SLAMTrainingArguments(neftune_noise_alpha=0.0).neftune_noise_alpha == 0.0
    for bad in (-1, -0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="neftune_noise_alpha"):
            SLAMTrainingArguments(neftune_noise_alpha=bad)
    with pytest.raises(ValueError, match="neftune_noise_alpha"):
        SLAMDPOTrainer(model=None, args=DPOConfig(neftune_noise_alpha=5.0))
    # a reference-style config: the training_args mapping as its YAML holds it, field included
    cfg = dict(output_dir="./results", learning_rate=1e-3, lr_scheduler_type="cosine_with_min_lr",
               lr_scheduler_kwargs={"min_lr": 5e-5}, warmup_ratio=0.01, max_grad_norm=0.5, bf16=True, num_train_epochs=1,
               per_device_train_batch_size=8, gradient_accumulation_steps=1, eval_strategy="steps", eval_steps=1000,
               neftune_noise_alpha=5)
    assert SLAMTrainingArguments(**cfg).neftune_noise_alpha == 5


def test_cli_override_reaches_the_arguments():
    from slamkit_amd.trainer import SLAMTrainingArguments
    from slamkit_amd.utils.config import load_config, to_container
    known = SLAMTrainingArguments.__dataclass_fields__
    for top in ("train", "train_inter_scale"):
        assert to_container(load_config(top).training_args)["neftune_noise_alpha"] is None, top
    ta = to_container(load_config("train", ["training_args.neftune_noise_alpha=5"]).training_args)
    assert SLAMTrainingArguments(**{k: v for k, v in ta.items() if k in known}).neftune_noise_alpha == 5


def _recorder():
    from tests.test_trainer_dp_gloo import StubLM

    class Rec(StubLM):
        def __init__(self):
            super().__init__()
            self.training = False
            self.events = []  # ("set", alpha, seed) | ("call", n) | ("fwd", training)

        def set_neftune(self, alpha, seed=None):
            self.events.append(("set", float(alpha or 0.0), seed))

        def set_neftune_state(self, seed=None, call=None):
            self.events.append(("call", call))

        def forward(self, **kw):
            self.events.append(("fwd", self.training))
            return super().forward(**kw)

        def train(self, mode=True):
            self.training = mode
            return self

        def eval(self):
            return self.train(False)

    return Rec()


def _trainer(tmp_path, model, alpha, max_steps=3, ga=2, seed=5, eval_rows=None, **kw):
    from slamkit_amd.data import DataCollatorForLanguageModeling
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import make_rows
    args = SLAMTrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=2, gradient_accumulation_steps=ga,
                                 learning_rate=1e-2, warmup_steps=1, warmup_ratio=0.0, max_steps=max_steps, logging_steps=0,
                                 seed=seed, save_steps=0, neftune_noise_alpha=alpha, **kw)
    return SLAMTrainer(model=model, args=args, data_collator=DataCollatorForLanguageModeling(pad_token_id=0),
                       train_dataset=make_rows(), eval_dataset=eval_rows)


def test_trainer_switches_on_numbers_the_calls_and_switches_off(tmp_path):
    from slamkit_amd.trainer.slam_trainer import dropout_seed
    from tests.test_trainer_dp_gloo import make_rows
    m = _recorder()
    tr = _trainer(tmp_path, m, 5.0, eval_rows=make_rows(6, seed=9), eval_strategy="steps", eval_steps=2)
    assert m.events == []  # constructing the trainer switches nothing on: train() does, as HF's Trainer attaches its hook
    tr.train()
    assert m.events[0] == ("set", 5.0, dropout_seed(5, 0)) and m.events[-1] == ("set", 0.0, None)
    assert [e for e in m.events if e[0] == "set"] == [m.events[0], m.events[-1]]
    assert [e[1] for e in m.events if e[0] == "call"] == [0, 1, 2, 3, 4, 5]  # step * GA + micro-batch
    # every training forward follows its own call number; evaluate() inside train() runs in eval mode, without one
    fw = [i for i, e in enumerate(m.events) if e[0] == "fwd"]
    train_fw = [i for i in fw if m.events[i][1]]
    assert len(train_fw) == 6 and all(m.events[i - 1][0] == "call" for i in train_fw)
    eval_fw = [i for i in fw if not m.events[i][1]]
    assert eval_fw and all(m.events[i - 1][0] != "call" for i in eval_fw)
    # a run resumed at step k continues at k * GA
    m2 = _recorder()
    tr2 = _trainer(tmp_path, m2, 5.0)
    tr2.state.global_step = 2
    tr2.train()
    assert [e[1] for e in m2.events if e[0] == "call"] == [4, 5]


def test_trainer_switches_off_when_training_raises(tmp_path):
    m = _recorder()
    tr = _trainer(tmp_path, m, 5.0)

    def boom(*a, **k):
        raise RuntimeError("boom")

    tr.optimizer_step = boom
    with pytest.raises(RuntimeError, match="boom"):
        tr.train()
    assert m.events[0][:2] == ("set", 5.0) and m.events[-1] == ("set", 0.0, None)


@pytest.mark.parametrize("alpha", [None, 0, 0.0])
def test_trainer_without_the_option_touches_nothing(tmp_path, alpha):
    m = _recorder()
    _trainer(tmp_path, m, alpha).train()
    assert [e for e in m.events if e[0] != "fwd"] == []


def test_trainer_refuses_a_model_without_the_kernel(tmp_path):
    from tests.test_trainer_dp_gloo import StubLM
    with pytest.raises(ValueError, match="neftune_noise_alpha"):
        _trainer(tmp_path, StubLM(), 5.0)
    _trainer(tmp_path, StubLM(), None)
