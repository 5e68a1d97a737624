"""CPU tier of residual dropout (engine options "dropout_thr16" / "dropout_seed" / "dropout_call_next", OPT only): option
ranges and refusals, the workspace each setting asks for, the unbind rule, how the model config carries the probability, the
drop rate of the restated mask and the trainer's call numbering. Engine creation and sizing are host-only."""
import ctypes as C
import math

import numpy as np
import pytest

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS, UnitLMConfig, base_config_from_hf, dropout_thr16
from tests import dropout_ref as R

E_INVAL, E_STATE, E_NOMEM = -1, -2, -3
OPT125M = (12, 768, 12, 12, 64, 3072, 502, 1, 1e-5, 10000.0)
SLAM358M = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
OPT_HF = dict(model_type="opt", num_hidden_layers=2, hidden_size=256, num_attention_heads=4, ffn_dim=512,
              max_position_embeddings=128, init_std=0.02, tie_word_embeddings=True)


def _opt():
    return E.Engine(E.SlamModelDesc(*OPT125M), 1, 2048)


def test_symbols_exported_and_bound():
    lib = E.load_library()
    for n in ("slam_op_dropout_add", "slam_op_dropout_bwd"):
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n


def test_option_ranges():
    eng = _opt()
    for v in (0, 1, 6554, 65535, 0):
        eng.set_option("dropout_thr16", v)
    for v in (-1, 65536, 1 << 20):
        with pytest.raises(E.EngineError, match="out of range"):
            eng.set_option("dropout_thr16", v)
    for v in (0, 1, -1, (1 << 63) - 1, -(1 << 63)):
        eng.set_option("dropout_seed", v)
    eng.set_dropout_seed((1 << 64) - 1)  # 64 unsigned bits through the int64 argument
    eng.set_option("dropout_thr16", 6554)
    for v in (0, 7, (1 << 32) - 1):
        eng.set_option("dropout_call_next", v)
    for v in (-1, 1 << 32):
        with pytest.raises(E.EngineError, match="out of range"):
            eng.set_option("dropout_call_next", v)
    eng.set_option("dropout_thr16", 0)
    eng.set_option("dropout_call_next", 3)  # accepted and ignored while dropout is off
    with pytest.raises(E.EngineError, match="out of range"):
        eng.set_option("dropout_call_next", -1)
    eng.close()


def test_qwen2_refuses_dropout():
    eng = E.Engine(E.SlamModelDesc(*SLAM358M))
    eng.set_option("dropout_thr16", 0)
    with pytest.raises(E.EngineError, match="OPT"):
        eng.set_option("dropout_thr16", 6554)
    eng.close()


def test_op_entry_points_refuse_bad_arguments():
    lib = E.load_library()
    fake, other = C.c_void_p(1 << 20), C.c_void_p(1 << 21)  # never dereferenced: every call returns before a launch
    for fn in (lib.slam_op_dropout_add, lib.slam_op_dropout_bwd):
        assert fn(None, other, 8, 64, 1, 0, 0, 0, 0, None) == E_INVAL
        assert fn(fake, None, 8, 64, 1, 0, 0, 0, 0, None) == E_INVAL
        assert fn(fake, other, 0, 64, 1, 0, 0, 0, 0, None) == E_INVAL
        assert fn(fake, other, 8, 60, 1, 0, 0, 0, 0, None) == E_INVAL      # H not a multiple of 8
        assert fn(fake, other, 8, 64, 65536, 0, 0, 0, 0, None) == E_INVAL  # threshold
        assert fn(fake, other, 8, 64, -1, 0, 0, 0, 0, None) == E_INVAL
        assert fn(fake, other, 8, 64, 1, 0, -1, 0, 0, None) == E_INVAL     # call
        assert fn(fake, other, 8, 64, 1, 0, 1 << 32, 0, 0, None) == E_INVAL
        assert fn(fake, other, 8, 64, 1, 0, 0, -1, 0, None) == E_INVAL     # stream id
        assert fn(fake, other, 8, 64, 1, 0, 0, 0, 4, None) == E_INVAL      # index0 not a multiple of 8
        assert fn(fake, other, 8, 64, 1, 0, 0, 0, -8, None) == E_INVAL
    assert lib.slam_op_dropout_bwd(fake, fake, 8, 64, 1, 0, 0, 0, 0, None) == E_INVAL  # dy must stay intact: another buffer


@pytest.mark.parametrize("tokens", [256, 8192])
def test_workspace_size(tokens):
    plain, eng = _opt(), _opt()
    n0 = plain.workspace_bytes(tokens)
    eng.set_option("dropout_thr16", 0)
    assert eng.workspace_bytes(tokens) == n0
    eng.set_option("dropout_seed", 99)
    assert eng.workspace_bytes(tokens) == n0
    sizes = []
    for thr in (1, 6554, 65535):
        eng.set_option("dropout_thr16", thr)
        sizes.append(eng.workspace_bytes(tokens))
    assert sizes[0] == sizes[1] == sizes[2]  # the layout depends only on whether the value is non-zero
    assert sizes[0] == n0 + 4 * tokens * 768 * 2  # four [tokens][hidden] bf16 buffers (256-byte multiples at these sizes)
    for level in (1, 2):  # independent of the recompute level's own savings
        plain.set_option("recompute", level)
        eng.set_option("recompute", level)
        assert eng.workspace_bytes(tokens) == plain.workspace_bytes(tokens) + 4 * tokens * 768 * 2
    eng.set_option("dropout_thr16", 0)
    assert eng.workspace_bytes(tokens) == plain.workspace_bytes(tokens)
    plain.close()
    eng.close()


def test_zero_nonzero_change_unbinds_workspace():
    lib = E.load_library()
    eng = _opt()
    h = eng.h
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below returns before a launch

    def forward(B, T):
        return lib.slam_forward(h, fake, None, None, None, None, B, T, 1.0, None, None, None)

    def bind():
        n = lib.slam_workspace_bytes(h, 256)
        assert lib.slam_bind_workspace(h, fake, n, 256) == 0
        return n

    assert lib.slam_bind_params(h, fake, None) == 0
    n0 = bind()
    assert forward(2, 256) == E_NOMEM  # bound: past the state check, refused for its size
    eng.set_option("dropout_thr16", 0)  # no change: still bound
    assert forward(2, 256) == E_NOMEM
    eng.set_option("dropout_thr16", 6554)  # zero -> non-zero: the layout changed
    assert forward(2, 256) == E_STATE
    assert b"workspace" in lib.slam_last_error(h)
    assert lib.slam_backward(h, 1.0, 0, E.BUCKET_CB(), None, None) == E_STATE
    n1 = bind()
    assert n1 > n0
    assert forward(2, 256) == E_NOMEM
    eng.set_option("dropout_thr16", 32768)  # non-zero -> non-zero: still bound
    assert forward(2, 256) == E_NOMEM
    eng.set_option("dropout_seed", 5)
    eng.set_option("dropout_call_next", 1)
    assert forward(2, 256) == E_NOMEM
    eng.set_option("dropout_thr16", 0)  # non-zero -> zero
    assert forward(2, 256) == E_STATE
    assert bind() == n0
    assert forward(2, 256) == E_NOMEM
    eng.close()


def test_config_carries_dropout():
    assert base_config_from_hf(OPT_HF)["dropout"] == 0.0  # absent means 0.0
    b = base_config_from_hf({**OPT_HF, "dropout": 0.1})
    assert b["dropout"] == 0.1
    assert base_config_from_hf(b) == b  # idempotent
    # ignored as before, whatever they say
    assert base_config_from_hf({**OPT_HF, "attention_dropout": 0.1, "layerdrop": 0.1, "activation_dropout": 0.1}) == base_config_from_hf(OPT_HF)
    for name in ("facebook/opt-125m", "facebook/opt-1.3b"):  # the hub-less table carries none
        assert "dropout" not in KNOWN_BASE_CONFIGS[name]
        assert UnitLMConfig(base_model_name=name).dropout == 0.0
    assert UnitLMConfig(base_model_name="facebook/opt-125m", dropout=0.1).dropout == 0.1  # the kwarg override
    c = UnitLMConfig(base_model_name="local", base_config={**OPT_HF, "dropout": 0.1})
    assert c.dropout == 0.1 and c.base_config["dropout"] == 0.1
    assert UnitLMConfig(base_model_name="local", base_config={**OPT_HF, "dropout": 0.1}, dropout=0.0).dropout == 0.0
    d = c.to_dict()  # the round trip of a checkpoint's config.json
    c2 = UnitLMConfig(base_model_name="local", base_config=d["base_config"], vocab_size=d["vocab_size"])
    assert c2.dropout == 0.1 and c2.to_dict() == d
    with pytest.raises(ValueError, match="dropout"):
        UnitLMConfig(base_model_name="local", base_config={**OPT_HF, "dropout": 1.0})
    with pytest.raises(ValueError, match="dropout"):
        UnitLMConfig(base_model_name="local", base_config=OPT_HF, dropout=-0.1)


def test_qwen2_config_refuses_dropout():
    assert UnitLMConfig().dropout == 0.0
    assert UnitLMConfig(dropout=0.0).dropout == 0.0
    with pytest.raises(ValueError, match="OPT only"):
        UnitLMConfig(dropout=0.1)


def test_threshold_and_scale():
    assert dropout_thr16(0.1) == R.thr16(0.1) == 6554
    assert dropout_thr16(0.0) == 0 and dropout_thr16(0.5) == 32768
    assert R.scale(32768) == np.float32(2.0) and R.scale(0) == np.float32(1.0)
    assert R.scale(65535) == np.float32(65536.0)
    assert abs(float(R.scale(6554)) - 1.0 / (1.0 - 6554 / 65536)) < 1e-7


@pytest.mark.parametrize("stream", [0, 1, 2, 3])
def test_drop_rate(stream):
    M, H, thr = 300, 768, 6554
    keep = R.keep_mask(M, H, thr, seed=1234, call=7, stream=stream)
    n, q = M * H, thr / 65536.0
    rate = 1.0 - keep.mean()
    sigma = math.sqrt(q * (1.0 - q) / n)
    print(f"stream {stream}: drop rate {rate:.6f}, q {q:.6f}, {abs(rate - q) / sigma:.2f} sigma")
    assert abs(rate - q) <= 5.0 * sigma


def test_mask_depends_on_every_key_field():
    M, H, thr = 16, 64, 32768
    base = R.keep_mask(M, H, thr, 1234, 7, 0)
    assert (R.keep_mask(M, H, thr, 1234, 7, 0) == base).all()
    for other in (R.keep_mask(M, H, thr, 1235, 7, 0), R.keep_mask(M, H, thr, 1234 + (1 << 32), 7, 0),
                  R.keep_mask(M, H, thr, 1234, 8, 0), R.keep_mask(M, H, thr, 1234, 7, 1),
                  R.keep_mask(M, H, thr, 1234, 7, 0, index0=(1 << 35) + 8)):
        assert (other != base).mean() > 0.3
    # index0 shifts the window over one stream of bits
    assert (R.keep_mask(M, H, thr, 1234, 7, 0, index0=64)[:-1] == base[1:]).all()
    # a lower threshold only ever keeps more
    assert (R.keep_mask(M, H, 6554, 1234, 7, 0) | ~base).all()


class _Recorder:
    """What SLAMTrainer needs of a model, recording the dropout state it is given (tests/test_trainer_dp_gloo.StubLM)."""

    def __new__(cls):
        from tests.test_trainer_dp_gloo import StubLM

        class Rec(StubLM):
            def __init__(self):
                super().__init__()
                self.seeds, self.calls, self.training, self.modes = [], [], True, []

            def set_dropout_state(self, seed=None, call=None):
                if seed is not None:
                    self.seeds.append(seed)
                if call is not None:
                    self.calls.append(call)

            def forward(self, **kw):
                self.modes.append(self.training)
                return super().forward(**kw)

            def train(self, mode=True):
                self.training = mode
                return self

            def eval(self):
                return self.train(False)

        return Rec()


def _trainer(tmp_path, model, max_steps, ga=2, seed=5, eval_rows=None):
    from slamkit_amd.data import DataCollatorForLanguageModeling
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import make_rows
    args = SLAMTrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=2, gradient_accumulation_steps=ga,
                                 learning_rate=1e-2, warmup_steps=1, warmup_ratio=0.0, max_steps=max_steps, logging_steps=0,
                                 seed=seed, save_steps=0)
    return SLAMTrainer(model=model, args=args, data_collator=DataCollatorForLanguageModeling(pad_token_id=0),
                       train_dataset=make_rows(), eval_dataset=eval_rows)


def test_trainer_call_numbering(tmp_path):
    from slamkit_amd.trainer.slam_trainer import dropout_seed
    m = _Recorder()
    tr = _trainer(tmp_path, m, max_steps=4, ga=2)
    assert m.seeds == [dropout_seed(5, 0)] and m.seeds[0] & 0xFFFFFFFF == 5
    m.eval()  # train() puts the model into training mode itself, as the reference's Trainer does
    tr.train()
    assert m.training is True and all(m.modes)
    assert m.calls == [0, 1, 2, 3, 4, 5, 6, 7]  # call = step * GA + i
    # a run resumed at step k (what _load_checkpoint restores) continues at k * GA
    m2 = _Recorder()
    tr2 = _trainer(tmp_path, m2, max_steps=4, ga=2)
    tr2.state.global_step = 2
    tr2.train()
    assert m2.calls == [4, 5, 6, 7]
    m3 = _Recorder()
    tr3 = _trainer(tmp_path, m3, max_steps=3, ga=3)
    tr3.train()
    assert m3.calls == list(range(9))


def test_dropout_seed_mixes_rank_injectively():
    from slamkit_amd.trainer.slam_trainer import dropout_seed
    seen = {dropout_seed(s, r) for s in (0, 1, 5, (1 << 32) - 1) for r in (0, 1, 2, 7)}
    assert len(seen) == 16
    # never the key the stochastic rounding draws from (its seed defaults to args.seed itself)
    assert all(dropout_seed(s, 0) != s for s in (0, 1, 5, (1 << 32) - 1))
    assert all(dropout_seed(s, 0) >> 32 == 0x44524F50 for s in (0, 5))
    assert all(0 <= v < (1 << 64) for v in seen)


def test_evaluate_runs_in_eval_mode_and_restores(tmp_path):
    from tests.test_trainer_dp_gloo import make_rows
    m = _Recorder()
    tr = _trainer(tmp_path, m, max_steps=1, eval_rows=make_rows(6, seed=9))
    tr.evaluate()
    assert m.modes and not any(m.modes) and m.training is True
    m.modes.clear()
    m.eval()
    tr.evaluate()
    assert not any(m.modes) and m.training is False  # the previous mode comes back, whichever it was
