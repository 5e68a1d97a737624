"""CPU tier of activation recomputation (engine option "recompute", HF's gradient_checkpointing): the option's range, the
workspace each level asks for, the unbind rule and the trainer flag. Engine creation and sizing are host-only."""
import ctypes as C
import glob
import os

import pytest

from slamkit_amd import engine as E
from slamkit_amd.trainer import SLAMTrainingArguments
from slamkit_amd.trainer.slam_dpo_trainer import DPOConfig
from slamkit_amd.utils.config import CONFIG_DIR, load_config, _load_file, to_container

E_INVAL, E_STATE, E_NOMEM = -1, -2, -3
UNTIED = 1  # SLAM_MODEL_UNTIED_HEAD

# (description, arch, n_positions, flags, tokens, workspace bytes of the parent commit's build at level 0)
QWEN7B = ((28, 3584, 28, 4, 128, 18944, 152064, 0, 1e-6, 1000000.0), 0, 0, UNTIED, 16384, 82224492800)
SLAM358M = ((24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0), 0, 0, 0, 8192, 8383851008)
OPT125M = ((12, 768, 12, 12, 64, 3072, 502, 1, 1e-5, 10000.0), 1, 2048, 0, 8192, 3006952704)
TWO_LAYER = ((2, 128, 2, 2, 64, 256, 502, 0, 1e-6, 10000.0), 0, 0, 0, 512, None)


def _engine(case):
    desc, arch, npos, flags = case[:4]
    return E.Engine(E.SlamModelDesc(*desc), arch, npos, flags=flags)


def _bytes(case, level):
    eng = _engine(case)
    eng.set_option("recompute", level)
    n = eng.workspace_bytes(case[4])
    eng.close()
    return n


def _layer_sizes(case):
    """Per-layer buffers carve() takes at level 0, in bytes, from the description: name -> size."""
    (L, H, nH, nKV, hd, I, *_), arch, _, _, M, _ = case
    QKV = (nH + 2 * nKV) * hd
    s = {"hmid": 2 * M * H, "x1": 2 * M * H, "x2": 2 * M * H, "qkv": 2 * M * QKV, "o": 2 * M * nH * hd,
         "gu": 2 * M * (1 if arch == 1 else 2) * I, "act": 2 * M * I, "rstd1": 4 * M, "rstd2": 4 * M, "lse": 4 * M * nH}
    if arch == 1:
        s["mu1"] = s["mu2"] = 4 * M
    return s


def test_option_range():
    eng = _engine(SLAM358M)
    for v in (0, 1, 2, 1, 0):
        eng.set_option("recompute", v)
    for v in (3, -1):
        with pytest.raises(E.EngineError, match="out of range"):
            eng.set_option("recompute", v)
    eng.close()


@pytest.mark.parametrize("case", [QWEN7B, SLAM358M, OPT125M], ids=["qwen2.5-7b", "slam-358m", "opt-125m"])
def test_workspace_savings(case):
    L, arch, parent = case[0][0], case[1], case[5]
    sizes = _layer_sizes(case)
    a2 = sum(sizes.values())
    shared1 = ("x1", "x2") if arch == 1 else ("x1", "x2", "act")
    a1 = sum(sizes[k] for k in shared1)
    b0, b1, b2 = (_bytes(case, v) for v in (0, 1, 2))
    assert b0 == parent  # the option off changes nothing
    assert b0 - b2 >= (L - 3) * a2 - 256 * len(sizes) * L
    assert b0 - b1 >= (L - 3) * a1 - 256 * len(shared1) * L


def test_issue_arithmetic_7b():
    """The figures the feature was motivated with: 151,672 B per token per layer for the Qwen2.5-7B shape."""
    assert sum(_layer_sizes(QWEN7B).values()) == 151672 * 16384


def test_shallow_model_not_larger():
    b0, b1, b2 = (_bytes(TWO_LAYER, v) for v in (0, 1, 2))
    assert b2 <= b0 and b1 <= b0


def test_level_change_unbinds_workspace():
    lib = E.load_library()
    eng = _engine(SLAM358M)
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
    assert lib.slam_bind_kv_cache(h, fake, lib.slam_kv_cache_bytes(h, 2, 64), 2, 64) == 0
    assert forward(2, 256) == E_NOMEM  # bound: past the state check, refused for its size
    eng.set_option("recompute", 0)      # no change: still bound
    assert forward(2, 256) == E_NOMEM
    for level in (2, 1, 0):
        eng.set_option("recompute", level)
        assert forward(2, 256) == E_STATE
        assert b"workspace" in lib.slam_last_error(h)
        assert lib.slam_prefill(h, fake, fake, 1, 8, fake, None) == E_STATE
        assert lib.slam_decode_step(h, fake, fake, 1, fake, None) == E_STATE
        assert lib.slam_backward(h, 1.0, 0, E.BUCKET_CB(), None, None) == E_STATE
        n = bind()
        assert (n < n0) == (level != 0)
        assert forward(2, 256) == E_NOMEM  # the state error is gone
        assert lib.slam_prefill(h, fake, fake, 1, 512, fake, None) == E_INVAL  # ... for prefill too: refused for the cache's capacity
    eng.close()


def test_training_arguments_flag():
    a = SLAMTrainingArguments()
    assert a.gradient_checkpointing is False and a.recompute_level is None and a.get_recompute_level() == 0
    assert SLAMTrainingArguments(gradient_checkpointing=True).get_recompute_level() == 2
    assert SLAMTrainingArguments(gradient_checkpointing=True, recompute_level=1).get_recompute_level() == 1
    assert SLAMTrainingArguments(recompute_level=2).get_recompute_level() == 2
    assert DPOConfig(gradient_checkpointing=True).get_recompute_level() == 2
    with pytest.raises(ValueError):
        SLAMTrainingArguments(recompute_level=3).get_recompute_level()


def test_shipped_configs_carry_the_key():
    files = sorted(glob.glob(os.path.join(CONFIG_DIR, "training_args", "*.yaml")))
    assert len(files) >= 4
    known = SLAMTrainingArguments.__dataclass_fields__
    for f in files:
        name = os.path.splitext(os.path.basename(f))[0]
        ta = _load_file(os.path.join("training_args", name))
        assert ta["gradient_checkpointing"] is False, name
        args = SLAMTrainingArguments(**{k: v for k, v in ta.items() if k in known})
        assert args.gradient_checkpointing is False and args.get_recompute_level() == 0
    for top in ("train", "train_inter_scale", "preference_alignment_train"):
        assert to_container(load_config(top).training_args)["gradient_checkpointing"] is False
    on = load_config("train", ["training_args.gradient_checkpointing=true", "training_args.recompute_level=1"]).training_args
    assert SLAMTrainingArguments(**{k: v for k, v in to_container(on).items() if k in known}).get_recompute_level() == 1
