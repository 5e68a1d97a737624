"""CPU checks of the HF weight-decay rule (weight_decay_rule = "hf"): UnitLM.hf_decay_flags() against the names HF's Trainer
decays (tests/golden/decay_names.json, written by make_golden_decay_names.py), the slam_set_decay_mask entry point's argument
checks and binding, and the trainer argument."""
import ctypes as C
import json
import os
import re

import pytest

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import UnitLM, UnitLMConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = ["qwen2_tied", "qwen2_untied", "opt"]


def _fixture(key):
    with open(os.path.join(GOLDEN, "decay_names.json")) as f:
        return json.load(f)["models"][key]


def _host_model(config_dir):
    """A UnitLM without a GPU: the key map only needs the engine's tensor table."""
    with open(os.path.join(GOLDEN, config_dir, "config.json")) as f:
        hf_cfg = json.load(f)
    cfg = UnitLMConfig(base_model_name="local", base_config=hf_cfg, vocab_size=502)
    m = UnitLM.__new__(UnitLM)
    m.config = cfg
    m.engine = E.Engine(cfg.engine_desc(), *cfg.engine_arch(), flags=cfg.engine_flags())
    m._build_key_map()
    return m


def _names_by_tensor(m):
    """engine tensor name -> the HF names (without the `lm.` prefix) the key map puts into it"""
    specs = sorted(m.engine.tensors.values(), key=lambda t: t.offset)
    out = {t.name: [] for t in specs}
    for key, ent in m.key_map.items():
        owner = [t for t in specs if t.offset <= ent[0] < t.offset + t.numel]
        assert len(owner) == 1, key
        assert key.startswith("lm.")
        out[owner[0].name].append(key[3:])
    return out


def _check_against(m, parameters, decay):
    flags = m.hf_decay_flags()
    assert len(flags) == len(m.engine.tensors)
    by_tensor = _names_by_tensor(m)
    assert sorted(n for ns in by_tensor.values() for n in ns) == sorted(parameters)  # every HF parameter, exactly once
    for (name, _), flag in zip(m.engine.tensors.items(), flags):
        inside = {n in decay for n in by_tensor[name]}
        assert len(inside) == 1, f"{name}: HF names {by_tensor[name]} are split by the decay set"
        assert flag == inside.pop(), name
    return dict(zip(m.engine.tensors, flags))


@pytest.mark.parametrize("key", MODELS)
def test_hf_decay_flags_reproduce_the_fixture(key):
    fx = _fixture(key)
    m = _host_model(fx["config"])
    flags = _check_against(m, fx["parameters"], set(fx["decay"]))
    last = max(int(n.split(".")[1]) for n in flags if n.startswith("layers."))
    assert flags["embed"] and not flags["norm"] and not flags["layers.0.ln1"]
    assert not flags[f"layers.{last}.bqkv"] and flags[f"layers.{last}.wqkv"]
    if key == "qwen2_untied":
        assert flags["lm_head"]
    if key == "opt":
        assert flags["pos_embed"]  # a cols == 1 group of the optimizer's walk that IS decayed
        assert not any(flags[f"layers.0.{k}"] for k in ("ln1", "ln1_b", "bqkv", "bo", "ln2", "ln2_b", "b1", "b2")) and not flags["norm_b"]
        assert all(flags[f"layers.0.{k}"] for k in ("wqkv", "wo", "w1", "w2"))
    else:
        assert all(flags[f"layers.0.{k}"] for k in ("wqkv", "wo", "wgu", "wd")) and not flags["layers.0.ln2"]
    m.engine.close()


@pytest.mark.parametrize("key", MODELS)
def test_hf_decay_flags_match_live_transformers(key):
    transformers = pytest.importorskip("transformers")
    fx = _fixture(key)
    cfg = transformers.AutoConfig.from_pretrained(os.path.join(GOLDEN, fx["config"]))
    hf = transformers.AutoModelForCausalLM.from_config(cfg)
    decay = transformers.Trainer.get_decay_parameter_names(None, hf)
    names = [n for n, _ in hf.named_parameters()]
    assert (names, decay) == (fx["parameters"], fx["decay"])  # the fixture is what this transformers computes
    m = _host_model(fx["config"])
    _check_against(m, names, set(decay))
    m.engine.close()


def test_a_fused_tensor_with_split_names_is_refused():
    m = _host_model("hf_text_lm")
    k = "lm.model.layers.0.self_attn.q_proj.weight"
    m.key_map["lm.model.layers.0.self_attn.q_proj.bias_like"] = m.key_map[k]  # a no-decay name inside the decayed wqkv
    with pytest.raises(AssertionError, match="disagree"):
        m.hf_decay_flags()
    m.engine.close()


def test_set_decay_mask_argument_checks():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(2, 64, 1, 1, 64, 128, 502, 0, 1e-6, 10000.0))
    n = len(eng.tensors)
    assert n == lib.slam_tensor_count(eng.h)
    ones = (C.c_uint8 * (n + 1))(*([1] * (n + 1)))
    assert lib.slam_set_decay_mask(eng.h, ones, n - 1) == -1  # SLAM_EINVAL
    assert b"slam_tensor_count" in lib.slam_last_error(eng.h)
    assert lib.slam_set_decay_mask(eng.h, ones, n + 1) == -1
    assert lib.slam_set_decay_mask(None, ones, n) == -1
    assert lib.slam_set_decay_mask(eng.h, ones, n) == 0          # every tensor decayed: no range, nothing to upload
    assert lib.slam_set_decay_mask(eng.h, None, n) == 0          # NULL clears
    eng.set_decay_mask(None)
    with pytest.raises(E.EngineError):
        eng.set_decay_mask([1] * (n - 1))
    eng.close()


def test_set_decay_mask_is_declared_exported_and_bound():
    assert "slam_set_decay_mask" in E.header_symbols()
    lib = E.load_library()
    fn = lib.slam_set_decay_mask
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32]
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "slam_engine.h")).read()
    assert re.search(r"int slam_set_decay_mask\(SlamEngine\* h, const uint8_t\* decay, int32_t n_tensors\);", hdr)


class _RecordingEngine:
    def __init__(self, inner):
        self.inner, self.masks = inner, []
        self.n_params = inner.n_params

    def set_decay_mask(self, flags):
        self.masks.append(flags)

    def __getattr__(self, k):
        return getattr(self.inner, k)


def _stub_trainer(**kw):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import StubLM
    model = StubLM()
    model.engine = _RecordingEngine(model.engine)
    model.hf_decay_flags = lambda: [True, False]
    args = SLAMTrainingArguments(logging_steps=0, **kw)
    return SLAMTrainer(model=model, args=args), model


def test_weight_decay_rule_argument():
    from slamkit_amd.trainer import DPOConfig, SLAMTrainer, SLAMTrainingArguments
    assert SLAMTrainingArguments().weight_decay_rule == "all" and DPOConfig(weight_decay_rule="hf").weight_decay_rule == "hf"
    with pytest.raises(ValueError, match="weight_decay_rule"):
        SLAMTrainingArguments(weight_decay_rule="bogus")
    _, model = _stub_trainer(weight_decay=0.1)
    assert model.engine.masks == []  # "all" makes no engine call at all
    _, model = _stub_trainer(weight_decay=0.1, weight_decay_rule="hf")
    assert model.engine.masks == [[True, False]]  # set once, at init
    # a field set after construction gets past the arguments' own check: the trainer checks again
    args = SLAMTrainingArguments(logging_steps=0)
    args.weight_decay_rule = "bogus"
    from tests.test_trainer_dp_gloo import StubLM
    with pytest.raises(ValueError, match="weight_decay_rule"):
        SLAMTrainer(model=StubLM(), args=args)
    args.weight_decay_rule = "hf"
    with pytest.raises(ValueError, match="hf_decay_flags"):
        SLAMTrainer(model=StubLM(), args=args)  # a model that cannot name its tensors


def test_cli_override_reaches_the_arguments():
    from slamkit_amd.trainer import SLAMTrainingArguments
    from slamkit_amd.utils.config import load_config, to_container
    cfg = load_config("train", ["training_args.weight_decay_rule=hf", "training_args.weight_decay=0.1"])
    known = SLAMTrainingArguments.__dataclass_fields__
    args = SLAMTrainingArguments(**{k: v for k, v in to_container(cfg.training_args).items() if k in known})
    assert args.weight_decay_rule == "hf" and args.weight_decay == 0.1
    assert load_config("train", []).training_args.get("weight_decay_rule") is None  # the shipped recipes stay as they are
