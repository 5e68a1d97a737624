"""GPT-NeoX (Pythia) without a GPU: config parsing and refusals, the arch-4 tensor layout, the HF key set and the
query_key_value permutation."""
import ctypes as C

import pytest
import torch
import transformers

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import (KNOWN_BASE_CONFIGS, UnitLM, UnitLMConfig, base_config_from_hf, qkv_engine_to_hf,
                                       qkv_hf_to_engine)


def _tiny(**kw):
    c = dict(model_type="gpt_neox", vocab_size=502, hidden_size=256, num_hidden_layers=2, intermediate_size=1024,
             num_attention_heads=4, rotary_pct=0.25, rotary_emb_base=10000, layer_norm_eps=1e-5, hidden_act="gelu",
             use_parallel_residual=True, attention_bias=True, tie_word_embeddings=False)
    c.update(kw)
    return c


def test_config_parsing():
    b = base_config_from_hf(_tiny())
    assert (b["model_type"], b["head_dim"], b["rotary_ndims"], b["num_key_value_heads"]) == ("gpt_neox", 64, 16, 4)
    assert b["layer_norm_eps"] == 1e-5 and b["rope_theta"] == 10000.0 and b["tie_word_embeddings"] is False
    assert base_config_from_hf(b) == b  # idempotent: what a saved checkpoint's config.json holds
    assert base_config_from_hf(transformers.GPTNeoXConfig(**_tiny()).to_dict()) == b  # the installed HF's own serialisation
    cfg = UnitLMConfig(base_model_name="EleutherAI/pythia-160m")
    assert cfg.engine_arch() == (4, 16) and cfg.engine_flags() == E.MODEL_UNTIED_HEAD and abs(cfg.engine_desc().rms_eps - 1e-5) < 1e-11
    assert all(f"EleutherAI/pythia-{s}" in KNOWN_BASE_CONFIGS for s in ("70m", "160m", "410m", "1.4b"))


@pytest.mark.parametrize("change,word", [
    (dict(use_parallel_residual=False), "use_parallel_residual"), (dict(hidden_act="gelu_new"), "hidden_act"),
    (dict(attention_bias=False), "attention_bias"), (dict(rope_scaling=dict(type="linear", factor=2.0)), "rope_scaling"),
    (dict(attention_dropout=0.1), "attention_dropout"), (dict(hidden_dropout=0.1), "hidden_dropout"),
    (dict(num_attention_heads=8), "head_dim"), (dict(hidden_size=4096, num_attention_heads=32), "hidden_size"),
    (dict(rotary_pct=0.2), "rotary_pct"), (dict(rotary_pct=0.0), "rotary_pct")])
def test_config_refusals_name_the_field(change, word):
    with pytest.raises(ValueError, match=word):
        base_config_from_hf(_tiny(**change))


@pytest.mark.parametrize("name,why", [("EleutherAI/pythia-14m", "head_dim 32"), ("EleutherAI/pythia-31m", "head_dim 32"),
                                      ("EleutherAI/pythia-1b", "head_dim 256"), ("EleutherAI/pythia-2.8b", "above 2048")])
def test_pythia_sizes_outside_the_limits(name, why):
    with pytest.raises(ValueError, match=why):
        UnitLMConfig(base_model_name=name)


def _host_model(**kw):
    m = UnitLM.__new__(UnitLM)
    m.config = UnitLMConfig(base_model_name="local", base_config=_tiny(**kw), vocab_size=502)
    m.engine = E.Engine(m.config.engine_desc(), *m.config.engine_arch(), flags=m.config.engine_flags())
    m._build_key_map()
    return m


def test_arch4_tensor_list():
    t = _host_model().engine.tensors
    H, F = 256, 1024
    layer = [("ln1", H, 1), ("ln1_b", H, 1), ("ln2", H, 1), ("ln2_b", H, 1), ("wqkv", 3 * H, H), ("bqkv", 3 * H, 1), ("wo", H, H),
             ("bo", H, 1), ("w1", F, H), ("b1", F, 1), ("w2", H, F), ("b2", H, 1)]
    want = [("embed", 512, H)] + [(f"layers.{l}.{n}", r, c) for l in range(2) for n, r, c in layer] + \
           [("norm", H, 1), ("norm_b", H, 1), ("lm_head", 512, H)]
    assert [(n, v.rows, v.cols) for n, v in t.items()] == want
    assert "lm_head" not in _host_model(tie_word_embeddings=True).engine.tensors


@pytest.mark.parametrize("rot,n_kv", [(0, 4), (12, 4), (72, 4), (16, 2), (16, 1)])
def test_create_refuses(rot, n_kv):
    d = UnitLMConfig(base_model_name="local", base_config=_tiny(), vocab_size=502).engine_desc()
    d.n_kv_heads = n_kv
    h = C.c_void_p()
    assert E.load_library().slam_engine_create_arch(C.byref(d), 4, rot, C.byref(h)) == -1


@pytest.mark.parametrize("tied", [False, True])
def test_key_map_is_the_hf_state_dict(tied):
    m = _host_model(tie_word_embeddings=tied)
    hf = transformers.GPTNeoXForCausalLM(transformers.GPTNeoXConfig(**_tiny(tie_word_embeddings=tied)))
    want = {"lm." + k: tuple(v.shape) for k, v in hf.state_dict().items() if not (tied and k == "lm_head.weight")}
    assert {k: tuple(v[1]) for k, v in m.key_map.items()} == want
    assert len(m.hf_decay_flags()) == len(m.engine.tensors)
    assert {s.name.split(".")[-2] for s in m.hf_muon_segments()} == {"query_key_value", "dense", "dense_h_to_4h", "dense_4h_to_h"}


def test_qkv_permutation_round_trip():
    g = torch.Generator().manual_seed(0)
    for shape in ((768, 256), (768,)):
        t = torch.randn(*shape, generator=g)
        e = qkv_hf_to_engine(t, 4, 64)
        assert torch.equal(qkv_engine_to_hf(e, 4, 64), t) and not torch.equal(e, t)
        assert torch.equal(e.reshape(3, 4, 64, -1)[1, 2], t.reshape(4, 3, 64, -1)[2, 1])  # k of head 2
