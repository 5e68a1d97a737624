"""CPU checks of the wide (hidden <= 4096), untied-head Qwen2 bodies: slam_engine_create_ex, the layout of the `lm_head` tensor,
refusals, and the config surface (no GPU needed: the engine's tensor table is host code)."""
import ctypes as C

import pytest

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS, UnitLMConfig

QWEN7B = (28, 3584, 28, 4, 128, 18944)
SLAM = (24, 896, 14, 2, 64, 4864)


def _desc(dims, V, eps=1e-6, theta=1e6):
    return E.SlamModelDesc(*dims, V, 0, eps, theta)


def _table(eng):
    return [(k, v.offset, v.rows, v.cols) for k, v in eng.tensors.items()]


def test_create_ex_qwen7b_untied_layout():
    lib = E.load_library()
    assert hasattr(lib, "slam_engine_create_ex")
    eng = E.Engine(_desc(QWEN7B, 152064), flags=E.MODEL_UNTIED_HEAD)
    assert eng.n_params == 7_615_616_512  # HF's count for Qwen2.5-7B: vpad == vocab, no pad rows
    names = list(eng.tensors)
    assert names[0] == "embed" and names[-2:] == ["norm", "lm_head"]
    head = eng.tensors["lm_head"]
    assert (head.rows, head.cols) == (152064, 3584)
    assert head.offset == eng.tensors["norm"].offset + 3584 and head.offset + head.numel == eng.n_params
    assert all(s.offset % 8 == 0 for s in eng.tensors.values())
    assert eng.workspace_bytes(4096) > 0
    eng.close()


def test_flags_zero_is_the_tied_layout_and_untied_appends_lm_head():
    d = _desc(SLAM, 502, theta=10000.0)
    lib = E.load_library()
    h = C.c_void_p()
    assert lib.slam_engine_create(C.byref(d), C.byref(h)) == 0
    info, plain = E.SlamTensorInfo(), []
    for i in range(lib.slam_tensor_count(h)):
        assert lib.slam_tensor_info(h, i, C.byref(info)) == 0
        plain.append((info.name.decode(), info.offset, info.rows, info.cols))
    n_plain = lib.slam_param_count(h)
    lib.slam_engine_destroy(h)
    tied, untied = E.Engine(d, flags=0), E.Engine(d, flags=E.MODEL_UNTIED_HEAD)
    assert _table(tied) == plain and tied.n_params == n_plain
    assert _table(untied) == plain + [("lm_head", n_plain, 512, 896)]
    assert untied.n_params == n_plain + 512 * 896
    tied.close()
    untied.close()


def test_create_ex_refusals():
    lib = E.load_library()
    h = C.c_void_p()
    ok = _desc((2, 4096, 32, 8, 128, 11008), 502)
    assert lib.slam_engine_create_ex(C.byref(ok), 0, 0, 0, C.byref(h)) == 0  # the upper limit itself is accepted
    lib.slam_engine_destroy(h)
    wide = _desc((2, 4104, 32, 8, 128, 11008), 502)
    assert lib.slam_engine_create_ex(C.byref(wide), 0, 0, 0, C.byref(h)) == -1             # hidden = 4104
    assert lib.slam_engine_create_ex(C.byref(wide), 0, 0, E.MODEL_UNTIED_HEAD, C.byref(h)) == -1
    small = _desc((2, 256, 4, 4, 64, 512), 502, eps=1e-5)
    assert lib.slam_engine_create_ex(C.byref(small), 0, 0, 2, C.byref(h)) == -1             # unknown flag bit
    assert lib.slam_engine_create_ex(C.byref(small), 0, 0, 3, C.byref(h)) == -1
    assert lib.slam_engine_create_ex(C.byref(small), 1, 128, E.MODEL_UNTIED_HEAD, C.byref(h)) == -1  # untied OPT
    assert lib.slam_engine_create_ex(C.byref(small), 1, 128, 0, C.byref(h)) == 0
    lib.slam_engine_destroy(h)
    opt_wide = _desc((2, 2560, 40, 40, 64, 512), 502, eps=1e-5)
    assert lib.slam_engine_create_ex(C.byref(opt_wide), 1, 128, 0, C.byref(h)) == -1        # OPT keeps its 2048 limit


def test_config_accepts_untied_qwen2_and_refuses_untied_opt():
    base = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
                intermediate_size=256)
    c = UnitLMConfig(base_model_name="local", base_config=base, tie_word_embeddings=False)
    assert c.tie_word_embeddings is False and c.to_dict()["tie_word_embeddings"] is False
    assert c.base_config["tie_word_embeddings"] is False and c.engine_flags() == E.MODEL_UNTIED_HEAD
    c = UnitLMConfig(base_model_name="local", base_config={**base, "tie_word_embeddings": False})
    assert c.tie_word_embeddings is False
    c = UnitLMConfig(base_model_name="local", base_config=base)
    assert c.tie_word_embeddings is True and c.engine_flags() == 0 and c.to_dict()["tie_word_embeddings"] is True
    with pytest.raises(ValueError, match="tied"):
        UnitLMConfig(base_model_name="facebook/opt-125m", tie_word_embeddings=False)


def test_known_qwen25_3b_and_7b_descriptions():
    b3, b7 = KNOWN_BASE_CONFIGS["Qwen/Qwen2.5-3B"], KNOWN_BASE_CONFIGS["Qwen/Qwen2.5-7B"]
    assert (b3["num_hidden_layers"], b3["hidden_size"], b3["num_attention_heads"], b3["num_key_value_heads"], b3["head_dim"],
            b3["intermediate_size"], b3["tie_word_embeddings"]) == (36, 2048, 16, 2, 128, 11008, True)
    c7 = UnitLMConfig(base_model_name="Qwen/Qwen2.5-7B", vocab_size=152064)
    d = c7.engine_desc()
    assert (d.n_layers, d.hidden, d.n_heads, d.n_kv_heads, d.head_dim, d.intermediate, d.vocab) == QWEN7B + (152064,)
    assert abs(d.rms_eps - 1e-6) < 1e-12 and d.rope_theta == 1e6
    assert c7.tie_word_embeddings is False and c7.engine_arch() == (0, 0)
    eng = E.Engine(d, *c7.engine_arch(), flags=c7.engine_flags())
    assert eng.n_params == 7_615_616_512 and list(eng.tensors)[-1] == "lm_head"
    eng.close()
    c3 = UnitLMConfig(base_model_name="Qwen/Qwen2.5-3B", vocab_size=151936)
    eng = E.Engine(c3.engine_desc(), *c3.engine_arch(), flags=c3.engine_flags())
    # HF's count for Qwen2.5-3B plus the zero pad rows of the embedding (151,936 -> 152,064 rows)
    assert "lm_head" not in eng.tensors and eng.n_params == 3_085_938_688 + 128 * 2048
    eng.close()


def test_key_map_matches_hf_untied_qwen2_state_dict():
    """The key map of an untied model is Qwen2ForCausalLM's state dict, lm_head.weight included, under the `lm.` prefix."""
    import transformers
    from slamkit_amd.model.unit_lm import UnitLM
    cfg = transformers.Qwen2Config(vocab_size=502, hidden_size=128, num_hidden_layers=2, intermediate_size=256,
                                   num_attention_heads=2, num_key_value_heads=1, tie_word_embeddings=False, pad_token_id=0)
    hf = transformers.Qwen2ForCausalLM(cfg)
    want = {"lm." + k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert "lm.lm_head.weight" in want
    ucfg = UnitLMConfig(base_model_name="local-tiny", base_config=cfg.to_dict(), vocab_size=502)
    assert ucfg.tie_word_embeddings is False
    m = UnitLM.__new__(UnitLM)
    m.config = ucfg
    m.engine = E.Engine(ucfg.engine_desc(), *ucfg.engine_arch(), flags=ucfg.engine_flags())
    m._build_key_map()
    assert {k: tuple(v[1]) for k, v in m.key_map.items()} == want
    m.engine.close()
