"""CPU checks of the OPT decoder family: config parsing and refusals, the engine's OPT parameter layout (no GPU needed) and
the HF key map."""
import ctypes as C

import pytest

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import KNOWN_BASE_CONFIGS, base_config_from_hf

OPT_125M = dict(model_type="opt", num_hidden_layers=12, hidden_size=768, num_attention_heads=12, ffn_dim=3072,
                max_position_embeddings=2048, do_layer_norm_before=True, word_embed_proj_dim=768, enable_bias=True,
                layer_norm_elementwise_affine=True, activation_function="relu", _remove_final_layer_norm=False,
                init_std=0.02, tie_word_embeddings=True, vocab_size=50272)


def test_opt_config_to_base_config():
    b = base_config_from_hf(OPT_125M)
    assert b["model_type"] == "opt"
    assert (b["num_hidden_layers"], b["hidden_size"], b["num_attention_heads"], b["num_key_value_heads"], b["head_dim"],
            b["intermediate_size"], b["max_position_embeddings"]) == (12, 768, 12, 12, 64, 3072, 2048)
    assert b["layer_norm_eps"] == 1e-5 and b["initializer_range"] == 0.02
    assert base_config_from_hf(b) == b  # idempotent: the engine's own serialised base_config parses back
    assert base_config_from_hf(KNOWN_BASE_CONFIGS["facebook/opt-1.3b"])["intermediate_size"] == 8192


@pytest.mark.parametrize("change,what", [
    (dict(do_layer_norm_before=False), "post-LN"),
    (dict(word_embed_proj_dim=512), "project_in"),
    (dict(activation_function="gelu"), "activation"),
    (dict(tie_word_embeddings=False), "tied"),
    (dict(hidden_size=2560, num_attention_heads=40, word_embed_proj_dim=2560), "2048"),
    (dict(enable_bias=False), "bias"),
    (dict(layer_norm_elementwise_affine=False), "affine"),
    (dict(_remove_final_layer_norm=True), "final_layer_norm"),
])
def test_opt_unsupported_variants_raise(change, what):
    with pytest.raises(ValueError, match=what):
        base_config_from_hf({**OPT_125M, **change})


def test_unknown_family_still_raises():
    with pytest.raises(ValueError, match="Qwen2 and OPT"):
        base_config_from_hf({"model_type": "llama"})


def _opt_engine(L=12, H=768, nH=12, F=3072, V=502, npos=2048):
    return E.Engine(E.SlamModelDesc(L, H, nH, nH, 64, F, V, 0, 1e-5, 10000.0), arch=1, n_positions=npos)


def test_opt_125m_engine_layout():
    eng = _opt_engine()
    L, H, F, V, npos = 12, 768, 3072, 502, 2048
    per_layer = 4 * H * H + 4 * H + 2 * H * F + F + H + 4 * H  # q,k,v,out (+ biases), fc1, fc2 (+ biases), two LayerNorms
    hf = V * H + (npos + 2) * H + L * per_layer + 2 * H
    assert eng.n_params == hf + (512 - V) * H  # + the zero pad rows of the 512-row embedding image
    t = eng.tensors
    names = list(t)
    assert names[:2] == ["embed", "pos_embed"] and names[-2:] == ["norm", "norm_b"]
    assert [n.split(".", 2)[2] for n in names if n.startswith("layers.0.")] == [
        "ln1", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2", "ln2_b", "w1", "b1", "w2", "b2"]
    assert t["pos_embed"].rows == npos + 2 and t["pos_embed"].offset == 512 * H
    assert t["layers.0.ln1"].offset == t["pos_embed"].offset + t["pos_embed"].numel
    assert all(s.offset % 8 == 0 for s in t.values())
    stride = t["layers.1.ln1"].offset - t["layers.0.ln1"].offset
    assert stride == per_layer
    for l in range(1, L):
        for k in ("ln1", "wqkv", "bo", "w1", "b2"):
            assert t[f"layers.{l}.{k}"].offset - t[f"layers.{l - 1}.{k}"].offset == stride
    assert t["norm"].offset == t[f"layers.{L - 1}.ln1"].offset + stride
    assert t["norm_b"].offset + H == eng.n_params
    assert eng.workspace_bytes(4096) > 0
    eng.close()


def test_opt_engine_rejects_bad_descriptions():
    lib = E.load_library()
    h = C.c_void_p()
    gqa = E.SlamModelDesc(2, 256, 4, 2, 64, 512, 502, 0, 1e-5, 10000.0)
    assert lib.slam_engine_create_arch(C.byref(gqa), 1, 128, C.byref(h)) == -1  # OPT needs n_kv_heads == n_heads
    mha = E.SlamModelDesc(2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0)
    assert lib.slam_engine_create_arch(C.byref(mha), 1, 0, C.byref(h)) == -1    # no position table
    assert lib.slam_engine_create_arch(C.byref(mha), 2, 128, C.byref(h)) == -1  # unknown family
    assert lib.slam_engine_create_arch(C.byref(mha), 1, 128, C.byref(h)) == 0
    lib.slam_engine_destroy(h)


def test_opt_qwen2_arch0_matches_slam_engine_create():
    d = E.SlamModelDesc(24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
    a, b = E.Engine(d), E.Engine(d, arch=0)
    assert a.n_params == b.n_params == 358_347_904 + 10 * 896
    assert {k: (v.offset, v.rows, v.cols) for k, v in a.tensors.items()} == {k: (v.offset, v.rows, v.cols) for k, v in b.tensors.items()}


def test_opt_key_map_matches_hf_opt_state_dict():
    """The HF names the key map produces are OPTForCausalLM's (under the reference UnitLM's `lm.` prefix), minus the tied
    lm_head.weight. Built without a GPU: the key map only needs the engine's tensor table."""
    transformers = pytest.importorskip("transformers")
    from slamkit_amd.model.unit_lm import UnitLM, UnitLMConfig
    cfg = transformers.OPTConfig(vocab_size=502, hidden_size=256, num_hidden_layers=2, ffn_dim=512, num_attention_heads=4,
                                 max_position_embeddings=128, word_embed_proj_dim=256, pad_token_id=0)
    hf = transformers.OPTForCausalLM(cfg)
    want = {"lm." + k: tuple(v.shape) for k, v in hf.state_dict().items() if k != "lm_head.weight"}
    ucfg = UnitLMConfig(base_model_name="local-tiny-opt", base_config=cfg.to_dict(), vocab_size=502)
    m = UnitLM.__new__(UnitLM)
    m.config = ucfg
    m.engine = E.Engine(ucfg.engine_desc(), *ucfg.engine_arch())
    m._build_key_map()
    assert {k: tuple(v[1]) for k, v in m.key_map.items()} == want
    m.engine.close()
