"""CPU checks of the Qwen3 decoder family (arch 3): the plain-torch restatement against the HF golden, config parsing and
refusals, the engine's parameter layout and workspace (host code: no GPU needed), the HF key map, the decay flags and the
argument checks of the new op entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from slamkit_amd.model.unit_lm import ARCH_QWEN3, KNOWN_BASE_CONFIGS, UnitLM, UnitLMConfig, base_config_from_hf
from tests import qwen3_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen3.npz")

QWEN3_06B = dict(model_type="qwen3", num_hidden_layers=28, hidden_size=1024, num_attention_heads=16, num_key_value_heads=8,
                 head_dim=128, intermediate_size=3072, rms_norm_eps=1e-6, hidden_act="silu", attention_bias=False,
                 use_sliding_window=False, sliding_window=None, max_window_layers=28, layer_types=["full_attention"] * 28,
                 rope_parameters={"rope_type": "default", "rope_theta": 1000000.0}, tie_word_embeddings=True,
                 initializer_range=0.02, vocab_size=151936, max_position_embeddings=40960)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("tag", ["A", "B"])
def test_ref_forward_matches_hf_golden(tag, gold):
    cfg = R.CFGS[tag]
    sd = R.weights(cfg, int(gold[f"{tag}_seed"]))
    ids, mask, labels, lens = R.batch()
    logits = R.forward(cfg, sd, ids, attention_mask=mask)
    got = torch.cat([logits[b, :n] for b, n in enumerate(lens)]).double()
    want = torch.from_numpy(gold[f"{tag}_logits"]).double()
    rel = float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
    assert rel <= 1e-4, (tag, rel)
    assert abs(float(R.loss_of(logits, labels)) - float(gold[f"{tag}_loss"])) <= 1e-4


@pytest.mark.parametrize("tag", ["A", "B"])
def test_ref_gradients_match_hf_golden(tag, gold):
    cfg = R.CFGS[tag]
    sd = R.weights(cfg, int(gold[f"{tag}_seed"]))
    ids, mask, labels, _ = R.batch()
    _, _, grads = R.loss_and_grads(cfg, sd, ids, mask, labels)
    names = [k for k, _ in R.hf_keys(cfg)]
    norms = np.array([float(grads[k].double().norm()) for k in names])
    assert np.allclose(norms, gold[f"{tag}_grad_norms"], rtol=1e-3, atol=1e-7), (norms, gold[f"{tag}_grad_norms"])
    for short, key in (("input_layernorm", "input_layernorm"), ("post_attention_layernorm", "post_attention_layernorm"),
                       ("q_norm", "self_attn.q_norm"), ("k_norm", "self_attn.k_norm")):
        g, w = grads[f"lm.model.layers.0.{key}.weight"], torch.from_numpy(gold[f"{tag}_grad_{short}"])
        assert float((g - w).norm()) <= 1e-3 * float(w.norm()), (tag, short)


def test_kernel_contracts_agree_with_autograd():
    """The fp64 backward contract is the derivative of the forward contract (norm only: RoPE and the scale are undone by
    attn_bwd before the kernel runs)."""
    nH, nKV, hd, M = 3, 1, 64, 7
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, (nH + nKV) * hd, generator=g, dtype=torch.float64, requires_grad=True)
    wq = (1 + 0.1 * torch.randn(hd, generator=g, dtype=torch.float64)).requires_grad_(True)
    wk = (1 + 0.1 * torch.randn(hd, generator=g, dtype=torch.float64)).requires_grad_(True)
    dy = torch.randn(M, (nH + nKV) * hd, generator=g, dtype=torch.float64)
    w = torch.cat([wq[None].expand(nH, hd), wk[None].expand(nKV, hd)])[None]
    y, _ = R.head_norm(x.view(M, nH + nKV, hd), w, 1e-6)
    y.reshape(M, -1).backward(dy)
    dx, dwq, dwk = R.qknorm_bwd_ref(dy, x.detach(), wq.detach(), wk.detach(), nH, nKV, hd, 1e-6)
    assert torch.allclose(dx, x.grad, atol=1e-12) and torch.allclose(dwq, wq.grad, atol=1e-12) and torch.allclose(dwk, wk.grad, atol=1e-12)


# ---- configuration ------------------------------------------------------------------------------------------------------------
def test_qwen3_config_to_base_config():
    b = base_config_from_hf(QWEN3_06B)
    assert b["model_type"] == "qwen3"
    assert (b["num_hidden_layers"], b["hidden_size"], b["num_attention_heads"], b["num_key_value_heads"], b["head_dim"],
            b["intermediate_size"]) == (28, 1024, 16, 8, 128, 3072)
    assert b["rope_theta"] == 1000000.0 and b["rms_norm_eps"] == 1e-6 and b["tie_word_embeddings"] is True
    assert base_config_from_hf(b) == b  # idempotent: the engine's own serialised base_config parses back
    no_hd = {k: v for k, v in QWEN3_06B.items() if k != "head_dim"}
    assert base_config_from_hf(no_hd)["head_dim"] == 1024 // 16  # absent: hidden_size // num_attention_heads
    old = dict(no_hd, rope_theta=5e5)  # transformers 4.x keeps rope_theta at the top level
    del old["rope_parameters"]
    assert base_config_from_hf(old)["rope_theta"] == 5e5


@pytest.mark.parametrize("change,what", [
    (dict(attention_bias=True), "attention_bias"),
    (dict(use_sliding_window=True), "sliding"),
    (dict(layer_types=["full_attention"] * 27 + ["sliding_attention"]), "layer_types"),
    (dict(rope_parameters={"rope_type": "yarn", "rope_theta": 1e6, "factor": 4.0}), "rope"),
    (dict(rope_parameters=None, rope_scaling={"type": "linear", "factor": 2.0}), "rope"),
    (dict(hidden_act="gelu"), "hidden_act"),
])
def test_qwen3_unsupported_variants_raise(change, what):
    with pytest.raises(ValueError, match=what):
        base_config_from_hf({**QWEN3_06B, **change})


@pytest.mark.parametrize("mt", ["llama", "qwen3_moe"])
def test_other_families_still_raise(mt):
    with pytest.raises(ValueError, match="Qwen2 and OPT"):
        base_config_from_hf({"model_type": mt})
    with pytest.raises(ValueError, match="Qwen3"):
        base_config_from_hf({"model_type": mt})


def test_known_configs_and_unit_lm_config():
    for name, H, I in (("Qwen/Qwen3-0.6B", 1024, 3072), ("Qwen/Qwen3-1.7B", 2048, 6144)):
        k = KNOWN_BASE_CONFIGS[name]
        assert (k["model_type"], k["num_hidden_layers"], k["hidden_size"], k["num_attention_heads"], k["num_key_value_heads"],
                k["head_dim"], k["intermediate_size"], k["rms_norm_eps"], k["rope_theta"], k["tie_word_embeddings"]) == (
                    "qwen3", 28, H, 16, 8, 128, I, 1e-6, 1e6, True)
    c = UnitLMConfig(base_model_name="Qwen/Qwen3-0.6B", rope_theta=10000)
    assert c.is_qwen3 and not c.is_opt and c.engine_arch() == (ARCH_QWEN3, 0) == (3, 0) and c.engine_flags() == 0
    assert c.base_config["model_type"] == "qwen3" and c.base_config["rope_theta"] == 10000
    d = c.engine_desc()
    assert (d.n_layers, d.hidden, d.n_heads, d.n_kv_heads, d.head_dim, d.intermediate, d.vocab) == (28, 1024, 16, 8, 128, 3072, 502)
    # the serialised config parses back to the same model (save_pretrained / from_pretrained)
    c2 = UnitLMConfig(base_model_name="local", base_config=c.to_dict()["base_config"])
    assert c2.base_config == c.base_config and c2.engine_arch() == (3, 0)
    u = UnitLMConfig(base_model_name="local", base_config=dict(R.CFG_A), tie_word_embeddings=False)
    assert u.engine_arch() == (3, 0) and u.engine_flags() == E.MODEL_UNTIED_HEAD
    with pytest.raises(ValueError, match="dropout"):
        UnitLMConfig(base_model_name="local", base_config=dict(R.CFG_A), dropout=0.1)


def test_model_yaml_loads():
    from slamkit_amd.utils.config import load_config, to_container
    cfg = to_container(load_config("train", ["model=slam_qwen3"]))
    args = cfg["model"]["config_args"]
    assert args["base_model_name"] == "Qwen/Qwen3-0.6B" and cfg["model"]["context_len"] == 1024
    assert UnitLMConfig(**args).engine_arch() == (3, 0)


# ---- engine layout ------------------------------------------------------------------------------------------------------------
def _desc(L, H, nH, nKV, hd, I, V=502, eps=1e-6, theta=1e6):
    return E.SlamModelDesc(L, H, nH, nKV, hd, I, V, 0, eps, theta)


def test_qwen3_06b_engine_layout():
    L, H, nH, nKV, hd, I, V = 28, 1024, 16, 8, 128, 3072, 502
    eng = E.Engine(_desc(L, H, nH, nKV, hd, I, V), arch=3)
    QKV = (nH + 2 * nKV) * hd
    per_layer = H + QKV * H + hd + hd + H * nH * hd + H + 2 * I * H + H * I
    assert eng.n_params == 512 * H + L * per_layer + H  # the embedding image has 512 rows (10 zero pad rows)
    t = eng.tensors
    names = list(t)
    assert names[0] == "embed" and names[-1] == "norm"
    for l in (0, L - 1):
        assert [n.split(".", 2)[2] for n in names if n.startswith(f"layers.{l}.")] == [
            "ln1", "wqkv", "q_norm", "k_norm", "wo", "ln2", "wgu", "wd"]
    assert not any("bqkv" in n for n in names)
    for l in range(L):
        for k in ("q_norm", "k_norm"):
            assert (t[f"layers.{l}.{k}"].rows, t[f"layers.{l}.{k}"].cols) == (hd, 1)
    assert (t["layers.0.wqkv"].rows, t["layers.0.wqkv"].cols) == (QKV, H)
    assert (t["layers.0.wo"].rows, t["layers.0.wo"].cols) == (H, nH * hd)  # n_heads * head_dim = 2048 != hidden
    assert t["layers.0.q_norm"].offset == t["layers.0.wqkv"].offset + QKV * H
    assert t["layers.0.k_norm"].offset == t["layers.0.q_norm"].offset + hd
    assert t["layers.0.wo"].offset == t["layers.0.k_norm"].offset + hd
    assert all(s.offset % 8 == 0 for s in t.values())
    assert t["layers.1.ln1"].offset - t["layers.0.ln1"].offset == per_layer
    assert t["norm"].offset + H == eng.n_params
    eng.close()


def test_untied_accepted_and_other_archs_as_before():
    lib = E.load_library()
    d = _desc(2, 256, 4, 2, 128, 512)
    tied, untied = E.Engine(d, arch=3), E.Engine(d, arch=3, flags=E.MODEL_UNTIED_HEAD)
    assert list(untied.tensors)[-2:] == ["norm", "lm_head"] and untied.n_params == tied.n_params + 512 * 256
    assert [(k, v.offset) for k, v in tied.tensors.items()] == [(k, v.offset) for k, v in untied.tensors.items()][:-1]
    tied.close()
    untied.close()
    h = C.c_void_p()
    assert lib.slam_engine_create_arch(C.byref(d), 2, 0, C.byref(h)) == -1        # arch 2 stays refused
    assert lib.slam_engine_create_ex(C.byref(d), 3, 0, 2, C.byref(h)) == -1       # no new flag bit
    assert lib.slam_engine_create_ex(C.byref(d), 3, 0, 3, C.byref(h)) == -1
    mha = E.SlamModelDesc(2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0)
    assert lib.slam_engine_create_ex(C.byref(mha), 1, 128, 1, C.byref(h)) == -1   # untied OPT stays refused
    for bad in (_desc(2, 256, 4, 2, 96, 512), _desc(2, 260, 4, 2, 128, 512), _desc(2, 4104, 4, 2, 128, 512),
                _desc(2, 256, 4, 2, 128, 500), _desc(2, 256, 4, 3, 128, 512), _desc(2, 256, 16, 1, 64, 512)):
        assert lib.slam_engine_create_arch(C.byref(bad), 3, 0, C.byref(h)) == -1
    assert lib.slam_engine_create_arch(C.byref(d), 3, 12345, C.byref(h)) == 0     # n_positions is ignored
    lib.slam_engine_destroy(h)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_workspace_grows_by_exactly_the_two_buffers(level):
    L, H, nH, nKV, hd, I, M = 5, 256, 4, 2, 128, 512, 1024
    d = _desc(L, H, nH, nKV, hd, I)
    q2, q3 = E.Engine(d, arch=0), E.Engine(d, arch=3)
    for e in (q2, q3):
        e.set_option("recompute", level)
    raw, rstd = M * (nH + nKV) * hd * 2, M * (nH + nKV) * 4  # both multiples of 256: no alignment padding
    assert raw % 256 == 0 and rstd % 256 == 0
    copies = min(L, 3) if level == 2 else L  # kept per layer wherever qkv is: levels 0 and 1
    assert q3.workspace_bytes(M) - q2.workspace_bytes(M) == copies * (raw + rstd)
    q2.close()
    q3.close()


def test_arch0_workspace_is_unchanged():
    # the figures tests/test_recompute_host.py pins for the parent commit's build
    eng = E.Engine(E.SlamModelDesc(24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0))
    assert eng.workspace_bytes(8192) == 8383851008
    eng.close()


# ---- key map and decay flags --------------------------------------------------------------------------------------------------
def _host_model(cfg_dict, **kw):
    ucfg = UnitLMConfig(base_model_name="local", base_config=dict(cfg_dict), vocab_size=R.VOCAB, **kw)
    m = UnitLM.__new__(UnitLM)
    m.config = ucfg
    m.engine = E.Engine(ucfg.engine_desc(), *ucfg.engine_arch(), flags=ucfg.engine_flags())
    m._build_key_map()
    return m


def test_key_map_is_the_hf_qwen3_state_dict():
    m = _host_model(R.CFG_A)
    want = {k: shp for k, shp in R.hf_keys(R.CFG_A)}
    assert {k: tuple(v[1]) for k, v in m.key_map.items()} == want
    assert not any(k.endswith(".bias") for k in m.key_map)
    # every element of the flat buffer outside the embedding's pad rows belongs to exactly one HF tensor
    covered = sum(int(np.prod(v[1])) for v in m.key_map.values())
    assert covered == m.engine.n_params - (512 - R.VOCAB) * 256
    m.engine.close()
    u = _host_model(R.CFG_A, tie_word_embeddings=False)
    assert u.key_map["lm.lm_head.weight"] == (u.engine.tensors["lm_head"].offset, (R.VOCAB, 256))
    u.engine.close()


def test_ref_key_list_is_hf_qwen3s_own():
    """qwen3_ref.hf_keys - what the key map is held to above - against transformers' Qwen3ForCausalLM state dict."""
    transformers = pytest.importorskip("transformers")
    c = transformers.Qwen3Config(vocab_size=R.VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                 num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=True)
    hf = transformers.Qwen3ForCausalLM(c)
    want = {k: shp for k, shp in R.hf_keys(R.CFG_A)}
    assert {"lm." + k: tuple(v.shape) for k, v in hf.state_dict().items() if k != "lm_head.weight"} == want
    assert base_config_from_hf(c.to_dict())["head_dim"] == 128


def test_decay_flags():
    m = _host_model(R.CFG_A)
    flags = dict(zip(m.engine.tensors, m.hf_decay_flags()))
    no_decay = {n for n, f in flags.items() if not f}
    assert no_decay == {f"layers.{l}.{k}" for l in range(2) for k in ("ln1", "ln2", "q_norm", "k_norm")} | {"norm"}
    m.engine.close()


# ---- op entry points: refused before any launch --------------------------------------------------------------------------------
def test_op_entry_points_refuse_bad_arguments():
    lib = E.load_library()
    p = C.c_void_p(4096)  # never dereferenced: every call below is refused on the host
    ok = dict(M=8, T=8, nH=4, nKV=2, hd=128)

    def fwd(qkv=p, wq=p, wk=p, tab=p, **kw):
        a = {**ok, **kw}
        return lib.slam_op_qknorm_rope_fwd(qkv, wq, wk, None, 1e4, 1e-6, a["M"], a["T"], a["nH"], a["nKV"], a["hd"], None, None, tab, None)

    def bwd(dqkv=p, raw=p, rstd=p, wq=p, wk=p, dwq=p, dwk=p, ws=p, **kw):
        a = {**ok, **kw}
        return lib.slam_op_qknorm_bwd(dqkv, raw, rstd, wq, wk, dwq, dwk, ws, a["M"], a["nH"], a["nKV"], a["hd"], None)

    def rows(qkv=p, wq=p, wk=p, **kw):
        a = {**ok, **kw}
        return lib.slam_op_qknorm_rows_f32(qkv, wq, wk, 1e-6, a["M"], a["nH"], a["nKV"], a["hd"], None)

    for f, ptrs in ((fwd, ("qkv", "wq", "wk", "tab")), (bwd, ("dqkv", "raw", "rstd", "wq", "wk", "dwq", "dwk", "ws")),
                    (rows, ("qkv", "wq", "wk"))):
        for name in ptrs:
            assert f(**{name: None}) == -1, (f.__name__, name)
        for bad in (dict(hd=96), dict(hd=32), dict(M=0), dict(M=-5), dict(nH=0), dict(nKV=0)):
            assert f(**bad) == -1, (f.__name__, bad)
    big = dict(M=1 << 24, nH=16, nKV=8, hd=128)  # 2^24 x 24 heads x 16 lanes >= 2^31: past the kernels' 32-bit head index
    assert fwd(**big) == -1 and bwd(**big) == -1 and rows(**big) == -1
    assert lib.slam_op_qknorm_bwd_workspace(0, 4, 2, 128) == 0 and lib.slam_op_qknorm_bwd_workspace(8, 4, 2, 96) == 0
    assert lib.slam_op_qknorm_bwd_workspace(8, 4, 2, 128) > 0
