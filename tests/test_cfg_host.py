"""CPU tier of classifier-free guidance (slam_cfg_scores / slam_cfg_mirror_tokens, generate(guidance_scale=)): the numpy
restatement (tests/cfg_ref.py) against transformers' own logits processor (tests/golden/cfg_hf.npz, make_golden_cfg.py) and
against its float64 form; the three symbols declared, exported and bound; every refusal comes back before anything reaches the
device (fake pointers, as in test_extend_abi.py); the workspace arithmetic; generate's argument errors on a host-only model."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from slamkit_amd import engine as E
from tests import cfg_ref as R

NEW = ["slam_cfg_workspace_bytes", "slam_cfg_scores", "slam_cfg_mirror_tokens"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg_hf.npz")
E_INVAL = -1
FAKE = 1 << 20  # never dereferenced: every call below must return before a launch


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def cases():
    return R.op_cases()


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_matches_transformers_processor(gold, cases):
    tol = 10 * R.restatement_error(cases)
    for V in (502, 2049):
        logits = np.concatenate([gold[f"op_x_{V}"], gold[f"op_y_{V}"]])
        for g in R.GUIDANCE:
            want = gold[f"op_out_{V}_{g}"].astype(np.float64)
            got = R.cfg_f32(logits, g).astype(np.float64)
            assert np.isfinite(want).all() and np.abs(got - want).max() <= tol, (V, g, np.abs(got - want).max(), tol)


def test_restatement_f32_against_f64(cases):
    err = R.restatement_error(cases)  # asserts that the non-finite entries agree exactly
    assert 0 < err < 1e-4, err  # a few ulp of scores of magnitude 30 .. 60
    names = [c[0] for c in cases]
    for V in (502, 2048, 2049, 152167):
        for g in R.GUIDANCE:
            assert f"v{V}_g{g}" in names


def test_restatement_non_finite_rules(cases):
    by = {c[0]: c for c in cases}
    _, x, g = by["v502_g1.5"]
    out = R.cfg_f32(x, g)
    a = R.cfg_f32(x, 1.0)  # g = 1: d + u = a up to rounding; its -inf pattern is a's
    assert np.isfinite(out[0]).all()
    assert (out[1][np.isinf(R.clean(x[1]))] == -np.inf).all()  # a_i = -inf -> -inf, also where u_i = -inf too
    only_u = np.isinf(R.clean(x[4])) & ~np.isinf(R.clean(x[1]))
    assert only_u.any() and np.isfinite(out[1][only_u]).all()
    assert np.allclose(out[1][only_u], a[1][only_u], atol=1e-5)  # u_i = -inf, a_i finite -> a_i
    _, x, g = by["xdead_g1.5"]
    out = R.cfg_f32(x, g)
    assert (out[0] == -np.inf).all() and (out[2] == -np.inf).all()
    _, x, g = by["ydead_g1.5"]
    out, a = R.cfg_f32(x, g), R.cfg_f32(x, 1.0)
    assert np.array_equal(out[2], a[2]) and np.isfinite(out[0]).all()  # rows 3 and 5 are dead: pairs 0 and 2 give a
    assert np.array_equal(out[0], a[0])
    assert not np.isnan(np.concatenate([R.cfg_f32(c[1], c[2]).ravel() for c in cases if c[1].shape[1] < 3000])).any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    for n in ("cfg_workspace_bytes", "cfg_scores", "cfg_mirror_tokens"):
        assert hasattr(E, n), n


def test_workspace_arithmetic():
    ws = E.load_library().slam_cfg_workspace_bytes
    assert ws(1, 502) == 2 * 1 * 1 * 8          # (m_c, s_c) per chunk of both rows
    assert ws(3, 2048) == 2 * 3 * 1 * 8
    assert ws(3, 2049) == 2 * 3 * 2 * 8
    assert ws(8, 152576) == 2 * 8 * 75 * 8
    assert ws(32767, 502) == 2 * 32767 * 8
    for B, V in ((0, 502), (-1, 502), (32768, 502), (3, 0), (3, -5)):
        assert ws(B, V) == 0, (B, V)
    assert E.cfg_workspace_bytes(3, 2049) == ws(3, 2049)


def test_cfg_scores_refused_before_a_launch():
    lib = E.load_library()
    B, V = 3, 2049
    nb = lib.slam_cfg_workspace_bytes(B, V)
    far = FAKE + 2 * B * V * 4 + 64  # behind the logits

    def call(logits=FAKE, B=B, V=V, g=1.5, scores=far, ws=FAKE * 64, nb=nb):
        return lib.slam_cfg_scores(logits, B, V, g, scores, ws, nb, None)

    for kw in (dict(logits=None), dict(scores=None), dict(ws=None), dict(B=0), dict(B=-1), dict(B=32768), dict(V=0), dict(V=-3),
               dict(g=math.nan), dict(g=math.inf), dict(g=-math.inf), dict(logits=FAKE + 2), dict(scores=far + 1),
               dict(ws=FAKE * 64 + 4), dict(nb=nb - 1), dict(nb=0),
               dict(scores=FAKE),                      # the same start
               dict(scores=FAKE + 2 * B * V * 4 - 4),  # the last logit
               dict(scores=FAKE - B * V * 4 + 4),      # the last score on the first logit
               dict(scores=FAKE + B * V * 4)):         # the unconditional rows
        assert call(**kw) == E_INVAL, kw
    assert lib.slam_cfg_scores(FAKE, 32768, 1, 1.5, FAKE * 2, FAKE * 64, 1 << 30, None) == E_INVAL  # 2 B above 65535


def test_cfg_mirror_refused_before_a_launch():
    lib = E.load_library()
    for nxt, B in ((None, 4), (FAKE, 0), (FAKE, -1), (FAKE, 32768), (FAKE + 4, 4)):
        assert lib.slam_cfg_mirror_tokens(nxt, B, None) == E_INVAL, (nxt, B)


# ---- generate's argument errors ------------------------------------------------------------------------------------------------
def _host_model(vocab=502, max_tokens=64):
    import torch
    from slamkit_amd.model.unit_lm import UnitLM, UnitLMConfig
    base = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=2, num_key_value_heads=2, head_dim=32,
                intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    m = UnitLM.__new__(UnitLM)  # host-only: every check below happens before the model is touched
    m.config = UnitLMConfig(base_model_name="local", base_config=base, vocab_size=vocab, max_tokens=max_tokens)
    m.device = torch.device("cpu")
    return m


def test_generate_guidance_argument_errors():
    import torch
    m = _host_model()
    ids = torch.ones(2, 4, dtype=torch.long)
    neg = torch.full((2, 6), 3, dtype=torch.long)
    kw = dict(input_ids=ids, max_new_tokens=4)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="guidance_scale"):
            m.generate(guidance_scale=bad, **kw)
    # dangling arguments: guidance off
    for g in (None, 1.0, 1):
        with pytest.raises(ValueError, match="negative_prompt"):
            m.generate(guidance_scale=g, negative_prompt_ids=neg, **kw)
        with pytest.raises(ValueError, match="negative_prompt"):
            m.generate(guidance_scale=g, negative_prompt_attention_mask=torch.ones_like(neg), **kw)
    with pytest.raises(ValueError, match="negative_prompt_ids"):
        m.generate(guidance_scale=2.0, negative_prompt_attention_mask=torch.ones_like(neg), **kw)
    with pytest.raises(ValueError, match=r"negative_prompt_ids must be \[2, T_neg\]"):
        m.generate(guidance_scale=2.0, negative_prompt_ids=neg[:1], **kw)
    with pytest.raises(ValueError, match="negative_prompt_ids must be"):
        m.generate(guidance_scale=2.0, negative_prompt_ids=neg[0], **kw)
    am = torch.ones_like(neg)
    am[1] = 0
    with pytest.raises(ValueError, match="negative prompt row"):
        m.generate(guidance_scale=2.0, negative_prompt_ids=neg, negative_prompt_attention_mask=am, **kw)
    # the longer of the two prompts counts against max_tokens (64): 4 + 4 fits, 61 + 4 does not
    with pytest.raises(ValueError, match="max_tokens"):
        m.generate(guidance_scale=2.0, negative_prompt_ids=torch.full((2, 61), 3, dtype=torch.long), **kw)
    with pytest.raises(ValueError, match="assistant_model or prompt_lookup_num_tokens"):
        m.generate(guidance_scale=2.0, assistant_model=_host_model(), **kw)
    with pytest.raises(ValueError, match="assistant_model or prompt_lookup_num_tokens"):
        m.generate(guidance_scale=2.0, prompt_lookup_num_tokens=3, **kw)

    class GC:
        guidance_scale = math.nan
    with pytest.raises(ValueError, match="guidance_scale"):  # also read from generation_config
        m.generate(generation_config=GC(), **kw)
    # the long-standing refusals stay
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(guidance_scale=2.0, num_beams=2, **kw)
    with pytest.raises(ValueError, match="repetition_penalty"):
        m.generate(guidance_scale=2.0, repetition_penalty=1.2, **kw)


def test_golden_file_keeps_its_cap(gold):
    """What make_golden_cfg.py asserted when it wrote the file: by HF's margins alone, at least 60 % of the steps of every case
    lie before their row's first near-tie."""
    assert json.loads(str(gold["bad_words"])) and int(gold["no_repeat_ngram_size"]) == 2
    for tag in ("tiny", "wide"):
        for case in ("g15", "g30neg", "g05neg", "g05bans"):
            k = f"{tag}_{case}"
            g, margin = float(gold[f"{k}_g"]), gold[f"{k}_margin"]
            tol = (abs(g) + abs(1 - g)) * 2 * 2e-2 * float(gold[f"{k}_rms"])
            n = sum(int(np.argmax(row < tol)) if (row < tol).any() else len(row) for row in margin)
            assert n >= 0.6 * margin.size, (k, n, margin.size)
