"""CPU tier of assisted generation (draft-model speculative decoding): the four new symbols are declared, exported and bound;
slam_kv_rewind, slam_spec_accept, slam_sample_tokens_at and slam_extend_logits refuse bad arguments before anything reaches the
device (fake pointers, as in test_extend_abi.py); tests/spec_ref.py against hand-worked rows; the ValueErrors of
generate(assistant_model=) on model objects that never touch a GPU."""
import ctypes as C

import numpy as np
import pytest

from slamkit_amd import engine as E
from tests import spec_ref as S

NEW = ["slam_extend_logits", "slam_kv_rewind", "slam_sample_tokens_at", "slam_spec_accept"]
SLAM = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
OPT = (2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0)
E_INVAL, E_STATE, E_NOMEM = -1, -2, -3
FAKE = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    for n in ("extend_logits", "kv_rewind"):
        assert hasattr(E.Engine, n)
    assert callable(E.spec_accept) and callable(E.sample_tokens_at)


def test_kv_rewind_and_extend_logits_refused_before_a_launch():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    h = eng.h

    def ext(hh=h, ids=FAKE, new_lens=FAKE, lens=FAKE, B=2, T=5, logits=FAKE):
        return lib.slam_extend_logits(hh, ids, new_lens, lens, B, T, logits, None)

    assert lib.slam_kv_rewind(None, 4) == E_INVAL
    assert lib.slam_kv_rewind(h, 4) == E_STATE  # no cache
    assert b"cache" in lib.slam_last_error(h)
    for kw in (dict(hh=None), dict(ids=None), dict(new_lens=None), dict(lens=None), dict(logits=None), dict(B=0), dict(T=0)):
        assert ext(**kw) == E_INVAL, kw
    assert ext() == E_STATE  # nothing bound
    assert lib.slam_bind_params(h, FAKE, None) == 0
    assert lib.slam_bind_workspace(h, FAKE, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert ext() == E_STATE and b"cache" in lib.slam_last_error(h)
    assert lib.slam_bind_kv_cache(h, FAKE, lib.slam_kv_cache_bytes(h, 200, 64), 200, 64) == 0
    assert ext(B=2, T=129) == E_NOMEM
    assert ext(B=129, T=1) == E_NOMEM
    assert ext(B=2, T=65) == E_STATE and b"capacity" in lib.slam_last_error(h)
    assert ext() == E_STATE and b"prefill" in lib.slam_last_error(h)
    assert lib.slam_kv_rewind(h, 4) == E_STATE and b"prefill" in lib.slam_last_error(h)  # a cache, but nothing in it
    eng.close()
    opt = E.Engine(E.SlamModelDesc(*OPT), 1, 128)
    assert lib.slam_bind_params(opt.h, FAKE, None) == 0
    assert lib.slam_bind_workspace(opt.h, FAKE, lib.slam_workspace_bytes(opt.h, 256), 256) == 0
    assert lib.slam_extend_logits(opt.h, FAKE, FAKE, FAKE, 2, 5, FAKE, None) == E_INVAL
    assert b"Qwen2" in lib.slam_last_error(opt.h)
    opt.close()


def _accept(**kw):
    a = dict(chunk=FAKE, tgt=FAKE, B=3, K=4, max_new=16, pad_id=0, eos_ids=FAKE, n_eos=1, prompt_len=FAKE, n_new=FAKE, done=FAKE,
             out=FAKE, out_stride=16, lens_t=FAKE, lens_d=FAKE, draft_ids=FAKE, draft_new_lens=FAKE, tgt_new_lens=FAKE, stats=FAKE)
    a.update(kw)
    return E.load_library().slam_spec_accept(*a.values(), None)


def test_spec_accept_refused_before_a_launch():
    for name in ("chunk", "tgt", "eos_ids", "prompt_len", "n_new", "done", "out", "lens_t", "lens_d", "draft_ids", "draft_new_lens",
                 "tgt_new_lens", "stats"):
        assert _accept(**{name: None}) == E_INVAL, name
    for kw in (dict(K=0), dict(K=16), dict(K=-1), dict(B=0), dict(B=1025), dict(B=-3), dict(n_eos=17), dict(n_eos=-1),
               dict(max_new=0), dict(out_stride=15)):
        assert _accept(**kw) == E_INVAL, kw


def test_sample_tokens_at_refused_before_a_launch():
    lib = E.load_library()
    desc = E.SlamSampleDesc(do_sample=1, top_k=25, temperature=0.8, top_p=1.0, seed=1, step=0, pad_id=0, n_eos=0)
    nb = lib.slam_sample_workspace_bytes(10, 502, 25)

    def call(logits=FAKE, B=10, vocab=502, nxt=FAKE, ws=FAKE, ws_bytes=nb, steps=FAKE, group=5, out_col=0, d=desc):
        return lib.slam_sample_tokens_at(logits, B, vocab, None, C.byref(d) if d is not None else None, None, None, None, nxt,
                                         None, 0, ws, ws_bytes, steps, group, out_col, None)

    for kw in (dict(logits=None), dict(nxt=None), dict(ws=None), dict(d=None), dict(B=0), dict(vocab=0), dict(group=0),
               dict(group=-1), dict(group=3), dict(out_col=-1), dict(ws_bytes=nb - 8), dict(steps=C.c_void_p((1 << 20) + 2))):
        assert call(**kw) == E_INVAL, kw


# ---- spec_ref against hand-worked rows -----------------------------------------------------------------------------------------
K, MAXN, PAD, EOS = 3, 10, 0, [9]


def _one(chunk, tgt, n_new=2, done=0, plen=5, eos=EOS, max_new=MAXN):
    out = np.full((1, max_new), -1, np.int64)
    return S.accept([chunk], [tgt], [n_new], [done], [plen], out, K, max_new, PAD, eos)


def test_ref_no_acceptance():
    r = _one([7, 11, 12, 13], [21, 22, 23, 24])
    assert r["out"][0].tolist() == [-1, -1, 21] + [-1] * 7
    assert r["n_new"][0] == 3 and r["done"][0] == 0
    assert r["lens_t"][0] == 5 + 3 - 1 and r["lens_d"][0] == 7
    assert r["chunk"][0].tolist() == [21, 11, 12, 13]
    assert r["draft_ids"][0].tolist() == [21, PAD] and r["draft_new_lens"][0] == 1 and r["tgt_new_lens"][0] == K + 1
    assert r["stats"].tolist() == [1, 7, 7, 1, 0]


def test_ref_partial_and_full_acceptance():
    r = _one([7, 11, 12, 13], [11, 12, 30, 31])  # two proposals agree: t_0, t_1, t_2
    assert r["out"][0, 2:5].tolist() == [11, 12, 30] and r["n_new"][0] == 5
    assert r["lens_t"][0] == 9 and r["lens_d"][0] == 9 and r["draft_ids"][0].tolist() == [30, PAD]
    assert r["stats"].tolist() == [1, 9, 9, 3, 2]
    r = _one([7, 11, 12, 13], [11, 12, 13, 40])  # all three agree: K + 1 tokens, and the draft's cache lacks d_K
    assert r["out"][0, 2:6].tolist() == [11, 12, 13, 40] and r["n_new"][0] == 6
    assert r["lens_t"][0] == 10 and r["lens_d"][0] == 9
    assert r["chunk"][0, 0] == 40
    assert r["draft_ids"][0].tolist() == [13, 40] and r["draft_new_lens"][0] == 2
    assert r["stats"].tolist() == [1, 10, 9, 4, 3]


def test_ref_eos_inside_the_accepted_run():
    r = _one([7, 11, 9, 13], [11, 9, 13, 40])  # t_1 is the EOS id: t_2, t_3 are dropped although they were accepted
    assert r["out"][0].tolist() == [-1, -1, 11, 9] + [-1] * 6
    assert r["n_new"][0] == 4 and r["done"][0] == 1
    assert r["draft_new_lens"][0] == 0 and r["tgt_new_lens"][0] == 0
    assert r["lens_t"][0] == 8 and r["lens_d"][0] == 8
    assert r["stats"].tolist() == [0, 8, 8, 2, 2]
    r = _one([7, 11, 12, 13], [11, 12, 9, 40])  # the EOS id right behind the accepted run: it is the correction token
    assert r["out"][0, 2:5].tolist() == [11, 12, 9] and r["done"][0] == 1 and r["stats"].tolist() == [0, 9, 9, 3, 2]


def test_ref_budget_cut_and_done_row():
    r = _one([7, 11, 12, 13], [11, 12, 13, 40], n_new=8)  # two tokens of budget left
    assert r["out"][0].tolist() == [-1] * 8 + [11, 12] and r["n_new"][0] == 10 and r["done"][0] == 1
    assert r["lens_t"][0] == 14 and r["lens_d"][0] == 14  # no lag: m = 2 < K + 1
    assert r["stats"].tolist() == [0, 14, 14, 2, 2]
    r = _one([7, 11, 12, 13], [11, 12, 13, 40], n_new=6)  # exactly K + 1 left: full acceptance AND done
    assert r["n_new"][0] == 10 and r["done"][0] == 1 and r["lens_d"][0] == r["lens_t"][0] - 1 and r["draft_new_lens"][0] == 0
    r = _one([7, 11, 12, 13], [11, 12, 13, 40], n_new=4, done=1)  # a finished row: nothing emitted, lens restated
    assert (r["out"] == -1).all() and r["n_new"][0] == 4 and r["done"][0] == 1
    assert r["chunk"][0].tolist() == [7, 11, 12, 13] and r["draft_ids"][0].tolist() == [7, PAD]
    assert r["lens_t"][0] == 8 and r["lens_d"][0] == 8 and r["draft_new_lens"][0] == 0 and r["tgt_new_lens"][0] == 0
    assert r["stats"].tolist() == [0, 8, 8, 0, 0]


def test_ref_target_tokens_are_the_sampler_restatement():
    from tests import sampling_ref as R
    rng = np.random.default_rng(3)
    la = (rng.standard_normal((2, K + 1, 64)) * 3).astype(np.float32)
    banned = np.zeros(64, np.uint8)
    banned[int(la[1, 2].argmax())] = 1
    tg, ex = S.target_tokens(la, [4, 9], [0, 1], banned, False, 1, 1.0, 1.0, 0)
    assert not ex.any() and tg[0].tolist() == la[0].argmax(-1).tolist() and tg[1, 2] != la[1, 2].argmax()
    tg, ex = S.target_tokens(la, [4, 9], [1], None, True, 25, 0.8, 1.0, 11, row_ids=[70, 1 << 33])
    want = [int(R.sample_row(la[1, j], None, 25, 0.8, 1.0, 11, [1 << 33], [9 + j], fp64=True)[0][0, 0]) for j in range(K + 1)]
    assert tg[0].tolist() == want


# ---- generate(assistant_model=): refusals that need no GPU ----------------------------------------------------------------------
def _host_model(vocab=502, opt=False):
    import torch
    from slamkit_amd.model.unit_lm import UnitLM, UnitLMConfig
    base = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=2, num_key_value_heads=2, head_dim=64 if opt else 32,
                intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    if opt:
        base = dict(model_type="opt", num_hidden_layers=2, hidden_size=128, num_attention_heads=2, ffn_dim=256,
                    max_position_embeddings=128)
    m = UnitLM.__new__(UnitLM)  # host-only: every check below happens before the model is touched
    m.config = UnitLMConfig(base_model_name="facebook/opt-125m" if opt else "local", base_config=base, vocab_size=vocab)
    m.device = torch.device("cpu")
    return m


def test_generate_assistant_refusals():
    import torch
    m, d = _host_model(), _host_model()
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), max_new_tokens=4)
    with pytest.raises(ValueError, match="UnitLM"):
        m.generate(assistant_model=object(), **kw)
    with pytest.raises(ValueError, match="another model"):
        m.generate(assistant_model=m, **kw)
    with pytest.raises(ValueError, match="vocab_size"):
        m.generate(assistant_model=_host_model(vocab=300), **kw)
    other = _host_model()
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="is on"):
        m.generate(assistant_model=other, **kw)
    for bad in (0, 16, -1, 2.0, "4", True):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            m.generate(assistant_model=d, num_assistant_tokens=bad, **kw)
    with pytest.raises(ValueError, match="num_assistant_tokens"):
        m.generate(num_assistant_tokens=4, **kw)  # without a draft
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(assistant_model=d, num_return_sequences=2, do_sample=True, top_k=5, sampler="engine", **kw)
    with pytest.raises(ValueError, match="return_logprobs"):
        m.generate(assistant_model=d, return_logprobs=True, **kw)
    for c in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[3, 4]]), dict(min_new_tokens=2, eos_token_id=5),
              dict(min_length=7, eos_token_id=5), dict(begin_suppress_tokens=[3])):
        with pytest.raises(ValueError, match="history-dependent"):
            m.generate(assistant_model=d, **c, **kw)
    with pytest.raises(ValueError, match="sampler='engine'"):
        m.generate(assistant_model=d, do_sample=True, top_k=5, **kw)
    with pytest.raises(ValueError, match="sampler='engine'"):
        m.generate(assistant_model=d, do_sample=True, top_k=5, sampler="torch", **kw)
    with pytest.raises(ValueError, match="top_k"):  # the engine sampler's limits hold under an assistant
        m.generate(assistant_model=d, do_sample=True, top_k=300, sampler="engine", **kw)


def test_generate_assistant_refuses_opt_models():
    import torch
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), max_new_tokens=4)
    with pytest.raises(ValueError, match="OPT"):
        _host_model().generate(assistant_model=_host_model(opt=True), **kw)
    with pytest.raises(ValueError, match="OPT"):
        _host_model(opt=True).generate(assistant_model=_host_model(), **kw)
