"""CPU tier of prompt-lookup decoding: slam_ngram_propose is declared, exported and bound; it refuses bad arguments before
anything reaches the device (fake pointers, as in test_spec_host.py); tests/lookup_ref.py against transformers' own
PromptLookupCandidateGenerator (tests/golden/lookup_hf.npz, make_golden_lookup.py), exactly, and against hand-worked rows; the
ValueErrors of generate(prompt_lookup_num_tokens=) on model objects that never touch a GPU."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from slamkit_amd import engine as E
from tests import lookup_ref as L
from tests.test_spec_host import _host_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookup_hf.npz")
E_INVAL = -1
FAKE = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch


def test_new_symbol_exported_and_bound():
    lib = E.load_library()
    n = "slam_ngram_propose"
    assert n in E.header_symbols() and hasattr(lib, n) and n in lib._slam_signatures
    assert callable(E.ngram_propose) and E.NGRAM_MAX == 16 and E.NGRAM_STATS == ("rows", "proposed")


def _propose(**kw):
    a = dict(chunk=FAKE, n_prop=FAKE, B=3, K=4, max_ngram=2, fill_id=0, prompt=FAKE, prompt_stride=16, prompt_len=FAKE, new=FAKE,
             new_stride=8, n_new=FAKE, done=FAKE, eos_ids=FAKE, n_eos=1, stats=FAKE)
    a.update(kw)
    return E.load_library().slam_ngram_propose(*a.values(), None)


def test_ngram_propose_refused_before_a_launch():
    for name in ("chunk", "n_prop", "prompt", "prompt_len", "new", "n_new", "done", "eos_ids"):
        assert _propose(**{name: None}) == E_INVAL, name
    for kw in (dict(B=0), dict(B=1025), dict(B=-3), dict(K=0), dict(K=16), dict(K=-1), dict(max_ngram=0), dict(max_ngram=17),
               dict(max_ngram=-2), dict(n_eos=17), dict(n_eos=-1), dict(prompt_stride=-1), dict(new_stride=-1),
               dict(prompt_stride=1 << 30), dict(new_stride=1 << 30)):
        assert _propose(**kw) == E_INVAL, kw


def _lists(g, name):
    val, off = g[name + "_val"], g[name + "_off"]
    return [val[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def test_ref_equals_hf_candidates():
    g = dict(np.load(GOLDEN))
    hist, eos, cand = (_lists(g, k) for k in ("hist", "eos", "cand"))
    assert len(hist) >= 300
    seen = dict(none=0, some=0, cut=0, emptied=0, short=0)
    sizes = set()
    for c in range(len(hist)):
        K, n = int(g["K"][c]), int(g["max_ngram"][c])
        got, size, idx = L.propose(hist[c], K, n, eos[c])
        assert got == cand[c], (c, hist[c], K, n, eos[c], got, cand[c])
        free = L.propose(hist[c], K, n)[0]
        sizes.add(size)
        seen["none"] += size == 0
        seen["some"] += bool(got)
        seen["cut"] += 0 < len(got) < len(free)   # an EOS id inside the candidates
        seen["emptied"] += size > 0 and not got   # an EOS id in front of them: nothing proposed, no fall-back
        seen["short"] += len(hist[c]) <= 2
    assert all(v >= 10 for v in seen.values()), seen
    assert {0, 1, 2, 3, 4, 5} <= sizes, sizes  # every n-gram size matched somewhere


def test_ref_hand_worked_rows():
    assert L.propose([7], 4, 3) == ([], 0, -1)                      # Lh == 1
    assert L.propose([7, 8], 4, 3) == ([], 0, -1)                   # no match
    assert L.propose([7, 7], 4, 3) == ([7], 1, 0)                   # the continuation is cut by the end of the history
    assert L.propose([5, 5, 5, 5], 4, 3) == ([5], 3, 0)             # a match overlapping the tail
    assert L.propose([5, 5, 5, 5], 4, 16) == ([5], 3, 0)            # max_ngram above Lh - 1
    assert L.propose([1, 2, 3, 9, 1, 2, 4, 8, 1, 2], 2, 2) == ([3, 9], 2, 0)      # the EARLIEST match of the longest n
    assert L.propose([1, 2, 5, 7, 1, 2, 4, 7, 1, 2], 3, 3) == ([4, 7, 1], 3, 3)   # the longest n beats an earlier shorter match
    assert L.propose([1, 2, 9, 4, 2, 3, 1, 2], 3, 2, [9]) == ([], 2, 0)           # EOS first: nothing, although n = 1 matches
    assert L.propose([1, 2, 3, 9, 4, 1, 2], 3, 2, [9]) == ([3], 2, 0)             # EOS in the middle
    r = L.propose_rows(np.full((3, 4), -7), [[1, 2, 1, 0], [1, 2, 1, 2], [4, 4, 4, 4]], [3, 4, 4], [[2, 5], [5, 5], [4, 5]],
                       [1, 0, 1], [0, 0, 1], 3, 2, 0)
    assert r["chunk"].tolist() == [[-7, 1, 2, 0], [-7, 1, 2, 0], [-7, 0, 0, 0]]  # row 0 straddles prompt / new; row 2 is done
    assert r["n_prop"].tolist() == [2, 2, 0] and r["stats"].tolist() == [2, 4]


# ---- generate(prompt_lookup_num_tokens=): refusals that need no GPU -------------------------------------------------------------
def test_generate_lookup_refusals():
    import torch
    m, d = _host_model(), _host_model()
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), max_new_tokens=4)
    with pytest.raises(ValueError, match="exclude each other"):
        m.generate(assistant_model=d, prompt_lookup_num_tokens=4, **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size needs"):
        m.generate(max_matching_ngram_size=2, **kw)
    for bad in (0, 16, -1, 2.0, "4", True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens must"):
            m.generate(prompt_lookup_num_tokens=bad, **kw)
    for bad in (0, 17, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="max_matching_ngram_size must"):
            m.generate(prompt_lookup_num_tokens=4, max_matching_ngram_size=bad, **kw)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(prompt_lookup_num_tokens=4, num_return_sequences=2, do_sample=True, top_k=5, sampler="engine", **kw)
    with pytest.raises(ValueError, match="return_logprobs"):
        m.generate(prompt_lookup_num_tokens=4, return_logprobs=True, **kw)
    for c in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[3, 4]]), dict(min_new_tokens=2, eos_token_id=5),
              dict(min_length=7, eos_token_id=5), dict(begin_suppress_tokens=[3])):
        with pytest.raises(ValueError, match="history-dependent"):
            m.generate(prompt_lookup_num_tokens=4, **c, **kw)
    with pytest.raises(ValueError, match="sampler='engine'"):
        m.generate(prompt_lookup_num_tokens=4, do_sample=True, top_k=5, **kw)
    with pytest.raises(ValueError, match="sampler='engine'"):
        m.generate(prompt_lookup_num_tokens=4, do_sample=True, top_k=5, sampler="torch", **kw)
    with pytest.raises(ValueError, match="top_k"):  # the engine sampler's limits hold under lookup
        m.generate(prompt_lookup_num_tokens=4, do_sample=True, top_k=300, sampler="engine", **kw)
    with pytest.raises(ValueError, match="OPT"):
        _host_model(opt=True).generate(prompt_lookup_num_tokens=4, **kw)
    with pytest.raises(ValueError, match="1024 rows"):
        m.generate(input_ids=torch.ones(1025, 4, dtype=torch.long), max_new_tokens=4, prompt_lookup_num_tokens=4)


def test_generate_lookup_reads_generation_config():
    import torch
    m = _host_model()
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), max_new_tokens=4)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens must"):
        m.generate(generation_config=types.SimpleNamespace(prompt_lookup_num_tokens=99), **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size must"):
        m.generate(generation_config=types.SimpleNamespace(prompt_lookup_num_tokens=4, max_matching_ngram_size=99), **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size needs"):
        m.generate(generation_config=types.SimpleNamespace(max_matching_ngram_size=3), **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size must"):  # the explicit argument overrides the config
        m.generate(generation_config=types.SimpleNamespace(prompt_lookup_num_tokens=4, max_matching_ngram_size=3),
                   max_matching_ngram_size=0, **kw)
