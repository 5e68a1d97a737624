"""CPU: the numpy restatement of slam_constrain_scores (tests/constrain_ref.py) against the installed transformers' own logits
processors (tests/golden/constrain_hf.npz, make_golden_constrain.py), exactly; the entry point's argument checks, which return
before any launch; generate's argument checks that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

from slamkit_amd import engine as E
from tests import constrain_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "constrain_hf.npz")


def _lists(g, name, lo=0, hi=None):
    val, off = g[name + "_val"], g[name + "_off"]
    hi = len(off) - 1 if hi is None else hi
    return [val[off[i]:off[i + 1]].tolist() for i in range(lo, hi)]


def test_ref_equals_hf_banned_sets():
    g = dict(np.load(GOLDEN))
    V = int(g["vocab"])
    hist, eos, begin, banned = (_lists(g, k) for k in ("hist", "eos", "begin", "banned"))
    n_cases = len(hist)
    assert n_cases >= 300 and sum(len(b) > 0 for b in banned) >= n_cases // 2
    seen = {"ngram": 0, "seq": 0, "eos": 0, "begin": 0}
    for c in range(n_cases):
        h, pl = hist[c], int(g["prompt_len"][c])
        step = len(h) - pl
        seqs = _lists(g, "seq", int(g["seq_case"][c]), int(g["seq_case"][c + 1]))
        # the host's rule for the flag (UnitLM.generate): HF's cur_len is the prompt width as passed; the fixtures are unpadded
        ban_eos = step < int(g["min_new_tokens"][c]) or pl + step < int(g["min_length"][c])
        got = R.banned_set(h, step, V, int(g["ngram"][c]), seqs, ban_eos, eos[c], begin[c])
        assert got == set(banned[c]), (c, h, pl, int(g["ngram"][c]), seqs, eos[c], begin[c], sorted(got), banned[c])
        seen["ngram"] += bool(R.ngram_bans(h, int(g["ngram"][c])))
        seen["seq"] += bool(R.sequence_bans(h, seqs))
        seen["eos"] += bool(ban_eos)
        seen["begin"] += bool(step == 0 and begin[c])
    assert all(v >= 10 for v in seen.values()), seen  # every kind of ban is exercised


def test_ref_scores_and_edge_rules():
    x = np.array([[0.5, np.nan, -np.inf, np.inf, 1.0], [1.0, 2.0, 3.0, 4.0, 5.0]], np.float32)
    sets, s = R.constrain(x, [[1, 3, 1], [7, -2, 7]], step=1, n=2, ban_eos=True, eos_ids=[4, 9, -1], done=[0, 0])
    assert sets == [{3, 4}, {4}]  # row 1: the window (7, -2) bans -2, which is no id; EOS ids outside the row are dropped
    assert np.isneginf(s[0, [3, 4]]).all() and s[0, 0] == 0.5 and np.isnan(s[0, 1]) and np.isneginf(s[0, 2])
    assert np.array_equal(s[1, :4], x[1, :4])
    sets, s = R.constrain(x, [[1, 3, 1], [1, 1, 1]], step=1, n=1, done=[1, 0])
    assert sets == [set(), {1}] and np.array_equal(s[0].view(np.int32), x[0].view(np.int32))
    assert R.ngram_bans([1, 2], 3) == set() and R.ngram_bans([], 1) == set() and R.ngram_bans([5], 1) == {5}
    assert R.sequence_bans([1, 2], [[1, 2, 3], [2, 4], [4]]) == {4}
    assert R.has_repeated_ngram([1, 2, 3, 1, 2, 3], 3) and not R.has_repeated_ngram([1, 2, 3, 1, 2], 3)


def _desc(**kw):
    d = dict(step=0, no_repeat_ngram=3, n_per_prompt=1, prompt_stride=16, ban_eos=0, n_eos=0, n_begin=0, n_seqs=0, n_seq_tokens=0)
    d.update(kw)
    return E.SlamConstrainDesc(**d)


def test_constrain_scores_rejects_bad_arguments_before_any_launch():
    lib = E.load_library()
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch

    def call(logits=fake, scores=fake, B=6, V=502, use_desc=True, prompt=fake, plen=fake, new=fake, stride=64, eos=None,
             begin=None, st=None, so=None, **kw):
        d = C.byref(_desc(**kw)) if use_desc else None
        return lib.slam_constrain_scores(logits, scores, B, V, d, prompt, plen, new, stride, None, eos, begin, st, so, None)

    bad = [dict(logits=None), dict(scores=None), dict(use_desc=False), dict(prompt=None), dict(plen=None),
           dict(B=0), dict(B=-1), dict(B=65536), dict(V=0), dict(no_repeat_ngram=-1), dict(n_per_prompt=0),
           dict(n_per_prompt=4), dict(ban_eos=2), dict(step=-1), dict(step=1, new=None), dict(step=65, stride=64),
           dict(prompt_stride=-1), dict(n_eos=1), dict(n_eos=17, eos=fake), dict(n_eos=-1), dict(n_begin=1),
           dict(n_begin=E.CONSTRAIN_MAX_BEGIN + 1, begin=fake), dict(n_seqs=1, st=fake), dict(n_seqs=1, so=fake),
           dict(n_seqs=E.CONSTRAIN_MAX_SEQS + 1, st=fake, so=fake),
           dict(n_seqs=1, n_seq_tokens=E.CONSTRAIN_MAX_SEQS * E.CONSTRAIN_MAX_SEQ_LEN + 1, st=fake, so=fake),
           dict(logits=C.c_void_p((1 << 20) + 2)), dict(scores=C.c_void_p((1 << 20) + 1)), dict(prompt=C.c_void_p((1 << 20) + 4)),
           dict(step=1, new=C.c_void_p((1 << 20) + 4)), dict(n_eos=1, eos=C.c_void_p((1 << 20) + 2))]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert R.MAX_SEQS == E.CONSTRAIN_MAX_SEQS and R.MAX_SEQ_LEN == E.CONSTRAIN_MAX_SEQ_LEN and R.MAX_BEGIN == E.CONSTRAIN_MAX_BEGIN
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slam_engine.h")).read()
    for name, v in (("SEQS", E.CONSTRAIN_MAX_SEQS), ("SEQ_LEN", E.CONSTRAIN_MAX_SEQ_LEN), ("BEGIN", E.CONSTRAIN_MAX_BEGIN)):
        assert f"#define SLAM_CONSTRAIN_MAX_{name} {v}\n" in hdr


def test_constraint_plan_validation():
    """The part of generate's argument handling that needs no device: caps and ranges raise ValueError."""
    from slamkit_amd.model.unit_lm import _constraint_plan
    p = _constraint_plan(no_repeat_ngram_size=0, min_new_tokens=0, min_length=0, begin_suppress=[], suppress=[], bad=[], eos=[3])
    assert not p.active and p.single == []
    p = _constraint_plan(3, 2, 0, [1], [7], [[4], [5, 6], [5, 6, 7]], [3])
    assert p.active and sorted(p.single) == [4, 7] and p.seqs == [[5, 6], [5, 6, 7]] and p.begin == [1]
    p = _constraint_plan(0, 5, 0, [], [], [], [])  # no EOS id: min_new_tokens has nothing to ban
    assert not p.active
    for kw in (dict(no_repeat_ngram_size=-1), dict(min_new_tokens=-1), dict(min_length=-2), dict(bad=[[]]),
               dict(bad=[[1, 2]] * (E.CONSTRAIN_MAX_SEQS + 1)), dict(bad=[list(range(E.CONSTRAIN_MAX_SEQ_LEN + 1))]),
               dict(begin_suppress=list(range(E.CONSTRAIN_MAX_BEGIN + 1))), dict(no_repeat_ngram_size=2.5),
               dict(min_new_tokens=1, eos=list(range(17)))):
        a = dict(no_repeat_ngram_size=0, min_new_tokens=0, min_length=0, begin_suppress=[], suppress=[], bad=[], eos=[3])
        a.update(kw)
        with pytest.raises(ValueError):
            _constraint_plan(**a)
