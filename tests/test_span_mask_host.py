"""CPU tier of span batches (left- and both-side-padded attention masks: UnitLM.forward, slam_forward_unpadded_spans): the host
helper that reads a mask into (starts, lens), the numpy restatement of the span pack rule and of the logits scatter
(tests/span_ref.py) against tests/unpad_ref.py at starts = 0, the ABI surface, and the golden file of the reference's outputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from slamkit_amd.model import UnitLM
from slamkit_amd.model.unit_lm import mask_spans
from tests import span_ref as S
from tests import unpad_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "span_mask.npz")
NEW_SYMBOLS = ("slam_forward_unpadded_spans", "slam_op_unpad_pack_spans", "slam_op_unpad_logits_spans")


def _mask(T, spans):
    m = torch.zeros(len(spans), T, dtype=torch.int64)
    for b, (s, n) in enumerate(spans):
        m[b, s:s + n] = 1
    return m


# --------------------------------------------------------------------------------------------------------- the host helper
@pytest.mark.parametrize("name,T,spans", [
    ("right", 8, [(0, 8), (0, 3), (0, 1)]),
    ("left", 8, [(0, 8), (5, 3), (7, 1)]),
    ("both", 8, [(2, 3), (1, 6), (3, 1)]),
    ("mixed", 9, [(0, 4), (5, 4), (2, 5), (0, 9)]),
    ("lens_T", 5, [(0, 5), (0, 5)]),
    ("lens_1", 5, [(0, 1), (4, 1), (2, 1)]),
    ("T_1", 1, [(0, 1)]),
])
def test_mask_spans_reads_one_run_per_row(name, T, spans):
    for dtype in (torch.int64, torch.bool, torch.float32):
        st, ln = mask_spans(_mask(T, spans).to(dtype))
        assert st.dtype == torch.int32 and ln.dtype == torch.int32 and not st.is_cuda
        assert st.tolist() == [s for s, _ in spans] and ln.tolist() == [n for _, n in spans]
    # what forward goes by: a span batch only when some row starts past column 0
    got = UnitLM._host_spans(len(spans), T, _mask(T, spans), None, None, True)
    if all(s == 0 for s, _ in spans):
        assert got is None  # right padding: the routes it always took, with the switch on or off
        assert UnitLM._host_spans(len(spans), T, _mask(T, spans), None, None) is None
        assert UnitLM._host_lengths(len(spans), T, _mask(T, spans), None).tolist() == [n for _, n in spans]
    else:
        assert got[0].tolist() == [s for s, _ in spans] and got[1].tolist() == [n for _, n in spans]
        with pytest.raises(ValueError, match="right-padded"):  # span masks are opt-in: off, the mask is refused as before
            UnitLM._host_spans(len(spans), T, _mask(T, spans), None, None)


def test_mask_spans_refuses_holes_and_empty_rows():
    with pytest.raises(ValueError, match="row 1 has a hole"):
        mask_spans(torch.tensor([[1, 1, 1, 0], [1, 0, 1, 1], [0, 1, 1, 0]]))
    with pytest.raises(ValueError, match="hole"):
        mask_spans(torch.tensor([[0, 1, 0, 0, 1, 0]]))
    with pytest.raises(ValueError, match="row 2 is all zeros"):
        mask_spans(torch.tensor([[1, 1], [0, 1], [0, 0]]))
    # forward's gate is the same helper: refused with padding_free on or off, before anything touches a device
    for am in (torch.tensor([[1, 0, 1]]), torch.tensor([[0, 0, 0]])):
        with pytest.raises(ValueError, match="hole|all zeros"):
            UnitLM._host_spans(1, 3, am, None, None, True)
    # with the switch off nothing moved: a hole is "not right padding", a row of zeros passes as it did
    with pytest.raises(ValueError, match="right-padded"):
        UnitLM._host_spans(1, 3, torch.tensor([[1, 0, 1]]), None, None)
    assert UnitLM._host_spans(1, 3, torch.tensor([[0, 0, 0]]), None, None) is None


class _OnDevice(torch.Tensor):
    """A tensor that reports itself on the device (this tier has none): the check reads .is_cuda and nothing else."""
    is_cuda = True


def test_explicit_starts_and_lengths():
    """starts= with lengths= is a per-call request: honoured with the span_masks switch off."""
    hs = UnitLM._host_spans
    st, ln = hs(3, 10, None, [10, 4, 1], [0, 6, 3])
    assert st.tolist() == [0, 6, 3] and ln.tolist() == [10, 4, 1] and st.dtype == ln.dtype == torch.int32
    st, ln = hs(2, 10, None, torch.tensor([4, 5]), torch.tensor([6, 0], dtype=torch.int32))
    assert st.tolist() == [6, 0] and ln.tolist() == [4, 5]
    assert hs(2, 10, None, [3, 10], [0, 0]) is None          # all rows from column 0: right padding, today's routes
    assert hs(2, 10, None, [3, 10], None) is None            # lengths alone are right padding
    assert hs(2, 10, None, None, None) is None
    am = _mask(10, [(2, 3), (0, 10)])
    assert hs(2, 10, am, [3, 10], None, True) is None        # explicit lengths win over the mask, as they always did
    assert hs(2, 10, am, [5, 5], [5, 0])[0].tolist() == [5, 0]
    for lengths, starts in (([0, 1], [1, 1]), ([5, 6], [0, 5]), ([1, 1], [-1, 0]), ([1, 1, 1], [0, 1, 2]), ([1], [1])):
        with pytest.raises(ValueError, match="span batch"):
            hs(2, 10, None, lengths, starts)
    with pytest.raises(ValueError, match="starts needs lengths"):
        hs(2, 10, None, None, [0, 1])
    on_dev = torch.tensor([4, 5]).as_subclass(_OnDevice)
    assert on_dev.is_cuda
    with pytest.raises(ValueError, match="host"):
        hs(2, 10, None, on_dev, [1, 0])
    with pytest.raises(ValueError, match="host"):
        hs(2, 10, None, [4, 5], on_dev)
    with pytest.raises(ValueError, match="host"):  # and the right-padded route refuses device lengths as before
        UnitLM._host_lengths(2, 10, None, on_dev)


# --------------------------------------------------------------------------------------------------- the numpy restatement
@pytest.mark.parametrize("B,T,lens,Mp", [(3, 64, [64, 1, 37], None), (3, 64, [64, 1, 37], 192), (2, 64, [64, 64], None),
                                        (1, 37, [37], None), (300, 7, None, None)])
@pytest.mark.parametrize("with_labels", [True, False])
def test_span_ref_equals_unpad_ref_at_starts_zero(B, T, lens, Mp, with_labels):
    rng = np.random.default_rng(5)
    lens = rng.integers(1, T + 1, B) if lens is None else lens
    ids, lab = rng.integers(1, 502, (B, T)), rng.integers(1, 502, (B, T))
    want = R.pack(ids, lab if with_labels else None, lens, Mp)
    for starts in (None, np.zeros(B, np.int64)):
        got = S.pack(ids, lab if with_labels else None, starts, lens, Mp)
        assert sorted(got) == sorted(want)
        for k in want:
            assert (got[k] is None and want[k] is None) or np.array_equal(got[k], want[k]), k
    vals = rng.integers(1, 1000, (len(want["ids"]), 3))
    assert np.array_equal(S.scatter_rows(vals, want["off"], None, B, T), R.unpack_rows(vals, want["off"], B, T))


def test_span_ref_pack_rule():
    ids = np.arange(1, 1 + 3 * 40).reshape(3, 40)
    lab = ids + 1000
    starts, lens = [0, 23, 9], [40, 17, 12]
    p = S.pack(ids, lab, starts, lens)
    assert len(p["ids"]) == 128 and p["off"].tolist() == [0, 40, 57, 69]
    assert p["ids"][:40].tolist() == ids[0].tolist() and p["ids"][40:57].tolist() == ids[1, 23:].tolist()
    assert p["ids"][57:69].tolist() == ids[2, 9:21].tolist()
    assert p["position_ids"][38:43].tolist() == [38, 39, 0, 1, 2] and p["position_ids"][56:59].tolist() == [16, 0, 1]
    # a row's first real token is never a target; every other real token keeps its label
    assert [p["labels"][o] for o in (0, 40, 57)] == [-100] * 3
    assert p["labels"][41:57].tolist() == lab[1, 24:].tolist() and p["labels"][58:69].tolist() == lab[2, 10:21].tolist()
    assert (p["seg_start"][40:57] == 40).all() and (p["seg_end"][40:57] == 57).all() and (p["row"][57:69] == 2).all()
    assert (p["ids"][69:] == 0).all() and (p["labels"][69:] == -100).all() and (p["row"][69:] == -1).all()
    assert p["position_ids"][69:].tolist() == list(range(59)) and (p["seg_start"][69:] == 69).all() and (p["seg_end"][69:] == 128).all()
    # the scatter is the inverse on the spans and zero on both sides
    back = S.scatter_rows(p["ids"], p["off"], starts, 3, 40)
    m = _mask(40, list(zip(starts, lens))).numpy().astype(bool)
    assert np.array_equal(back[m], ids[m]) and (back[~m] == 0).all()
    # the memory guard: starts to [0, T], lens to [0, T - starts] - a span that breaks its contract is cut, never read past its row
    q = S.pack(ids, lab, [30, 50, -4], [17, 3, 50], Mp=128)
    assert q["off"].tolist() == [0, 10, 10, 50] and q["ids"][:10].tolist() == ids[0, 30:].tolist()
    assert q["ids"][10:50].tolist() == ids[2].tolist() and q["row"][10] == 2


def test_spans_for_covers_the_three_placements():
    st, ln = S.spans_for(300, 7, 1)
    assert ((st >= 0) & (ln >= 1) & (st + ln <= 7)).all()
    assert (st == 0).any() and ((st + ln == 7) & (st > 0)).any() and ((st > 0) & (st + ln < 7)).any()


# ------------------------------------------------------------------------------------------------------------ ABI surface
def test_symbols_declared_exported_and_bound():
    lib = E.load_library()
    names = E.header_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(lib, n) and n in lib._slam_signatures, n


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Nothing here reaches a device; starts may be NULL everywhere (right padding)."""
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(2, 256, 4, 2, 64, 512, 502, 0, 1e-6, 10000.0))
    one = C.c_void_p(256)
    sb = E.unpadded_scratch_bytes(2, 64)
    p = lib.slam_op_unpad_pack_spans
    assert p(None, None, one, one, 2, 64, 128, 0, one, sb, None) == -1
    assert p(one, None, one, None, 2, 64, 128, 0, one, sb, None) == -1       # lens are not optional
    assert p(one, None, one, one, 2, 64, 100, 0, one, sb, None) == -1
    assert p(one, None, None, one, 2, 64, 128, 0, one, sb - 1, None) == -1
    f = lib.slam_forward_unpadded_spans
    assert f(eng.h, one, None, one, one, 2, 64, 96, one, sb, 0.0, None, None, None) == -1
    assert f(eng.h, one, None, one, None, 2, 64, 128, one, sb, 0.0, None, None, None) == -1
    assert f(eng.h, one, None, one, one, 2, 64, 128, one, sb, 0.0, None, None, None) == -2  # no params / workspace bound
    assert f(eng.h, one, None, None, one, 2, 64, 128, one, sb, 0.0, None, None, None) == -2
    assert b"bind params" in lib.slam_last_error(eng.h)
    assert f(None, one, None, one, one, 2, 64, 128, one, sb, 0.0, None, None, None) == -1
    s = lib.slam_op_unpad_logits_spans
    assert s(None, 512, one, 502, one, one, 2, 64, 128, None) == -1
    assert s(one, 512, one, 502, None, one, 2, 64, 128, None) == -1
    assert s(one, 508, one, 502, one, None, 2, 64, 128, None) == -1          # Vp % 8
    eng.close()


# ------------------------------------------------------------------------------------------------------------- the golden
def test_golden_file_loads_and_rows_equal_themselves_alone():
    g = dict(np.load(GOLDEN))
    assert g["ids"].shape == (3, 40) and g["starts"].tolist() == [0, 23, 9] and g["lens"].tolist() == [40, 17, 12]
    st, ln = mask_spans(torch.from_numpy(g["mask"]))
    assert st.tolist() == g["starts"].tolist() and ln.tolist() == g["lens"].tolist()
    p = S.pack(g["ids"], g["labels"], g["starts"], g["lens"])
    # the stored labels already follow the rule: -100 outside the spans and at each row's first real token
    real = g["mask"].astype(bool)
    assert (g["labels"][~real] == -100).all() and np.array_equal(p["labels"][:69], g["labels"][real])
    for name in ("qwen2", "opt"):
        assert g[name + "_logits_real"].shape == (69, 502) and np.isfinite(g[name + "_logits_real"]).all()
        assert np.isfinite(g[name + "_loss"]) and np.isfinite(g[name + "_loss_num_items"])
        assert len(g[name + "_grad_names"]) == len(g[name + "_grad_norms"]) and np.isfinite(g[name + "_grad_norms"]).all()
        assert g[name + "_row_alone_maxdiff"].shape == (3,) and float(g[name + "_row_alone_maxdiff"].max()) < 1e-5
