"""CPU tier of the exact attention parity tests: the evidence that the inputs of tests/test_gpu_attn_exact.py are what
tests/attn_exact_ref.py says they are - for every case the GPU file runs, with no row exempted - and that the comparison
would notice the defects it is there for. No GPU, no library call.

  * the six conditions of the generator, proved on the finished tensors;
  * the expected bits (bf16 of the plain fp64 reference) are also the bits of the same function evaluated with the roundings
    any bf16-MFMA flash kernel makes (P, O and dS to bf16 before their second products): the match the GPU file demands is
    guaranteed by the inputs, not lucky;
  * sensitivity, on data alone: leaking key i + 1 or key seg_start - 1 into a row changes that row of o for EVERY row;
    leaving out one (16-row fragment x 64-key tile) product of the backward changes dq or dv for every sampled pair;
  * for contrast the same leak and the same dropped product on test_attention_fwd_bwd's Gaussian inputs at [1024], next to
    that test's bars (figures in profiles/attn_exact.md)."""
import time

import pytest
import torch

from tests import attn_exact_ref as R
from tests.gpu_util import rnd
from tests.test_gpu_attn_block import _attn_ref64
from tests.test_gpu_ops import _attn_case, _attn_prescale

CASE_IDS = R.case_ids()


def _id(cid):
    return f"{cid[0]}-{cid[1]}-{cid[2]}-{cid[3]}"


@pytest.mark.parametrize("cid", CASE_IDS, ids=_id)
def test_generator_conditions(cid):
    """Conditions 1-6 (attn_exact_ref.check_conditions) on every case of the GPU file; a single KV head is proved over its two
    parities together, as the GPU file runs both. Also: the generator is deterministic and takes about a second."""
    t0 = time.time()
    cases = R.cases_of(*cid)
    fig = R.check_conditions(cases)
    took = time.time() - t0
    print(f"[attn-exact] {_id(cid)}: M={cases[0].M} fragment x tile pairs={fig.pairs} tie sizes={fig.sizes} tie share={fig.tie_share:.3f} "
          f"d_o density={fig.density} nonzero dq/dk/dv={fig.nonzero['dq']:.2f}/{fig.nonzero['dk']:.2f}/{fig.nonzero['dv']:.2f} "
          f"generated and checked in {took:.2f} s")
    again = R.make_case(cases[0].seg_lens, cid[1], cid[2], cid[3], cases[0].seed, cases[0].flip)
    assert torch.equal(again.qkv_dev, cases[0].qkv_dev) and torch.equal(again.d_o, cases[0].d_o) and again.ties == cases[0].ties


def test_case_list_is_the_one_the_issue_sets():
    shapes = R.SHAPES
    assert [sum(v) for v in shapes.values()] == [1, 6, 128, 256, 129, 300, sum(shapes["many_short"]), 1433, 1296]
    assert shapes["many_short"][:40] == [(3 * i) % 7 + 1 for i in range(40)] and shapes["many_short"][40:] == [257]
    ids = R.case_ids()
    assert len(ids) == 9 + 3 * 5 and all((n, 4, 2, 64) in ids for n in shapes)
    for n in R.LAST_THREE:
        assert {i[1:] for i in ids if i[0] == n} == {(4, 2, 64), (4, 2, 128), (7, 1, 64), (3, 3, 64), (3, 3, 128), (6, 1, 128)}
    assert 1433 % 64 == 25 and max(sum(v) for v in shapes.values()) == 1433


@pytest.mark.parametrize("cid", CASE_IDS, ids=_id)
def test_rounded_emulation_reproduces_the_expected_bits(cid):
    """bf16(fp64 reference) == bf16(the exp2-domain function with P, O and dS rounded to bf16) for o, dv and head_dim-64 dq,
    bit for bit; lse2 equal; dk and head_dim-128 dq (one irrational factor) within fp64 noise of each other. The unrounded
    evaluation gives the same: the roundings have nothing to round."""
    for c in R.cases_of(*cid):
        exp = R.expectations(c, _attn_ref64)
        for rounded in (True, False):
            emu = c.exact if not rounded else R.exact_values(c, round_bf16=True)
            assert emu.ds_is_bf16
            name = f"{R.describe(c)} rounded={rounded}"
            R.assert_bits(f"{name} o", c, "o", (emu.o + 0.0).to(R.F32).to(R.BF16), exp.o)
            R.assert_bits(f"{name} dv", c, "dv", (emu.dv + 0.0).to(R.F32).to(R.BF16), exp.dv)
            assert torch.equal(emu.lse2, exp.lse2), f"{name}: lse2"
            dq = emu.dq * R.dq_factor(c.hd)
            if c.hd == 64:
                R.assert_bits(f"{name} dq", c, "dq", (dq + 0.0).to(R.F32).to(R.BF16), exp.dq)
            else:
                assert float((dq - exp.dq_ref).abs().max()) <= 1e-6 * max(1.0, float(exp.dq_ref.abs().max())), f"{name}: dq"
                assert torch.equal(dq == 0, exp.dq_ref == 0), f"{name}: zeros of dq"
            dk = emu.dk * 0.6931471805599453
            assert float((dk - exp.dk_ref).abs().max()) <= 1e-9 * max(1.0, float(exp.dk_ref.abs().max())), f"{name}: dk"
            assert torch.equal(dk == 0, exp.dk_ref == 0), f"{name}: zeros of dk"


def _rows_changed(a, b, c, width):
    """bool [M]: the bf16 bits of row i differ in some column."""
    return (R.bits(a.to(R.F32).to(R.BF16)) != R.bits(b.to(R.F32).to(R.BF16))).reshape(c.M, width).any(1)


SENSITIVITY_CASES = [(n, 4, 2, 64) for n in ("residue_63", "aligned_boundaries") + R.LAST_THREE] + \
                    [("ragged_1433", 7, 1, 64), ("sixteen_key_tiles", 3, 3, 128)]


@pytest.mark.parametrize("cid", SENSITIVITY_CASES, ids=_id)
def test_a_leaked_key_changes_its_row(cid):
    """In the rounded emulation, make key i + 1 visible to row i - for all rows at once, each row's o depends on its own mask
    only - and likewise key seg_start - 1. Every row must change in the bf16 bits of o in at least one head (over the two
    parities of a single KV head): condition 3 at work. dq follows in the tie rows."""
    cases = R.cases_of(*cid)
    c0 = cases[0]
    rows = torch.arange(c0.M)
    seg_s = c0.seg_start.long()
    for what, sel, key in (("key i+1", rows + 1 < c0.M, rows + 1), ("key seg_start-1", seg_s > 0, seg_s - 1)):
        if not bool(sel.any()):
            continue
        changed = torch.zeros(c0.M, dtype=torch.bool)
        for c in cases:
            base = R.exact_values(c, round_bf16=True)
            leaky = R.exact_values(c, round_bf16=True, leak=list(zip(rows[sel].tolist(), key[sel].tolist())))
            changed |= _rows_changed(base.o, leaky.o, c, c.nH * c.hd)
        missed = sel & ~changed
        assert not bool(missed.any()), f"{R.describe(c0)}: leaking {what} leaves o of row {int(missed.nonzero()[0])} unchanged"
        print(f"[attn-exact] {_id(cid)}: leaking {what}: o changes in {int((sel & changed).sum())} of {int(sel.sum())} rows")


@pytest.mark.parametrize("cid", SENSITIVITY_CASES, ids=_id)
def test_a_dropped_fragment_tile_product_changes_dq_or_dv(cid):
    """Leave one (16-row fragment x 64-key tile) block of P and dS out of the backward products: dq of the fragment's rows or
    dv of the tile's keys must change in their bf16 bits. Sampled pairs with distinct fragments and distinct tiles are dropped
    together (dq rows belong to one fragment, dv rows to one tile, so every instance is judged on its own rows): condition 4
    at work. A single KV head is judged over its two parities."""
    cases = R.cases_of(*cid)
    c0 = cases[0]
    vis = R.visible(c0)
    r, k = vis.nonzero(as_tuple=True)
    pairs = sorted(set(zip((r // 16).tolist(), (k // 64).tolist())))
    g = torch.Generator().manual_seed(3)
    order = torch.randperm(len(pairs), generator=g).tolist()
    rounds = []
    for _ in range(3):   # three rounds of a greedy matching over a shuffled list
        frags, tiles, picked = set(), set(), []
        for idx in order:
            f, t = pairs[idx]
            if f not in frags and t not in tiles and (f, t) not in [p for rr in rounds for p in rr]:
                frags.add(f), tiles.add(t), picked.append((f, t))
        if picked:
            rounds.append(picked)
        order = order[::-1] if len(rounds) == 1 else order[len(order) // 2:] + order[: len(order) // 2]
    base = [R.exact_values(c, round_bf16=True) for c in cases]
    n = 0
    for picked in rounds:
        hit = {p: False for p in picked}
        for c, b in zip(cases, base):
            d = R.exact_values(c, round_bf16=True, drop=picked)
            dq, dv = _rows_changed(b.dq, d.dq, c, c.nH * c.hd), _rows_changed(b.dv, d.dv, c, c.nKV * c.hd)
            for f, t in picked:
                hit[(f, t)] |= bool(dq[16 * f:16 * f + 16].any()) or bool(dv[64 * t:64 * t + 64].any())
        missed = [p for p, h in hit.items() if not h]
        assert not missed, f"{R.describe(c0)}: dropping fragment x tile {missed[0]} changes neither dq nor dv"
        n += len(picked)
    print(f"[attn-exact] {_id(cid)}: {n} of {len(pairs)} fragment x tile pairs dropped one by one, each changed dq or dv")


# ------------------------------------------------------------------------------------------------ the contrast
def _gaussian_attention(q, k, v, d_o, mask, drop=None):
    """fp64 masked attention of one head and its dq (in units of the scale) - enough to see what a defect moves."""
    s = (q @ k.t()).masked_fill(~mask, -float("inf"))
    p = torch.softmax(s, -1)
    o = p @ v
    ds = p * (d_o @ v.t() - (d_o * o).sum(-1, keepdim=True))
    if drop is not None:
        f, t = drop
        ds = ds.clone()
        ds[16 * f:16 * f + 16, 64 * t:64 * t + 64] = 0
    return o, ds @ k


def test_gaussian_inputs_do_not_see_the_same_defects():
    """test_attention_fwd_bwd's own inputs at [1024] (7 heads, 1 KV head, head_dim 64): leak key i + 1 into row 900, and drop
    the (fragment 56 x key tile 3) product of dQ. What the leak moves, measured the way that test measures (gpu_util.check:
    rel-RMS and max-abs over the whole tensor, relative to the abs-max), stays several times below its bars (6e-3 / 3e-2), while
    the exact inputs change bits in every row (the two tests above). The dropped product is reported next to the backward
    bars (1.5e-2 / 6e-2)."""
    nH, nKV, hd, row = 7, 1, 64, 900
    M, ld, qkv, seg_s, seg_e = _attn_case([1024], nH, nKV, seed=1, hd=hd)
    d_o = rnd(M, nH * hd, seed=9).double()
    _, x = _attn_prescale(qkv, nH, hd)
    x = x.double()
    i = torch.arange(M)
    mask = i[None, :] <= i[:, None]
    leaky = mask.clone()
    leaky[row, row + 1] = True
    outs = {n: [] for n in ("o", "o leak", "dq", "dq drop")}
    for h in range(nH):
        q, k, v = x[:, h * hd:(h + 1) * hd] * hd ** -0.5, x[:, nH * hd:(nH + 1) * hd], x[:, (nH + 1) * hd:]
        o, dq = _gaussian_attention(q, k, v, d_o[:, h * hd:(h + 1) * hd], mask)
        outs["o"].append(o), outs["dq"].append(dq)
        outs["o leak"].append(_gaussian_attention(q, k, v, d_o[:, h * hd:(h + 1) * hd], leaky)[0])
        outs["dq drop"].append(_gaussian_attention(q, k, v, d_o[:, h * hd:(h + 1) * hd], mask, drop=(56, 3))[1])
    outs = {n: torch.cat(t, 1) for n, t in outs.items()}
    fig = {}
    for name, a, b in (("leak: o", outs["o leak"], outs["o"]), ("drop: dq", outs["dq drop"], outs["dq"])):
        fig[name] = (float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()), float((a - b).abs().max() / b.abs().max()))
        print(f"[attn-exact] gaussian [1024] {name}: rel-RMS change {fig[name][0]:.3e}, max-abs change / abs-max {fig[name][1]:.3e}")
    # the leak hides under the forward bars with room for the kernels' own rounding error (measured 3.8e-3 rel-RMS there);
    # the dropped product is only reported: at this depth it is of the order of the backward bars, neither safely seen nor safely missed
    assert fig["leak: o"][0] < 6e-3 / 4 and fig["leak: o"][1] < 3e-2 / 4


# ------------------------------------------------------------------------------------------------ schedule cases, buffers
@pytest.mark.parametrize("segments", list(R.SCHEDULE_SEGMENTS))
@pytest.mark.parametrize("profile", list(R.SCHEDULE_PROFILES))
def test_schedule_cases_reach_the_decision_points(profile, segments):
    """The deferred-max inputs are bf16 numbers with integer scores, and each profile does what its name says."""
    c = R.make_schedule_case(profile, segments)
    q, k, _ = R.split_heads(c)
    s = q[0] @ k[0].t()
    assert bool((s == s.round()).all()) and float(s.abs().max()) <= 512
    sigma = k[0][:, 0]
    tile_max = torch.stack([sigma[t * 64:(t + 1) * 64].max() for t in range(c.M // 64)])
    step = (tile_max[1:] - tile_max[:-1])[: 1024 // 64 - 2]   # inside the first segment
    if profile == "plus8_per_tile":
        assert bool((step == 8).all())
    if profile == "plus9_per_tile":
        assert bool((step == 9).all())
    if profile == "minus8_per_tile":
        assert bool((step == -8).all()) and float(sigma[0]) == 248
    if profile in ("low_then_high", "high_then_low"):
        first = -250.0 if profile == "low_then_high" else 250.0
        for s0 in sorted(set(c.seg_start.tolist())):
            assert float(sigma[s0]) == first and float(sigma[s0 + 69]) == first and float(sigma[s0 + 70]) == -first
    assert set(q[:, :, 0].unique().tolist()) == {-1.0, 1.0, 2.0}
    assert len({float(q[h, 32 + r, 0]) for h in range(1) for r in range(3)}) == 3   # neighbouring rows of a wave differ


def test_bands_and_poison():
    t, check = R.guarded((5, 8), torch.float32, "cpu")
    assert bool(torch.isnan(t).all())
    check("untouched")
    t.fill_(1.0)
    check("payload written")
    torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() + t.numel()).fill_(2.0)
    with pytest.raises(AssertionError, match="trailing guard band"):
        check("one element behind")
    p = R.poisoned(torch.ones(3, 4), torch.bfloat16, "cpu")
    assert bool((p == 1).all())
    assert bool(torch.isnan(torch.as_strided(p, (4,), (1,), storage_offset=p.storage_offset() + p.numel())).all())
    assert bool(torch.isnan(torch.as_strided(p, (4,), (1,), storage_offset=p.storage_offset() - 4)).all())
