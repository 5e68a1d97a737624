"""Host checks of tests/optim_exact_ref.py (no GPU): the float64 AdamW reference against torch.optim.AdamW itself, fp32
restatements of both expressions of adam_elem (separately rounded and fused) through the acceptance rule - 0 violations: DELTA_OPT
= 2^-20 is a property of the reference, not of the kernels -, the rule's power to reject seven seeded variants on data alone, and
the conditions the designed inputs must meet (profiles/optim_exact.md has the tables these tests print)."""
import numpy as np
import pytest
import torch

from tests import optim_exact_ref as X
from tests import row_exact_ref as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
N = 1 << 18
RANGES = [(lo, lo + w) for lo, w in zip(np.cumsum([0] + [4096, 192, 64, 8192, 256] * 20).tolist(), [4096, 192, 64, 8192, 256] * 20)]
RANGES.append((RANGES[-1][1], N))
assert RANGES[-1][1] > RANGES[-1][0] + 64 and all(lo % 8 == 0 for lo, _ in RANGES)
MODES = (0, 1, 2)
IDS = [f"set{i}" for i in range(len(X.HYPERS))]


def stored(x64, mode, k):
    """the float64 value -> what the kernel stores for array k in `mode` (one rounding)"""
    bf = mode == 2 if k == "p" else mode != 0
    return R.bf16_rne(x64) if bf else x64.to(F32)


@pytest.fixture(scope="module")
def designs():
    return {(mode, g16): X.design(RANGES, mode, g16) for mode in MODES for g16 in (False, True)}


def test_hyper_is_what_adam_hyper_computes():
    h = X.hyper(*X.HYPERS[2])
    assert h["bc1"] == 1.0 and h["bc2s"] == 1.0            # both corrections are 1.0f exactly at t = 100000
    h = X.hyper(*X.HYPERS[0])
    assert h["b1"] == float(np.float32(0.9)) and h["bc1"] == float(np.float32(1.0 - 0.9))   # from the double beta, not from f32(0.9)
    assert h["bc1"] != 1.0 - h["b1"]
    assert h["bc2s"] == float(np.float32(np.sqrt(1.0 - 0.999)))
    assert float(np.float32(1.0) - np.float32(h["b1"])) == 1.0 - h["b1"]      # 1.f - b1 is exact in fp32: the reference's (1 - b1)
    assert float(np.float32(1.0) - np.float32(h["b2"])) == 1.0 - h["b2"]


# ------------------------------------------------------------------------------------------------ generator conditions
@pytest.mark.parametrize("mode", MODES)
def test_designed_inputs_meet_their_conditions(designs, mode):
    for g16 in (False, True):
        d = designs[(mode, g16)]
        X.check_design(RANGES, d)
        for k in "pmv":
            assert torch.equal(stored(d[k], mode, k).double(), d[k]), f"{k} is not representable in its storage type"
        assert torch.equal((R.bf16_rne(d["g"]) if g16 else d["g"].to(F32)).double().nan_to_num(7.0), d["g"].nan_to_num(7.0))
    shares = torch.bincount(designs[(mode, False)]["cls"].long(), minlength=8).double() / N
    print("[optim-exact] class shares " + ", ".join(f"{c} {s:.3f}" for c, s in zip(X.CLASSES, shares.tolist())))


@pytest.mark.parametrize("hp", X.HYPERS, ids=IDS)
def test_reference_conditions_in_bf16_state(designs, hp):
    """Mode 2, both gradient types, both clips: at least half of the ordinary, eps-dominated and first-step elements - and of the
    four moving classes together - have bf16_rne(ref p') != p; so do the cancelling ones wherever the clip coefficient (0.37) or
    the betas (set 3) undo their cancellation (with m' ~ 0 and lr wd = 1e-5 a cancelling element cannot leave its bf16 value: that
    is what the class is for, and its m is where it shows); at most 5 % of the intervals hold two bf16 values; no non-zero
    reference below 2^-120 outside the underflow class."""
    h = X.hyper(*hp)
    for g16 in (False, True):
        d = designs[(2, g16)]
        for cs in X.CLIPS:
            ref = X.adam_ref(d["p"], d["m"], d["v"], d["g"], cs, h, lerp=True)
            X.check_reference(f"set {X.HYPERS.index(hp)} g16={int(g16)} clip {cs:.2f}", d, ref, cancel_moves=cs != 1.0 or hp[1] != .9)


# ------------------------------------------------------------------------------------------------ the proof behind DELTA_OPT
@pytest.mark.parametrize("hp", X.HYPERS, ids=IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_fp32_restatement_has_no_violations(designs, hp, fused):
    """adam_elem's two expressions in fp32 - every operation rounded separately, and every multiply-add contracted - through the
    rule on every class, set, state mode, gradient type and clip coefficient: 0 violations, and the worst |err| / S of the
    unrounded fp32 values in units of 2^-24 next to the 16 the rule allows."""
    h = X.hyper(*hp)
    worst = {}
    for mode in MODES:
        for g16 in (False, True):
            d = designs[(mode, g16)]
            for cs in X.CLIPS:
                ref = X.adam_ref(d["p"], d["m"], d["v"], d["g"], cs, h, lerp=mode == 2)
                out = X.adam_restated(d["p"], d["m"], d["v"], d["g"], cs, h, mode == 2, fused)
                for k, o in zip("pmv", out):
                    st = {}
                    tag = f"restated {k} mode {mode} g16 {int(g16)} clip {cs:.2f}"
                    assert X.accept(tag + " fp32", o.to(F32), *ref[k], d["cls"], stats=st) == 0, st.get("msg")
                    worst[(k, mode)] = max(worst.get((k, mode), 0.0), st["worst"])
                    if stored(o, mode, k).dtype == BF16:
                        assert X.accept(tag, stored(o, mode, k), *ref[k], d["cls"], stats=st) == 0, st.get("msg")
    print(f"[optim-exact] restatement ({'fused' if fused else 'separate'}) set {X.HYPERS.index(hp)}: worst |err|/S in 2^-24: "
          + ", ".join(f"{k} mode {m} {w:.2f}" for (k, m), w in sorted(worst.items())))
    assert max(worst.values()) <= 16.0


# ------------------------------------------------------------------------------------------------ reference == torch.optim.AdamW
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_reference_is_torch_adamw(wd):
    """Three consecutive steps of torch.optim.AdamW(foreach=False) on float64 CPU tensors against the reference with the same
    (unrounded) hyper-parameters, designed gradients (a new draw every step, the non-finite ones in the last), 1e-12 relative per element - relative to
    the element's sum of absolute terms S, which is |ref| wherever nothing cancels (torch's lerp and the reference's b1 m + (1 - b1) g
    differ by a few float64 roundoffs of S, which is 1e-12 of a moment that cancelled to 1e-4 of its terms); NaN where torch has NaN."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    ranges = [(0, 4096), (4096, 4096 + 192), (4288, 8192)]
    d = X.design(ranges, 0, False, seed=5)
    p = torch.nn.Parameter(d["p"].clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    rp, rm, rv = d["p"].clone(), torch.zeros_like(d["p"]), torch.zeros_like(d["p"])
    for t in (1, 2, 3):
        g = X.design(ranges, 0, False, seed=5 + t, nonfinite=t == 3)["g"]   # (inf - inf in torch's lerp is a matter of form, not of the step)
        p.grad = g.clone()
        opt.step()
        out = X.adam_ref(rp, rm, rv, g, 1.0, X.hyper_exact(lr, b1, b2, eps, wd, t), lerp=False)
        rp, rm, rv = out["p"][0], out["m"][0], out["v"][0]
        st = opt.state[p]
        for k, name, mine, theirs in (("p", "p", rp, p.detach()), ("m", "exp_avg", rm, st["exp_avg"]), ("v", "exp_avg_sq", rv, st["exp_avg_sq"])):
            assert torch.equal(torch.isnan(mine), torch.isnan(theirs)), f"step {t} {name}: NaN pattern"
            ok = torch.isfinite(theirs)
            assert torch.equal(mine[~ok].nan_to_num(7.0), theirs[~ok].nan_to_num(7.0)), f"step {t} {name}: inf pattern"
            err, S = (mine[ok] - theirs[ok]).abs(), out[k][1][ok]
            assert bool((err <= 1e-12 * S).all()), f"step {t} {name}: {float((err / S.clamp_min(1e-300)).max()):.3e}"
            assert float((err / theirs[ok].abs().clamp_min(1e-300)).median()) <= 1e-15
    assert int(torch.isnan(rp).sum()) >= 9      # the non-finite gradients reached the parameters in both


# ------------------------------------------------------------------------------------------------ sensitivity, on data alone
def test_rule_rejects_every_seeded_variant(designs):
    """Each variant of the reference arithmetic, rounded once to the storage type of the mode, through the rule: rejected in every
    state mode under at least one hyper-parameter set (clip 0.37: variant e needs one). Prints the count per (variant, mode, set)."""
    cs = X.CLIPS[1]
    rejected = {}
    for which in X.VARIANTS:
        for mode in MODES:
            d = designs[(mode, False)]
            keep = d["cls"] != X.NONF                       # the variants are arithmetic: the patterns of inf and NaN do not tell them apart
            row = []
            for hp in X.HYPERS:
                h = X.hyper(*hp)
                ref = X.adam_ref(d["p"], d["m"], d["v"], d["g"], cs, h, lerp=mode == 2)
                out = X.adam_variant(which, d["p"], d["m"], d["v"], d["g"], cs, h, hp)
                bad = 0
                for k, o in zip("pmv", out):
                    o = torch.where(keep, o, ref[k][0])
                    import contextlib
                    import io
                    with contextlib.redirect_stdout(io.StringIO()):
                        bad += X.accept(f"variant {which} {k}", stored(o, mode, k), *ref[k], d["cls"])
                row.append(bad)
            rejected[(which, mode)] = row
            print(f"[optim-exact] variant {which} mode {mode}: violations per set {row} of {3 * N}")
    for (which, mode), row in rejected.items():
        assert max(row) > 0, f"variant {which} passes the rule in mode {mode} under every set"
    # and the unchanged arithmetic passes: the rejections above are the variants', not the rounding's
    for mode in MODES:
        d = designs[(mode, False)]
        h = X.hyper(*X.HYPERS[3])
        ref = X.adam_ref(d["p"], d["m"], d["v"], d["g"], cs, h, lerp=mode == 2)
        for k in "pmv":
            assert X.accept(f"unchanged {k}", stored(ref[k][0], mode, k), *ref[k], d["cls"]) == 0


# ------------------------------------------------------------------------------------------------ helpers of the rule
def test_bf16_neighbours_and_clip_coefficient():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 0.0, 2.0 ** -140, -2.0 ** -140, 3.0], dtype=F64)
    lo, hi = X.bf16_floor(x).double(), X.bf16_ceil(x).double()
    assert lo.tolist() == [1.0, 1.0, -1.0 - 2.0 ** -7, 0.0, 0.0, -2.0 ** -133, 3.0]
    assert hi.tolist() == [1.0, 1.0 + 2.0 ** -7, -1.0, 0.0, 2.0 ** -133, 0.0, 3.0]
    assert X.clip_coef(np.float32(0.0), 1.0) == np.float32(1.0) and X.clip_coef(np.float32(5.0), 0.0) == np.float32(1.0)
    assert X.clip_coef(np.float32("inf"), 1.0) == np.float32(0.0) and np.isnan(X.clip_coef(np.float32("nan"), 1.0))
    assert X.clip_coef(np.float32(2.0), 1.0) == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6))
    assert X.ulp_apart(1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))) == 1
