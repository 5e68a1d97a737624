"""CPU tier of the optimizer's stochastic rounding ("adamw_sr"): the generator's known answers against the numpy restatement
the GPU tests compare the kernels with, the option's range, the export, and the trainer arguments (no GPU calls)."""
import numpy as np
import pytest

from slamkit_amd import engine as E
from tests import sr_ref as R

# Philox4x32-10 known answers (the Random123 distribution's kat_vectors: counter, key -> output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_restatement_reproduces_the_known_answers():
    for ctr, key, out in KAT:
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == out
    # vectorised over counters: the same words as one call per counter
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint64).T
    w = R.philox4x32_10(tuple(ctrs), KAT[0][1])
    assert tuple(int(x[0]) for x in w) == KAT[0][2]


def test_mapping_takes_the_halves_of_the_four_words_in_order():
    """Element j of a group of 8 takes bits (w[j >> 1] >> 16 (j & 1)) & 0xffff; counter = (i8 lo, i8 hi, step, which),
    key = (seed lo, seed hi)."""
    seed, step, which = 0x299f31d0a4093822, 0x13198a2e, 2
    i8 = (0x05a308d3 << 32) | 0x243f6a88  # both counter words in use; 8 * i8 still fits an int64 index
    w = [int(x) for x in R.philox4x32_10((i8 & R.MASK, i8 >> 32, step, which), (seed & R.MASK, seed >> 32))]
    got = R.sr_bits(seed, step, np.arange(8, dtype=np.uint64) + np.uint64(8 * i8), which)
    assert [int(g) for g in got] == [(w[j >> 1] >> (16 * (j & 1))) & 0xffff for j in range(8)]
    # a negative int64 seed is read as its 64 unsigned bits
    assert np.array_equal(R.sr_bits(-1, 1, np.arange(16), 0), R.sr_bits(0xffffffffffffffff, 1, np.arange(16), 0))


def test_rounding_restatement_on_values_with_known_results():
    x = np.array([0x3f800000, 0xbf800000, 0, 0x80000000, 0x3f808000, 0xbf808000, 0x7f800000, 0xff800000, 0x7f7e0001],
                 dtype=np.uint32).view(np.float32)  # 1, -1, 0, -0, +-(1 + 2^-8), +-inf, just above the bf16 value 0x7f7e
    lo, hi = np.zeros(x.size, dtype=np.uint32), np.full(x.size, 0xffff, dtype=np.uint32)
    # r = 0 truncates, r = 0xffff rounds every inexact value away from zero; exact values and infinities never move
    assert [hex(v) for v in R.sr_bf16(x, lo)] == ["0x3f80", "0xbf80", "0x0", "0x8000", "0x3f80", "0xbf80", "0x7f80", "0xff80", "0x7f7e"]
    assert [hex(v) for v in R.sr_bf16(x, hi)] == ["0x3f80", "0xbf80", "0x0", "0x8000", "0x3f81", "0xbf81", "0x7f80", "0xff80", "0x7f7f"]
    nan = R.sr_bf16(np.array([np.nan], dtype=np.float32), hi[:1])
    assert (int(nan[0]) & 0x7f80) == 0x7f80 and (int(nan[0]) & 0x7f) != 0


def test_option_range_and_export():
    lib = E.load_library()
    assert hasattr(lib, "slam_op_sr_round_bf16") and "slam_op_sr_round_bf16" in E.header_symbols()
    assert "slam_op_sr_round_bf16" in lib._slam_signatures
    eng = E.Engine(E.SlamModelDesc(2, 64, 4, 2, 64, 128, 502, 0, 1e-6, 10000.0))
    eng.set_option("adamw_sr", 1)
    eng.set_option("adamw_sr", 0)
    with pytest.raises(E.EngineError, match="out of range"):
        eng.set_option("adamw_sr", 2)
    with pytest.raises(E.EngineError, match="out of range"):
        eng.set_option("adamw_sr", -1)
    for seed in (0, 42, -7, 2 ** 63 - 1):
        eng.set_option("adamw_sr_seed", seed)
    eng.close()
    # an engine option: without an engine there is nothing to set
    assert lib.slam_set_option(None, b"adamw_sr", 1) == -1
    # bad arguments of the single-op entry are rejected before anything is launched
    assert lib.slam_op_sr_round_bf16(None, None, 8, 0, 0, 1, 0, None) == -1


def test_training_arguments_carry_the_fields():
    from slamkit_amd.trainer import SLAMTrainingArguments
    a = SLAMTrainingArguments()
    assert a.optim_stochastic_rounding is False and a.optim_sr_seed is None
    a = SLAMTrainingArguments(optim_state_dtype="bfloat16", optim_stochastic_rounding=True, seed=5)
    assert a.get_sr_seed() == 5
    a = SLAMTrainingArguments(optim_state_dtype="float32_bf16_moments", optim_stochastic_rounding=True, seed=5, optim_sr_seed=9)
    assert a.get_sr_seed() == 9


def test_recipe_config_names_the_field():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "slamkit_amd", "config", "training_args", "_recipe_common.yaml")).read()
    assert "optim_stochastic_rounding: false" in txt


def test_float32_state_with_stochastic_rounding_raises():
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    with pytest.raises(ValueError, match="optim_stochastic_rounding"):
        SLAMTrainingArguments(optim_stochastic_rounding=True)  # optim_state_dtype defaults to float32
    with pytest.raises(ValueError, match="optim_stochastic_rounding"):
        SLAMTrainingArguments(optim_state_dtype="float32", optim_stochastic_rounding=True)

    # and the trainer refuses the pair when the field was set after the arguments were built
    class _Eng:
        n_params = 8

    class _Model:
        device = "cpu"
        engine = _Eng()

    a = SLAMTrainingArguments()
    a.optim_stochastic_rounding = True
    with pytest.raises(ValueError, match="optim_stochastic_rounding"):
        SLAMTrainer(model=_Model(), args=a)
