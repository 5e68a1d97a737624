"""CPU tier of padding-free execution (SLAMTrainingArguments.padding_free, UnitLM.padding_free, slam_forward_unpadded): the pack
rule's numpy restatement, the argument / YAML / trainer plumbing, and the ABI surface - declared, exported, bound, and refusing
bad arguments and bad call order before anything touches a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from slamkit_amd import engine as E
from tests import unpad_ref as R

NEW_SYMBOLS = ("slam_unpadded_scratch_bytes", "slam_forward_unpadded", "slam_last_forward_tokens", "slam_seq_loglik_unpadded",
               "slam_scale_loss_unpadded", "slam_op_unpad_pack")


def test_unpad_ref_pack_rule():
    R.test_pack_rule()


def test_unpad_ref_matches_the_flattening_collator():
    """The pack rule is DataCollatorWithFlattening's layout: same ids, labels and positions for the same rows."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, DataCollatorWithFlattening
    g = torch.Generator().manual_seed(0)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (n,), generator=g).tolist(), "attention_mask": [1] * (n + 1)}
            for n in (30, 7, 63, 1)]
    pad = DataCollatorForLanguageModeling(pad_token_id=0)(rows)
    flat = DataCollatorWithFlattening()(rows)
    lens = pad["attention_mask"].sum(1).numpy()
    p = R.pack(pad["input_ids"].numpy(), pad["labels"].numpy(), lens)
    S = int(lens.sum())
    assert p["ids"][:S].tolist() == flat["input_ids"][0].tolist()
    assert p["labels"][:S].tolist() == flat["labels"][0].tolist()
    assert p["position_ids"][:S].tolist() == flat["position_ids"][0].tolist()
    assert len(p["ids"]) == 128 and S == 105


def test_symbols_declared_exported_and_bound():
    lib = E.load_library()
    names = E.header_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(lib, n) and n in lib._slam_signatures, n


@pytest.mark.parametrize("B,T", [(1, 1), (1, 37), (2, 37), (3, 64), (8, 1024), (257, 65)])
def test_scratch_bytes_and_views(B, T):
    mm = -(-(B * T) // 64) * 64
    n = E.unpadded_scratch_bytes(B, T)
    assert n == mm * (3 * 8 + 3 * 4) + -(-(4 * (B + 1)) // 256) * 256 and n % 256 == 0
    v = E.unpadded_scratch_views(torch.zeros(n, dtype=torch.uint8), B, T)
    assert [k for k in v] == ["ids", "labels", "position_ids", "seg_start", "seg_end", "row", "off"]
    assert all(v[k].numel() == mm for k in list(v)[:6]) and v["off"].numel() == B + 1
    assert v["off"].data_ptr() + 4 * (B + 1) <= v["ids"].data_ptr() + n
    assert E.unpadded_scratch_bytes(0, 4) == 0 and E.unpadded_scratch_bytes(4, -1) == 0


def test_entry_points_refuse_bad_arguments_and_call_order():
    """Nothing here reaches a device: every refusal happens on the host."""
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(2, 256, 4, 2, 64, 512, 502, 0, 1e-6, 10000.0))
    one = C.c_void_p(256)  # a non-null, 256-byte aligned address that is never dereferenced
    sb = E.unpadded_scratch_bytes(2, 64)
    # the pack op alone
    assert lib.slam_op_unpad_pack(None, None, one, 2, 64, 128, 0, one, sb, None) == -1
    assert lib.slam_op_unpad_pack(one, None, one, 2, 64, 100, 0, one, sb, None) == -1      # not a multiple of 64
    assert lib.slam_op_unpad_pack(one, None, one, 2, 64, 192, 0, one, sb, None) == -1      # beyond B * T
    assert lib.slam_op_unpad_pack(one, None, one, 2, 64, 128, 0, one, sb - 1, None) == -1  # scratch too small
    assert lib.slam_op_unpad_pack(one, None, one, 2, 64, 128, 0, C.c_void_p(264), sb, None) == -1  # misaligned
    # the forward: arguments first, then state (nothing bound)
    f = lib.slam_forward_unpadded
    assert f(eng.h, one, None, one, 2, 64, 96, one, sb, 0.0, None, None, None) == -1
    assert f(eng.h, one, None, one, 2, 64, 0, one, sb, 0.0, None, None, None) == -1
    assert f(eng.h, one, None, None, 2, 64, 128, one, sb, 0.0, None, None, None) == -1
    assert f(eng.h, one, None, one, 2, 64, 128, one, sb, 0.0, None, None, None) == -2      # no params / workspace bound
    assert b"bind params" in lib.slam_last_error(eng.h)
    assert f(None, one, None, one, 2, 64, 128, one, sb, 0.0, None, None, None) == -1
    # the per-row calls without an unpadded forward
    assert lib.slam_seq_loglik_unpadded(eng.h, 2, one, one, None) == -2
    assert lib.slam_scale_loss_unpadded(eng.h, one, 2, None) == -2
    assert lib.slam_seq_loglik_unpadded(eng.h, 2, None, one, None) == -1
    assert lib.slam_last_forward_tokens(eng.h) == 0 and lib.slam_last_forward_tokens(None) == 0
    with pytest.raises(E.EngineError, match="unpadded forward"):
        eng.seq_loglik_unpadded(2, torch.zeros(2), torch.zeros(2), stream=0)
    eng.close()


def test_arguments_and_yaml_carry_the_option():
    from slamkit_amd.trainer import DPOConfig, SLAMTrainingArguments
    from slamkit_amd.utils.config import CONFIG_DIR, load_config, to_container
    assert SLAMTrainingArguments().padding_free is False and DPOConfig().padding_free is False
    assert SLAMTrainingArguments(padding_free=True).padding_free is True
    assert "padding_free: false" in open(os.path.join(CONFIG_DIR, "training_args", "_recipe_common.yaml")).read()
    for top in ("train", "train_inter_scale", "preference_alignment_train"):
        assert to_container(load_config(top).training_args)["padding_free"] is False, top
    on = load_config("train", ["training_args.padding_free=true"]).training_args
    assert to_container(on)["padding_free"] is True


def test_host_lengths():
    from slamkit_amd.model import UnitLM
    am = torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0], [1, 1, 1, 1]])
    assert UnitLM._host_lengths(3, 4, am, None).tolist() == [3, 1, 4]
    assert UnitLM._host_lengths(3, 4, None, [2, 4, 1]).tolist() == [2, 4, 1]
    assert UnitLM._host_lengths(3, 4, am, torch.tensor([1, 1, 1])).tolist() == [1, 1, 1]  # explicit lengths win
    assert UnitLM._host_lengths(3, 4, None, None) is None
    for bad in ([0, 1, 1], [1, 1, 5], [1, 1]):
        with pytest.raises(ValueError, match="row lengths"):
            UnitLM._host_lengths(3, 4, None, bad)
    with pytest.raises(ValueError, match="row lengths"):
        UnitLM._host_lengths(1, 4, torch.zeros(1, 4, dtype=torch.long), None)  # an empty row


def _recorder():
    from tests.test_trainer_dp_gloo import StubLM

    class Rec(StubLM):
        padding_free = False  # what the trainer switches on

        def __init__(self):
            super().__init__()
            self.masks = []

        def forward(self, attention_mask=None, **kw):
            self.masks.append(attention_mask is not None)
            return super().forward(**kw)

    return Rec()


@pytest.mark.parametrize("on", [False, True])
def test_trainer_sets_the_model_switch_for_training_and_evaluation(tmp_path, on):
    from slamkit_amd.data import DataCollatorForLanguageModeling
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_trainer_dp_gloo import StubLM, make_rows
    m = _recorder()
    args = SLAMTrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=2, learning_rate=1e-2, warmup_steps=1,
                                 warmup_ratio=0.0, max_steps=2, logging_steps=0, save_steps=0, padding_free=on,
                                 per_device_eval_batch_size=2)
    tr = SLAMTrainer(model=m, args=args, data_collator=DataCollatorForLanguageModeling(pad_token_id=0),
                     train_dataset=make_rows(), eval_dataset=make_rows(6, seed=9))
    assert m.padding_free is on
    tr.train()
    assert m.masks == [True, True]  # training steps always hand the collated mask over
    m.masks.clear()
    tr.evaluate()
    assert m.masks == [on] * 3      # evaluate() hands it over only to a padding-free model
    # the default False never switches a model off that its owner switched on
    keep = _recorder()
    keep.padding_free = True
    SLAMTrainer(model=keep, args=SLAMTrainingArguments(output_dir=str(tmp_path), logging_steps=0),
                data_collator=DataCollatorForLanguageModeling(pad_token_id=0), train_dataset=make_rows())
    assert keep.padding_free is True
    # a model without the switch (other TokenLM implementations) is left alone
    plain = StubLM()
    SLAMTrainer(model=plain, args=args, data_collator=DataCollatorForLanguageModeling(pad_token_id=0), train_dataset=make_rows())
    assert not hasattr(plain, "padding_free")


def test_dpo_collator_carries_row_lengths():
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer
    rows = [{"prompt_input_ids": [1, 5, 6], "chosen_input_ids": [7, 8, 1], "rejected_input_ids": [9, 1]},
            {"prompt_input_ids": [1, 5], "chosen_input_ids": [7] * 70 + [1], "rejected_input_ids": [9, 9, 1]}]

    class T(SLAMDPOTrainer):
        def __init__(self):  # the collator needs only these two
            self.args, self.pad_id = DPOConfig(), 0

    mb = T()._collate_pairs(rows)
    assert mb["input_ids"].shape == (4, 128) and mb["lengths"].tolist() == [6, 73, 5, 5] and mb["lengths"].dtype == torch.int32
    assert ((mb["input_ids"] != 0).sum(1) == mb["lengths"]).all()
    on, off = type("M", (), {"padding_free": True})(), type("M", (), {"padding_free": False})()
    assert SLAMDPOTrainer._lengths_kw(on, mb) == {"lengths": mb["lengths"]}
    assert SLAMDPOTrainer._lengths_kw(off, mb) == {} and SLAMDPOTrainer._lengths_kw(object(), mb) == {}
