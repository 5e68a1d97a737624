"""The 8-bit Adam moment format without a GPU: tests/adam8_ref.py on hand-made values, the size formula, the names and refusals."""
import numpy as np
import pytest

from tests import adam8_ref as A


def test_tables_and_the_quantiser_on_hand_made_values():
    tm, tv = A.table(True), A.table(False)
    assert tm.dtype == tv.dtype == np.float32 and tm.size == 128 and tv.size == 256
    assert tm[0] == tv[0] == 0 and tm[127] == tv[255] == 1 and tm[119] == tv[247] == 0.5 and tm[1] == np.float32(2.0 ** -15.75)
    assert tv[1] == np.float32(2.0 ** -31.75) and (np.diff(tm) > 0).all() and (np.diff(tv) > 0).all()
    x = np.zeros(3 * 256 - 60, dtype=np.float32)               # block 0: table hits and midpoints; 1: zeros; 2: short, one value
    mid = A.midpoints(tm)
    x[:8] = [4.0, -4.0 * tm[100], 4.0 * mid[100], -4.0 * mid[100], 4.0 * np.nextafter(mid[100], np.float32(1)), 4.0 * mid[0], 4.0 * tm[1], -0.0]
    x[700] = -3.0
    c, amax = A.quantise(x, True)
    assert list(c[:8]) == [127, 128 + 100, 100, 128 + 100, 101, 0, 1, 0] and list(amax) == [4.0, 0.0, 3.0]   # ties go down; k = 0 has no sign
    assert not c[8:700].any() and c[700] == 255 and c.size == x.size
    back = A.dequantise(c, amax, True)
    assert list(back[:3]) == [4.0, -4.0 * tm[100], 4.0 * tm[100]] and back[700] == -3.0 and not back[256:512].any()
    cv, av = A.quantise(np.array([9.0, 9.0 * tv[77], 9.0 * A.midpoints(tv)[254], 0.0], dtype=np.float32), False)
    assert list(cv) == [255, 77, 254, 0] and list(av) == [9.0]
    assert list(A.dequantise(cv, av, False)) == [9.0, np.float32(9.0) * tv[77], np.float32(9.0) * tv[254], 0.0]


@pytest.mark.parametrize("n", [8, 256, 264, 1000, 358_000_008])
def test_size_formula(n):
    from slamkit_amd.engine import Engine
    size, off, blocks = Engine.adam8_state_layout(n)
    assert (size, off, blocks) == A.layout(n) and off % 256 == 0 and off >= n and blocks == -(-n // 256) and size == off + 4 * blocks


def test_optim_names_and_refusals():
    from slamkit_amd.trainer import SLAMTrainingArguments
    from slamkit_amd.trainer.optimizers import BY_OPTION, KINDS
    from tests.test_trainer_optimizers_host import _stub_trainer
    assert SLAMTrainingArguments(optim="adamw_bnb_8bit").optim == "adamw_bnb_8bit" and BY_OPTION["adamw_bnb_8bit"] is KINDS["adamw_8bit"]
    with pytest.raises(ValueError, match="optim must be"):       # HF's other spelling: tests/test_adafactor_host.py keeps it refused
        SLAMTrainingArguments(optim="adamw_8bit")
    for kw, why in ((dict(optim_state_dtype="float32"), "8 bits.*not float32"), (dict(optim_state_dtype="bfloat16", ddp_algo="rs_ag"), "256-element blocks.*rs_ag"),
                    (dict(optim_state_dtype="bfloat16", overlap_optimizer=True), "overlap_optimizer")):
        with pytest.raises(ValueError, match=why):
            _stub_trainer(optim="adamw_bnb_8bit", **kw)
    tr, model = _stub_trainer(optim="adamw_bnb_8bit", optim_state_dtype="float32_bf16_moments")
    n = model.engine.n_params
    assert tr.optimizer.state_bytes == (2 * A.layout(n)[0], 0) and [t.numel() for t in tr.optimizer.state.values()] == [n, -(-n // 256)] * 2
