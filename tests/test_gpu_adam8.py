"""-m gpu: AdamW on 8-bit block-wise moments ("adamw_state8", adamw_q8_kernel) through slam_adamw_step_bf16 / _bf16_moments against
tests/adam8_ref.py: the float64 AdamW step from the dequantised stored state, then the header's fp32 quantiser. Body: the hidden-192
one of test_gpu_optim_exact (665,152 parameters: a short last block). Planted: an all-zero block (1), a block whose maximum is one
huge gradient so that every other code is 0 (2), step 1 from the zero state, step 2 from the stored codes.
  p       optim_exact_ref's rule and DELTA_OPT, from the dequantised state
  absmax  |got - max64| <= DELTA_OPT max(S) over the block (every m', v' is within DELTA_OPT S of its reference)
  codes   the reference's, or the neighbour's where the float64 y = |x| / max lies within DELTA_OPT (S + y S_max) / max + 2^-23 y of
          the midpoint between the two (the same bound carried through the division); at most 1 % of a case may use that. Observed
          on the CPU (adam_restated + the fp32 quantiser against this reference, these seeds, 384,192 elements): at most 1 element.
  bytes   every byte of an allocation that is neither a code nor a block maximum keeps its fill pattern"""
import numpy as np
import pytest
import torch

from tests import adam8_ref as A
from tests import optim_exact_ref as X
from tests import row_exact_ref as R
from tests.test_gpu_optim_exact import Body, same_bits

pytestmark = pytest.mark.gpu
DEV, FILL = "cuda", 0xA5
HP = [(1e-3, .9, .999, 1e-8, .1, 1), (1e-3, .9, .999, 1e-8, .1, 2)]   # step 1, step 2
_bodies = {}


def inputs(n, g16, seed):
    """p, g as float64; block 1 has zero gradients, block 2 one gradient of 1e4"""
    gen = torch.Generator().manual_seed(seed)
    p, g = 0.02 * torch.randn(n, generator=gen, dtype=torch.float64), 1e-2 * torch.randn(n, generator=gen, dtype=torch.float64)
    g[256:512] = 0.0
    g[512 + 7] = 1e4
    return p, X.store(g, g16)


def run(b, mode, g, hp, clip, flags, alloc, master, state8=1):
    (b.m.flat_grads16 if b.g16 else b.m.flat_grads).copy_(g)
    b.eng.set_decay_mask(flags)
    if state8 is not None:
        b.eng.set_option("adamw_state8", state8)
    norm_out = torch.tensor([3.0, clip], dtype=torch.float32, device=DEV)
    try:
        if mode == 2:
            b.eng.adamw_step_bf16(alloc[0], alloc[1], norm_out, *hp, zero_grad=False)
        else:
            b.eng.adamw_step(master, alloc[0], alloc[1], norm_out, *hp, zero_grad=False)
        torch.cuda.synchronize()
    finally:
        b.eng.set_decay_mask(None)
        if state8 is not None:
            b.eng.set_option("adamw_state8", 0)


def body(g16):
    """the body, and - before the option is ever set on its engine - the bits of one bf16-moment step (`never`)"""
    if g16 not in _bodies:
        b = _bodies[g16] = Body("b192", g16)
        assert b.n % 256 != 0 and b.n % 8 == 0
        p, g = inputs(b.n, g16, 7)
        b.m.flat_params.copy_(p)
        b.never = [torch.zeros(b.n, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        run(b, 2, g, HP[0], 0.5, None, b.never, None, state8=None)
        b.never.append(b.m.flat_params.clone())
    return _bodies[g16]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _bodies.clear()
    torch.cuda.empty_cache()


def check_moment(tag, alloc, n, ref, S, signed):
    codes, amax, rest = A.split(alloc.cpu().numpy(), n)
    assert (rest == FILL).all(), f"{tag}: a byte outside codes[n] and absmax[blocks] changed"
    ref, S, K = ref.cpu().numpy(), S.cpu().numpy(), 127 if signed else 255
    max64, smax = A.block_max(ref), A.block_max(S)
    assert (np.abs(amax.astype(np.float64) - max64) <= X.DELTA_OPT * smax).all(), f"{tag}: absmax"
    want, _ = A.quantise(ref.astype(np.float32), signed)
    k, kw, diff = codes.astype(np.int64) & K, want.astype(np.int64) & K, codes != want
    max64, smax = (np.repeat(x, A.BLOCK)[:n] for x in (max64, smax))
    with np.errstate(all="ignore"):
        y = np.where(max64 > 0, np.abs(ref) / max64, 0.0)
        tol = X.DELTA_OPT * (S + y * smax) / max64 + 2.0 ** -23 * y
    lo = np.minimum(k, kw)
    near = (np.abs(k - kw) == 1) & (np.abs(y - A.midpoints(A.table(signed)).astype(np.float64)[lo.clip(max=K - 1)]) <= tol)
    near &= (lo == 0) | ((codes & (255 - K)) == (want & (255 - K)))   # the same sign, unless one of the two is the unsigned code 0
    print(f"[adam8] {tag}: {int(diff.sum())} of {n} codes are the neighbour's")
    assert not (diff & ~near).any(), f"{tag}: {int((diff & ~near).sum())} codes differ, first at {int((diff & ~near).nonzero()[0][0])}"
    assert diff.mean() <= 0.01, (tag, diff.mean())
    return int((codes[256:512] != 0).sum()), int((codes[512:768] != 0).sum())


@pytest.mark.parametrize("masked", [False, True], ids=["decay-all", "decay-mask"])
@pytest.mark.parametrize("clip", [1.0, X.CLIPS[1]], ids=["clip1", "clip.37"])
@pytest.mark.parametrize("g16", [False, True], ids=["g32", "g16"])
@pytest.mark.parametrize("mode", [1, 2], ids=["master", "bf16"])
def test_two_steps_against_the_reference(mode, g16, clip, masked):
    b = body(g16)
    n, m = b.n, b.m
    flags = [i % 2 == 0 for i in range(len(b.layout.names))] if masked else None
    alloc = [torch.full((A.layout(n)[0],), FILL, dtype=torch.uint8, device=DEV) for _ in range(2)]
    for a in alloc:   # the zero state: codes and maxima 0
        a[:n] = 0
        a[A.layout(n)[1]:] = 0
    p0, _ = inputs(n, g16, 11)
    master = p0.float().to(DEV) if mode == 1 else None
    m.flat_params.copy_(p0)
    for t, hp in enumerate(HP):
        tag = f"mode {mode} {'g16' if g16 else 'g32'} clip {clip} {'masked' if masked else 'all'} step {t + 1}"
        g, h = inputs(n, g16, 20 + t)[1].to(DEV), X.hyper(*hp)
        mv = [torch.from_numpy(A.dequantise(*A.split(a.cpu().numpy(), n)[:2], signed=s)).double().to(DEV) for a, s in zip(alloc, (True, False))]
        ref = X.adam_ref((master if mode == 1 else m.flat_params).double(), mv[0], mv[1], g, clip, h, lerp=mode == 2,
                         wd=b.wd_elements(flags, h["wd"]) if masked else None)
        run(b, mode, g, hp, clip, flags, alloc, master)
        X.check(f"{tag} p", master if mode == 1 else m.flat_params, *ref["p"], torch.zeros(n, dtype=torch.int8), None, "flat")
        if mode == 1:
            same_bits(f"{tag}: working copy vs RNE(master)", m.flat_params, R.bf16_rne(master.double()))
        lo, hi, cols = next((lo, hi, c) for lo, hi, c in zip(b.layout.lo, b.layout.hi, b.layout.cols) if c > 1 and lo > 0)
        same_bits(f"{tag}: a transposed image", m.flat_params_t[lo:hi].view(cols, -1).t().contiguous(), m.flat_params[lo:hi].view(-1, cols))
        nz = [check_moment(f"{tag} {k}", a, n, *ref[k], signed=s) for k, a, s in (("m", alloc[0], True), ("v", alloc[1], False))]
        assert nz[0][0] == 0 and nz[1][0] == 0, "the all-zero block stored a code"
        assert t or (nz[0][1] == 1 and nz[1][1] == 1), "the block of the huge gradient keeps one non-zero code"


@pytest.mark.parametrize("g16", [False, True], ids=["g32", "g16"])
def test_option_off_is_the_run_that_never_set_it_and_ranges_are_refused(g16):
    from slamkit_amd.engine import EngineError
    b = body(g16)
    p, g = inputs(b.n, g16, 7)
    b.m.flat_params.copy_(p)
    mv = [torch.zeros(b.n, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    b.eng.set_option("adamw_state8", 1)
    for bad in (2, -1):
        with pytest.raises(EngineError, match="out of range"):
            b.eng.set_option("adamw_state8", bad)
    for master in (None, torch.zeros(b.n, device=DEV)):
        with pytest.raises(EngineError, match=r"\(-1\).*state block"):
            b.eng.adamw_range(0, 256, master, mv[0], mv[1], None, *HP[0])
    run(b, 2, g, HP[0], 0.5, None, mv, None, state8=0)
    for name, x, y in zip(("m", "v", "p"), mv + [b.m.flat_params], b.never):
        same_bits(f"option back at 0: {name}", x, y)


def test_trainer_checkpoint_round_trip(tmp_path):
    """4 steps + checkpoint + resume to 6 = the parameter and code bits of 6 uninterrupted steps; resuming under AdamW raises."""
    from oracle import slam_oracle as O
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_gpu_adafactor import _tiny_model
    sd, gen = O.init_weights(O.TINY, seed=9), torch.Generator().manual_seed(1)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (40,), generator=gen).tolist(), "attention_mask": [1] * 41} for _ in range(16)]
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)

    def train(out, resume=None, optim="adamw_bnb_8bit"):
        a = SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=6, warmup_steps=1, warmup_ratio=0.0, logging_steps=0, save_steps=4,
                                  output_dir=str(out), num_train_epochs=4, optim=optim, optim_state_dtype="bfloat16", weight_decay=0.01)
        tr = SLAMTrainer(model=_tiny_model(sd), args=a, data_collator=coll, train_dataset=ds)
        tr.train(resume_from_checkpoint=resume)
        return tr

    full = train(tmp_path / "a")
    ck, n = str(tmp_path / "a" / "checkpoint-4"), full.model.engine.n_params
    st = torch.load(ck + "/optimizer.pt")
    assert st["optim"] == "adamw_8bit" and st["opt_step"] == 4 and st["exp_avg_codes"].numel() == n and st["exp_avg_sq_absmax"].numel() == -(-n // 256)
    assert full.optimizer.state_bytes == (2 * A.layout(n)[0], 0) and int(st["exp_avg_sq_codes"].count_nonzero()) > n // 2
    res = train(tmp_path / "b", resume=ck)
    assert res.opt_step == 6 and all(torch.equal(x, y) for x, y in zip(full.optimizer._alloc, res.optimizer._alloc))
    same_bits("parameters", full.model.flat_params, res.model.flat_params)
    with pytest.raises(ValueError, match="8-bit AdamW checkpoint"):
        train(tmp_path / "c", resume=ck, optim="adamw_torch")
