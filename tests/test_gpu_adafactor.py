"""-m gpu: slam_adafactor_step (csrc/adafactor.hip) through the engine's entry points and the trainer under optim = "adafactor".
tests/adafactor_ref.py holds the float64 restatement, the synthetic segment table, the inputs and the per-element bound with its
derivation (tests/test_adafactor_host.py shows an fp32 emulation of the kernels' summation orders inside it with no violation);
nothing here widens it. Three consecutive steps (t = 1, where beta = 0, then 2 and 3) with fresh gradients and a clip coefficient
!= 1; every step is compared from the parameters the engine stored (u does not depend on p, so the state trajectory is the
restatement's own). Measured figures: profiles/adafactor.md."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import adafactor_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
G, GID = [False, True], ["g32", "g16"]
P, PID = [True, False], ["f32-master", "bf16-only"]


def ibits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class Body:
    """The 2-layer TINY model: an engine, its flat buffers, and - g16 - a real final = 2 backward behind it, so that the optimizer
    reads the bf16 gradient image."""

    def __init__(self, g16):
        from tests.test_gpu_model import _mk
        self.g16 = g16
        self.m = m = _mk(O.TINY, None, max_tokens=64)
        self.eng, self.n = m.engine, m.engine.n_params
        if g16:
            ids = torch.randint(2, O.TINY.vocab, (1, 64), generator=torch.Generator().manual_seed(1))
            ids[:, 0] = 1
            m.engine.set_option("grad_overwrite_next", 1)
            m(input_ids=ids, labels=ids, return_logits=False)
            m.backward(1.0, final=2)
            torch.cuda.synchronize()
            assert m.flat_grads16 is not None


_bodies = {}


def body(g16):
    if g16 not in _bodies:
        _bodies[g16] = Body(g16)
    return _bodies[g16]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    synthetic_run.cache_clear()
    _bodies.clear()
    torch.cuda.empty_cache()


def run_steps(b, table, p0, gs, master, lr, cs, wd, zero_grad=True, sr=False, seed=0, flags=None, first_step=1):
    """len(gs) consecutive steps over the body's flat buffers from p0 (float64 [<= n], NaN outside the table) -> per step the
    stored weights (float64 values and bits), the bf16 parameter bits and the state. Everything the table does not cover holds NaN
    before and must hold the same bits afterwards; so must the state and the workspace beyond their stated sizes."""
    m, eng, n = b.m, b.eng, b.n
    assert len(p0) <= n
    cov_np = np.zeros(n, dtype=bool)
    cov_np[:len(p0)] = A.covered(table, len(p0))
    cov = torch.from_numpy(cov_np).to(DEV)

    def guarded(x64, dtype):
        t = torch.full((n,), NAN, dtype=F64)
        t[:len(x64)] = torch.from_numpy(np.where(cov_np[:len(x64)], x64, np.nan))
        return t.to(dtype).to(DEV)
    n_state, ws_bytes = eng.adafactor_set_segments(table)
    assert n_state == A.state_offsets(table)[1]
    state = torch.full((n_state + 64,), NAN, dtype=F32, device=DEV)
    state[:n_state] = 0
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    eng.adafactor_bind_workspace(ws[:ws_bytes])
    eng.set_decay_mask(flags)
    eng.set_option("adamw_sr", int(sr))
    eng.set_option("adamw_sr_seed", seed)
    mt = guarded(p0, F32) if master else None
    m.flat_params.copy_(guarded(p0, BF16) if not master else torch.full((n,), NAN, dtype=BF16, device=DEV))
    norm_out = torch.tensor([3.0, cs], dtype=F32, device=DEV)
    out = {"p": [], "w_bits": [], "params_bits": [], "state": [], "cov": cov_np}
    try:
        for k, g in enumerate(gs):
            if b.g16:
                m.flat_grads16.copy_(guarded(g, BF16))
                m.flat_grads.fill_(NAN)           # an update that reads the wrong buffer shows
                g16_before = ibits(m.flat_grads16).clone()
            else:
                m.flat_grads.copy_(guarded(g, F32))
            g_before = ibits(m.flat_grads).clone()
            eng.adafactor_step(mt, state[:n_state], norm_out, lr, first_step + k, weight_decay=wd, zero_grad=zero_grad)
            torch.cuda.synchronize()
            w = mt if master else m.flat_params
            out["p"].append(w.double().cpu().numpy())
            out["w_bits"].append(ibits(w).cpu().numpy().copy())
            out["params_bits"].append(ibits(m.flat_params).cpu().numpy().copy())
            out["state"].append(state[:n_state].cpu().numpy().copy())
            # zero_grad clears the whole fp32 buffer, whichever buffer was read; without it nothing moves; the image never does
            if zero_grad:
                assert not bool(ibits(m.flat_grads).any())
            else:
                assert torch.equal(ibits(m.flat_grads), g_before)
            if b.g16:
                assert torch.equal(ibits(m.flat_grads16), g16_before)
            assert bool(torch.isnan(w[~cov]).all()) and bool(torch.isnan(m.flat_params[~cov]).all()), "an uncovered element was written"
            assert not bool(torch.isnan(w[cov]).any())
            assert bool(torch.isnan(state[n_state:]).all()) and bool((ws[ws_bytes:] == 0xA5).all()), "a write beyond a stated size"
            if master:    # the working copy is the round-to-nearest-even of the master the kernel stored
                assert torch.equal(ibits(m.flat_params)[cov], ibits(mt.to(BF16))[cov])
    finally:
        eng.set_option("adamw_sr", 0)
        eng.set_decay_mask(None)
        eng.adafactor_bind_workspace(None)
    return out


SYN = A.synthetic_table()


@functools.lru_cache(maxsize=None)
def synthetic_inputs():
    return A.synthetic_inputs(SYN[2], bf16_values=True)      # bf16-exact: the fp32 buffer and the bf16 image hold the same values


@functools.lru_cache(maxsize=None)
def synthetic_run(g16, master, zero_grad=True, rep=0):
    p0, gs = synthetic_inputs()
    return run_steps(body(g16), SYN[0], p0, gs, master, A.SYN_LR, A.SYN_CS, A.SYN_WD, zero_grad=zero_grad)


def check_against_restatement(tag, r, table, n, p0, gs, master, lr, cs, wd):
    """every step from the stored parameters, every covered element, at the derived bound -> the per-segment d of every step"""
    cov = r["cov"][:n]
    s64, prev, ds = np.zeros(A.state_offsets(table)[1]), p0, []
    for t, g in enumerate(gs):
        ref, s64, terms = A.step_f64(np.where(cov, prev, 0.0), g, s64, table, t + 1, lr, cs=cs, wd=wd, want_terms=True)
        bound, rel = A.bounds(table, t + 1, n, terms, ref)
        got = r["p"][t][:n]
        nbad = (A.violations_f32 if master else A.violations_bf16)(got, ref, bound, cov)
        err = np.abs(np.where(cov, got, 0.0) - np.where(cov, ref, 0.0))
        worst = float((err[cov] / bound[cov]).max())
        st = r["state"][t].astype(np.float64)
        st_worst = float((np.abs(st - s64) / (rel * np.abs(s64))).max())
        shown = f"worst |got - ref| / bound {worst:.3f}" if master else "bf16 stores held to the bf16 roundings of ref -+ bound"
        print(f"[adafactor] {tag} step {t + 1}: {shown}, state {st_worst:.3f}, violations {nbad}")
        assert nbad == 0, f"{tag} step {t + 1}: {nbad} elements outside the bound, worst ratio {worst}"
        assert st_worst <= 1.0, f"{tag} step {t + 1}: state outside its bound ({st_worst})"
        prev = got
        ds.append(terms[2])
    return ds


# =============================================================================================== (a) kernel vs float64
@pytest.mark.parametrize("g16", G, ids=GID)
@pytest.mark.parametrize("master", P, ids=PID)
def test_kernel_against_the_float64_restatement(g16, master):
    table, names, n, pad = SYN
    p0, gs = synthetic_inputs()
    r = synthetic_run(g16, master)
    assert not r["cov"][pad[0]:pad[1]].any() and r["cov"][pad[0] - 1]          # the pad rows of the 512-row slot kept their bits (run_steps)
    check_against_restatement(f"synthetic {GID[g16]} {PID[not master]}", r, table, n, p0, list(gs), master, A.SYN_LR, A.SYN_CS, A.SYN_WD)


# =============================================================================================== (b) determinism
@pytest.mark.parametrize("master", P, ids=PID)
def test_same_bits_every_run_either_buffer_either_zero_grad(master):
    base = synthetic_run(False, master)
    for other, what in ((synthetic_run(False, master, True, 1), "a second run"), (synthetic_run(False, master, False), "zero_grad = 0"),
                        (synthetic_run(True, master), "the bf16 gradient image")):
        for k in ("w_bits", "params_bits", "state"):
            for t in range(3):
                a, c = base[k][t], other[k][t]
                same = (a.view(np.int32) == c.view(np.int32)) if k == "state" else (a == c)
                assert bool(same.all()), f"{what}: {k} differs at step {t + 1} in {int((~same).sum())} elements"


# =============================================================================================== (c) decay mask
@pytest.mark.parametrize("master", P, ids=PID)
def test_decay_mask_per_engine_tensor(master):
    b = body(False)
    segs = b.m.hf_param_segments()
    table = [s.entry for s in segs]
    flags = b.m.hf_decay_flags()
    assert not all(flags) and any(flags)
    rng = np.random.default_rng(3)
    p0 = A.bf16_rne(0.05 * rng.standard_normal(b.n))
    g = A.bf16_rne(1e-2 * rng.standard_normal(b.n))
    kw = dict(master=master, lr=A.SYN_LR, cs=A.SYN_CS, first_step=2)
    masked = run_steps(b, table, p0, [g], wd=A.SYN_WD, flags=flags, **kw)
    plain = run_steps(b, table, p0, [g], wd=A.SYN_WD, **kw)
    zero = run_steps(b, table, p0, [g], wd=0.0, **kw)
    starts = sorted((t.offset, i) for i, t in enumerate(b.eng.tensors.values()))
    dec = np.zeros(b.n, dtype=bool)
    for s in segs:
        owner = [i for off, i in starts if off <= s.offset][-1]
        dec[A.seg_index(s.entry).reshape(-1)] = flags[owner]
    cov = masked["cov"]
    for k in ("w_bits", "params_bits"):
        assert np.array_equal(masked[k][0][cov & dec], plain[k][0][cov & dec]), k
        assert np.array_equal(masked[k][0][cov & ~dec], zero[k][0][cov & ~dec]), k
    # the decay shows where it applies (wd lr = 2^-9: a quarter to a half of a bf16 ulp, every fp32 value)
    assert (plain["w_bits"][0][cov & dec] != zero["w_bits"][0][cov & dec]).mean() > (0.9 if master else 0.05)
    assert np.array_equal(masked["state"][0].view(np.int32), plain["state"][0].view(np.int32))


# =============================================================================================== (d) per-segment update clip
def test_update_clip_is_per_segment():
    table, names, n, _ = SYN
    p0, gs = synthetic_inputs()
    up, down = A.seg_index(table[names.index("wide 96x2056")]), A.seg_index(table[names.index("tall 2050x8")])
    gs = [g.copy() for g in gs]
    for t in range(3):          # powers of two keep the values bf16-exact: one segment's gradients grow 16x a step, another's shrink
        gs[t][up] *= 16.0 ** t
        gs[t][down] *= 16.0 ** -t
    r = run_steps(body(False), table, p0, gs, True, A.SYN_LR, A.SYN_CS, A.SYN_WD)
    ds = check_against_restatement("clip", r, table, n, p0, gs, True, A.SYN_LR, A.SYN_CS, A.SYN_WD)
    iu, idn = names.index("wide 96x2056"), names.index("tall 2050x8")
    assert ds[1][iu] > 1.2 and ds[2][iu] > 1.2, ds          # RMS(u) > 1 (about 1 / sqrt(1 - beta)): the update is scaled down
    assert ds[1][idn] == 1.0 and ds[2][idn] == 1.0, ds      # RMS(u) < 1: it is not


# =============================================================================================== (e) adamw_sr
def test_stochastic_rounding_of_the_bf16_only_step():
    table, names, n, _ = SYN
    p0, gs = synthetic_inputs()       # bf16-representable parameters
    b = body(False)
    seed, step = 1234, 5
    kw = dict(lr=A.SYN_LR, cs=A.SYN_CS, wd=A.SYN_WD, first_step=step)
    ref = run_steps(b, table, p0, gs[:1], True, **kw)
    cov = ref["cov"]
    x = torch.from_numpy(ref["p"][0]).to(F32).to(DEV)       # the fp32-master step's result
    y = torch.empty(b.n, dtype=BF16, device=DEV)
    assert E.load_library().slam_op_sr_round_bf16(x.data_ptr(), y.data_ptr(), b.n, 0, seed, step, 0, E.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    want_sr, want_rne = ibits(y).cpu().numpy(), ibits(x.to(BF16)).cpu().numpy()
    on = run_steps(b, table, p0, gs[:1], False, sr=True, seed=seed, **kw)
    off = run_steps(b, table, p0, gs[:1], False, **kw)
    assert np.array_equal(on["w_bits"][0][cov], want_sr[cov]), int((on["w_bits"][0][cov] != want_sr[cov]).sum())
    assert np.array_equal(off["w_bits"][0][cov], want_rne[cov]), int((off["w_bits"][0][cov] != want_rne[cov]).sum())
    assert (want_sr[cov] != want_rne[cov]).mean() > 0.1                                    # the option changes something
    assert np.array_equal(on["state"][0].view(np.int32), ref["state"][0].view(np.int32))   # the fp32 state is never rounded
    with_master = run_steps(b, table, p0, gs[:1], True, sr=True, seed=seed, **kw)           # with a master the option does nothing
    assert np.array_equal(with_master["w_bits"][0], ref["w_bits"][0]) and np.array_equal(with_master["params_bits"][0][cov], ref["params_bits"][0][cov])


# =============================================================================================== refusals behind a valid table
def test_step_refusals_and_the_table_survives_rebinding():
    b = body(False)
    eng = b.eng
    n_state, ws_bytes = eng.adafactor_set_segments(SYN[0])
    state = torch.zeros(n_state, dtype=F32, device=DEV)
    norm = torch.tensor([1.0, 1.0], dtype=F32, device=DEV)
    before = ibits(b.m.flat_params).clone()
    with pytest.raises(E.EngineError, match="workspace"):
        eng.adafactor_step(None, state, norm, 1e-3, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(E.EngineError, match="too small"):
        eng.adafactor_bind_workspace(ws[:ws_bytes - 16])
    eng.adafactor_bind_workspace(ws)
    with pytest.raises(E.EngineError, match="state_f32"):
        eng.adafactor_step(None, None, norm, 1e-3, 1)
    with pytest.raises(E.EngineError, match="counts from 1"):
        eng.adafactor_step(None, state, norm, 1e-3, 0)
    eng.set_option("overlap_adamw", 1)
    try:
        with pytest.raises(E.EngineError, match="overlap_adamw"):
            eng.adafactor_step(None, state, norm, 1e-3, 1)
    finally:
        eng.set_option("overlap_adamw", 0)
    eng.bind_params(b.m.flat_params, b.m.flat_grads)      # re-binding keeps the table, like the decay mask
    assert eng.adafactor_sizes() == (n_state, ws_bytes)
    eng.adafactor_bind_workspace(None)
    torch.cuda.synchronize()
    assert torch.equal(ibits(b.m.flat_params), before) and not bool(state.any())   # a refused step launches nothing


# =============================================================================================== (f) against HF
class _Fam:
    def __init__(self, fam):
        from slamkit_amd.model import UnitLM, UnitLMConfig
        base, vocab = A.FAMILIES[fam]
        self.m = UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(base), vocab_size=vocab, max_tokens=64))
        self.eng, self.n, self.g16 = self.m.engine, self.m.engine.n_params, False


@pytest.mark.parametrize("fam", list(A.FAMILIES))
def test_against_hf_adafactor(fam):
    """The engine's fp32-master run of the fixture's three steps - HF's decay groups through slam_set_decay_mask - against HF's
    own float64 result, per HF tensor, at the accumulated bound; HF's float32 result beside it for information."""
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"adafactor_hf_{fam}.npz"))
    b = _Fam(fam)
    segs = b.m.hf_param_segments()
    names = [str(x) for x in fx["names"]]
    assert sorted(s.name for s in segs) == sorted(names)
    inputs = A.hf_inputs([(nm, tuple(fx[f"p64_{i}"].shape)) for i, nm in enumerate(names)])
    table, n = [s.entry for s in segs], b.n
    p0, gs, want, hf32 = np.zeros(n), [np.zeros(n) for _ in range(A.HF_STEPS)], np.zeros(n), np.zeros(n)
    for s in segs:
        idx, i = A.seg_index(s.entry), names.index(s.name)
        p0[idx], want[idx], hf32[idx] = inputs[s.name][0].reshape(idx.shape), fx[f"p64_{i}"].reshape(idx.shape), fx[f"p32_{i}"].reshape(idx.shape)
        for t in range(A.HF_STEPS):
            gs[t][idx] = inputs[s.name][1][t].reshape(idx.shape)
    decay = dict(zip(names, fx["decay"]))
    wd = [A.HF_WD if decay[s.name] else 0.0 for s in segs]
    r = run_steps(b, table, p0, gs, True, A.HF_LR, A.HF_CS, A.HF_WD, flags=b.m.hf_decay_flags())
    cov = r["cov"]
    p64, s64, total = p0.copy(), np.zeros(A.state_offsets(table)[1]), np.zeros(n)
    for t in range(A.HF_STEPS):
        p64, s64, terms = A.step_f64(p64, gs[t], s64, table, t + 1, A.HF_LR, cs=A.HF_CS, wd=wd, want_terms=True)
        total += A.bounds(table, t + 1, n, terms, p64)[0]
    got = r["p"][-1]
    for s in segs:
        idx = A.seg_index(s.entry).reshape(-1)
        err, e32 = np.abs(got[idx] - want[idx]), np.abs(hf32[idx] - want[idx])
        print(f"[adafactor] {fam} {s.name}: engine worst |err| / bound {float((err / total[idx]).max()):.3f}; HF float32 {float((e32 / total[idx]).max()):.3f}")
        assert bool((err <= total[idx]).all()), f"{s.name}: {int((err > total[idx]).sum())} elements outside the bound"
    assert A.violations_f32(got, want, total, cov) == 0


# =============================================================================================== (g) trainer
def _tiny_model(sd, max_tokens=1024):
    from tests.test_gpu_model import _mk
    return _mk(O.TINY, sd, max_tokens=max_tokens)


def test_trainer_loss_trajectory_vs_oracle_under_adafactor():
    """6 optimizer steps, GA 2, clip 0.5, cosine_with_min_lr under optim = "adafactor": the engine trainer against the oracle's
    forward_loss_grads with the restatement's update in the same loop; the loss within 2e-2 absolute at every step (the bar of
    test_trainer_loss_trajectory_vs_oracle). No exp_avg buffers exist."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments, lr_lambda
    cfg = O.TINY
    sd = O.init_weights(cfg, seed=5, bias_std=0.02, norm_jitter=0.05)
    g = torch.Generator().manual_seed(0)
    rows = []
    for i in range(24):
        k = int(torch.randint(20, 70, (1,), generator=g))
        ids = [1] + torch.randint(2, 502, (k,), generator=g).tolist() + [1]
        rows.append({"input_ids": ids, "attention_mask": [1] * len(ids)})
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)
    args = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=2, num_train_epochs=1, warmup_steps=2,
                                 warmup_ratio=0.0, learning_rate=2e-3, logging_steps=1, max_grad_norm=0.5, weight_decay=0.0,
                                 seed=7, output_dir="/tmp/unused", optim="adafactor")
    m = _tiny_model(sd)
    tr = SLAMTrainer(model=m, args=args, data_collator=coll, train_dataset=ds)
    assert tr.exp_avg is None and tr.exp_avg_sq is None
    n_state = sum(s.state_floats for s in m.hf_param_segments())
    assert tr.adafactor_state.numel() == n_state and n_state < m.engine.n_params // 50      # that is the point
    state = tr.train()
    eng_losses = [r["loss"] for r in state.log_history if "loss" in r]
    assert state.global_step == 6 and tr.opt_step == 6
    p = {k: v.double().numpy().copy() for k, v in sd.items()}
    st, batches, ref_losses = {}, tr._epoch_batches(0), []
    for step in range(6):
        micro = [coll([ds[i] for i in bb]) for bb in batches[2 * step: 2 * step + 2]]
        n_items = float(sum(int((mb["labels"] != -100).sum()) for mb in micro))
        tot = {k: torch.zeros_like(v) for k, v in sd.items()}
        loss_sum = 0.0
        pw = {k: torch.from_numpy(v).to(BF16).float() for k, v in p.items()}    # the engine computes with the bf16 copy
        for mb in micro:
            l, _, gr = O.forward_loss_grads(cfg, pw, mb["input_ids"], mb["labels"], num_items_in_batch=n_items)
            loss_sum += float(l)
            for k in tot:
                tot[k] += gr[k]
        ref_losses.append(loss_sum)
        _, coef = O.clip_coef(tot, 0.5)
        lr = args.learning_rate * lr_lambda(args, step, 6)
        A.named_step_f64(p, {k: v.double().numpy() for k, v in tot.items()}, st, step + 1, lr, cs=float(coef))
    print("engine", [round(x, 4) for x in eng_losses])
    print("oracle", [round(x, 4) for x in ref_losses])
    for a, c in zip(eng_losses, ref_losses):
        assert abs(a - c) <= 2e-2, (eng_losses, ref_losses)


def test_checkpoint_resume_under_adafactor(tmp_path):
    """Three steps + checkpoint + resume = the parameter bits of six uninterrupted steps; optimizer.pt holds the factors."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    sd = O.init_weights(O.TINY, seed=9)
    g = torch.Generator().manual_seed(1)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (40,), generator=g).tolist(), "attention_mask": [1] * 41} for _ in range(16)]
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)

    def run(max_steps, out, resume=None, save_steps=0, optim="adafactor"):
        m = _tiny_model(sd)
        a = SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=max_steps, warmup_steps=1, warmup_ratio=0.0, logging_steps=0,
                                  save_steps=save_steps, output_dir=str(out), num_train_epochs=4, optim=optim, weight_decay=0.01)
        tr = SLAMTrainer(model=m, args=a, data_collator=coll, train_dataset=ds)
        tr.train(resume_from_checkpoint=resume)
        return m, tr

    m_full, tr_full = run(6, tmp_path / "a", save_steps=3)
    ck = str(tmp_path / "a" / "checkpoint-3")
    st = torch.load(os.path.join(ck, "optimizer.pt"))
    assert st["optim"] == "adafactor" and st["opt_step"] == 3 and st["adafactor_state"].numel() == tr_full.adafactor_state.numel()
    m_res, tr2 = run(6, tmp_path / "b", resume=ck)
    assert tr2.state.global_step == 6 and tr2.opt_step == 6
    assert torch.equal(ibits(m_full.flat_params), ibits(m_res.flat_params)) and torch.equal(m_full._weights, m_res._weights)
    assert torch.equal(ibits(tr_full.adafactor_state), ibits(tr2.adafactor_state))
    with pytest.raises(ValueError, match="Adafactor checkpoint"):
        run(6, tmp_path / "c", resume=ck, optim="adamw_torch")


def test_dpo_step_under_adafactor():
    from slamkit_amd.tokeniser import UnitTokeniser
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer
    from tests.test_gpu_dpo import _model, _pairs
    pol = _model(O.init_weights(O.TINY, seed=11, bias_std=0.02), 16 * 256)
    ref = _model(O.init_weights(O.TINY, seed=12, bias_std=0.02), 16 * 256)
    before = pol._weights.clone()
    args = DPOConfig(per_device_train_batch_size=4, beta=0.1, logging_steps=1, max_steps=1, output_dir="/tmp/unused", learning_rate=5e-5,
                     warmup_steps=0, warmup_ratio=0.0, optim="adafactor")
    tr = SLAMDPOTrainer(model=pol, ref_model=ref, args=args, train_dataset=_pairs(4), processing_class=UnitTokeniser(None, load_fe=False))
    assert tr.exp_avg is None
    st = tr.train()
    torch.cuda.synchronize()
    assert st.global_step == 1 and tr.opt_step == 1
    assert bool(torch.isfinite(pol._weights).all()) and float((pol._weights != before).float().mean()) > 0.5
    assert float(tr.adafactor_state.abs().max()) > 0
