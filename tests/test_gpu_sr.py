"""-m gpu: stochastic rounding of the bf16 optimizer state ("adamw_sr", SLAMTrainingArguments.optim_stochastic_rounding).

The rounding and its random bits against the numpy restatement (tests/sr_ref.py) bit for bit; unbiasedness within a binomial
bound; the constant-gradient case in which round-to-nearest never moves a weight; one bit pattern from every kernel form;
seeding; a trainer run tracked against the fp32-master run; resume."""
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import sr_ref as R
from tests.gpu_util import lib, ptr, stream

pytestmark = pytest.mark.gpu


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _sr_round(x: torch.Tensor, seed: int, step: int, index0: int, which: int) -> np.ndarray:
    y = torch.empty(x.numel(), dtype=torch.bfloat16, device="cuda")
    assert lib().slam_op_sr_round_bf16(ptr(x), ptr(y), x.numel(), index0, seed, step, which, stream()) == 0
    torch.cuda.synchronize()
    return _bits(y)


def _tiny_model(sd, max_tokens=1024):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    cfg = O.TINY
    base = dict(num_hidden_layers=cfg.n_layers, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads,
                num_key_value_heads=cfg.n_kv_heads, head_dim=cfg.head_dim, intermediate_size=cfg.intermediate,
                rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, tie_word_embeddings=True)
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=max_tokens))
    m.load_state_dict(sd)
    return m


def _trainer(m, osd, sr, seed=7, **kw):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    kw.setdefault("logging_steps", 0)
    return SLAMTrainer(model=m, args=SLAMTrainingArguments(optim_state_dtype=osd, optim_stochastic_rounding=sr, optim_sr_seed=seed, **kw))


# ---- 1. the rounding, bit for bit ---------------------------------------------------------------------------------------------
def _known_answer_inputs():
    g = np.random.default_rng(0)
    n = 2 ** 20
    x = (g.standard_normal(n) * np.exp2(g.integers(-60, 60, n))).astype(np.float32)       # many binades
    exact = (g.standard_normal(4096).astype(np.float32).view(np.uint32) & 0xffff0000).view(np.float32)  # bf16 values
    special = np.array([0x00000000, 0x80000000,                                     # +-0
                        0x00000001, 0x007fffff, 0x80000001, 0x00012345, 0x807f8001,   # denormals
                        0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0x7f7f0001,               # the largest finite values
                        0x7f800000, 0xff800000,                                     # +-inf
                        0x7fc00000, 0xffc00001, 0x7f800001],                         # NaN
                       dtype=np.uint32).view(np.float32)
    x = np.concatenate([x, exact, special, np.zeros(5, dtype=np.float32)])          # (a length that is no multiple of 8)
    return x, np.arange(n, n + 4096)


@pytest.mark.parametrize("seed,step,index0,which", [(0x0123456789abcdef, 7, 0, 0), (-5, 1000003, 2 ** 33 + 24 + 3, 2)])
def test_rounding_matches_the_restatement_bit_for_bit(seed, step, index0, which):
    """slam_op_sr_round_bf16 over 2^20 fp32 values of many binades plus +-0, denormals, exact bf16 values, the largest finite
    value and +-inf: equal, as int16, to the numpy restatement of the mapping and of sr_bf16 (NaN: NaN-ness only). The second
    setting has a negative seed, an index beyond 2^32 (the counter's second word) that is no multiple of 8, and another array."""
    x, exact_at = _known_answer_inputs()
    assert x.size >= 2 ** 20
    got = _sr_round(torch.from_numpy(x).cuda(), seed, step, index0, which)
    want = R.sr_round(x, seed, step, index0, which)
    nan = np.isnan(x)
    assert nan.sum() == 3
    assert np.array_equal(got[~nan], want[~nan]), int((got[~nan] != want[~nan]).sum())
    assert np.all((got[nan] & 0x7f80) == 0x7f80) and np.all((got[nan] & 0x7f) != 0)
    # representable inputs come back unchanged
    assert np.array_equal(got[exact_at], (x[exact_at].view(np.uint32) >> 16).astype(np.uint16))
    fin = np.isfinite(x)
    rtn = R.rtn_bf16_bits(x)
    changed = got[fin] != rtn[fin]
    print(f"[parity] sr_round seed {seed} step {step}: {int(changed.sum())} of {int(fin.sum())} finite values differ from "
          f"round-to-nearest (expected about a quarter)")
    assert np.all(np.abs(got[fin].astype(np.int32) - rtn[fin].astype(np.int32)) <= 1)  # the nearest value or its neighbour


# ---- 2. unbiased ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0.1, 0.5, 0.9])
def test_share_rounded_up_is_the_discarded_fraction(f):
    """x = 1 + f 2^-7 lies the fraction f of the way from the bf16 value 1 to the next one: over N = 2^22 distinct indices the
    share rounded up is f within 6 sqrt(f (1 - f) / N) - six standard deviations of the binomial share (derived, not measured;
    the fp32 rounding of x itself moves f by at most 2^-17)."""
    n = 2 ** 22
    x = torch.full((n,), float(np.float32(1.0 + f * 2.0 ** -7)), dtype=torch.float32, device="cuda")
    got = _sr_round(x, 42, 1, 0, 0)
    assert set(np.unique(got).tolist()) <= {0x3f80, 0x3f81}
    share = float((got == 0x3f81).mean())
    bound = 6.0 * (f * (1.0 - f) / n) ** 0.5
    print(f"[parity] sr_round share rounded up at f = {f}: {share:.6f} (bound +-{bound:.6f})")
    assert abs(share - f) <= bound


# ---- 3. constant-gradient drift ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [True, False])
def test_constant_gradient_drift(sr):
    """p0 = 1, g = 1, lr 1e-4, no weight decay, no clip, 200 bf16-state steps on >= 2^20 parameters. Every update (1e-4) is far
    below half an ulp of 1.0 in bf16 (2^-8): with round-to-nearest NO parameter ever moves - the failure the option fixes,
    pinned here - while with stochastic rounding the mean follows AdamW's 1 - 200 lr = 0.98 (per-element std 0.0087 in the
    fp32 emulation of the issue: the mean of 2^20 elements has a std <= 8.5e-6, the bound is beyond 10 sigma). Pad rows of the
    embedding (zero weights, zero gradients) stay exactly zero either way."""
    sd = O.init_weights(O.TINY, seed=4)
    m = _tiny_model(sd)
    tr = _trainer(m, "bfloat16", sr, weight_decay=0.0, max_grad_norm=0.0)
    n, H = m.engine.n_params, O.TINY.hidden
    assert n >= 2 ** 20
    emb = m.engine.tensors["embed"]
    pad = torch.zeros(n, dtype=torch.bool, device="cuda")
    pad[emb.offset + O.TINY.vocab * H: emb.offset + emb.rows * H] = True
    assert int(pad.sum()) == (emb.rows - O.TINY.vocab) * H > 0
    m.flat_params.fill_(1.0)
    m.flat_params[pad] = 0.0
    m.engine.refresh_transposed()
    for _ in range(200):
        m.flat_grads.fill_(1.0)
        m.flat_grads[pad] = 0.0
        tr._clip_and_update(1e-4, zero_grad=False)
    torch.cuda.synchronize()
    p, mo, vo = m.flat_params.float(), tr.exp_avg.float(), tr.exp_avg_sq.float()
    for t in (p, mo, vo):
        assert float(t[pad].abs().max()) == 0.0
    live = ~pad
    mp, mm, mv = float(p[live].double().mean()), float(mo[live].double().mean()), float(vo[live].double().mean())
    print(f"[parity] constant gradient, 200 steps, adamw_sr {int(sr)}: mean p {mp:.6f} (AdamW 0.98), std {float(p[live].std()):.5f}, "
          f"mean m {mm:.5f} (1), mean v {mv:.5f} ({1 - 0.999 ** 200:.5f})")
    if sr:
        assert abs(mp - 0.98) <= 1e-4
        assert abs(mm - 1.0) <= 1e-3
        assert abs(mv - (1.0 - 0.999 ** 200)) <= 1e-3
    else:
        assert bool((p[live] == 1.0).all())


# ---- 4. one bit pattern, every kernel form -----------------------------------------------------------------------------------
def _sharded_update(tr, m, world, lr):
    """tests/test_gpu_train.py's virtual-rank pattern: the ranks' shards of every bucket in turn, then the replicated tail."""
    eng, n = m.engine, m.engine.n_params
    chunk, nchunks = eng.grad_chunk_info()
    align = world * chunk
    top = (n // align) * align
    cuts = sorted({0, top} | {(int(top * f) // align) * align for f in (0.21, 0.5, 0.77)})
    buckets = [(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    cs = torch.zeros(nchunks, dtype=torch.float32, device="cuda")
    owned = {r: [(lo + r * ((hi - lo) // world), (hi - lo) // world) for lo, hi in buckets] for r in range(world)}
    for r in range(world):
        for off, cnt in owned[r]:
            eng.grad_sumsq_chunks(off, cnt, cs)
    if top < n:
        eng.grad_sumsq_chunks(top, n - top, cs)
    eng.grad_norm_from_chunks(cs, tr.args.max_grad_norm, tr.norm_out)
    tr.opt_step += 1
    master = None if tr.state_dtype == torch.bfloat16 else m.flat_master
    for r in reversed(range(world)):
        for off, cnt in owned[r] + ([(top, n - top)] if r == 0 and top < n else []):
            eng.adamw_range(off, cnt, master, tr.exp_avg, tr.exp_avg_sq, tr.norm_out, lr, tr.args.adam_beta1, tr.args.adam_beta2,
                            tr.args.adam_epsilon, tr.args.weight_decay, tr.opt_step, zero_grad=False)


def _assert_images_are_transposes(m):
    """Every matrix of the engine's layout (the padded embedding included): its image is its transpose."""
    seen = 0
    for name, t in m.engine.tensors.items():
        if t.cols > 1:
            w = m.flat_params[t.offset:t.offset + t.numel].view(t.rows, t.cols)
            wt = m.flat_params_t[t.offset:t.offset + t.numel].view(t.cols, t.rows)
            assert torch.equal(wt.t().contiguous(), w), name
            seen += 1
    assert seen >= 1 + 4 * O.TINY.n_layers


@pytest.mark.parametrize("osd", ["bfloat16", "float32_bf16_moments"])
def test_every_kernel_form_rounds_to_the_same_bits(osd):
    """adamw_sr on, one start state, the same gradients, 2 steps: the tile kernels that write the transposed images
    ("fuse_adamw_t" 1), the flat kernels + transpose pass (0), "overlap_adamw" 1, and the sharded update over 2 and 8 virtual
    ranks (slam_adamw_range*) give identical p, master, m, v and images as int16 / fp32 bits - the random bits of an element
    follow from its index in the flat buffer, not from the launch that reaches it. Every image is the transpose of its matrix."""
    sd = O.init_weights(O.TINY, seed=4, bias_std=0.02, norm_jitter=0.05)
    forms = [("fused", {"fuse_adamw_t": 1}, 0), ("flat", {"fuse_adamw_t": 0}, 0), ("overlap", {"overlap_adamw": 1}, 0),
             ("sharded2", {}, 2), ("sharded8", {}, 8)]
    res = {}
    for name, opts, world in forms:
        m = _tiny_model(sd)
        assert m.flat_params_t is not None
        tr = _trainer(m, osd, True, seed=11, weight_decay=0.01, max_grad_norm=0.5)
        for k, v in opts.items():
            m.engine.set_option(k, v)
        gen = torch.Generator().manual_seed(0)
        for _ in range(2):
            m.flat_grads.copy_(torch.randn(m.engine.n_params, generator=gen) * 1e-2)
            if world:
                _sharded_update(tr, m, world, 1e-3)
            else:
                tr._clip_and_update(1e-3, zero_grad=False)
        m.engine.join()
        torch.cuda.synchronize()
        if name == "fused":  # the images the tile kernels wrote themselves, before any refresh
            _assert_images_are_transposes(m)
        m.engine.refresh_transposed()
        torch.cuda.synchronize()
        _assert_images_are_transposes(m)
        res[name] = (m.flat_params.clone(), m._weights.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), m.flat_params_t.clone())
    # and the rounding was stochastic: the same steps with the option off give other bits
    m = _tiny_model(sd)
    tr = _trainer(m, osd, False, weight_decay=0.01, max_grad_norm=0.5)
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        m.flat_grads.copy_(torch.randn(m.engine.n_params, generator=gen) * 1e-2)
        tr._clip_and_update(1e-3, zero_grad=False)
    torch.cuda.synchronize()
    assert not torch.equal(tr.exp_avg, res["fused"][2])
    if osd == "float32_bf16_moments":  # the working copy of the fp32 master keeps round-to-nearest
        assert torch.equal(res["fused"][0], res["fused"][1].to(torch.bfloat16))
    for name, _, _ in forms[1:]:
        for a, b, what in zip(res["fused"], res[name], ("params", "weights", "exp_avg", "exp_avg_sq", "params_t")):
            assert torch.equal(a, b), (name, what, int((a != b).sum()))


def _train(sd, steps, fuse, sr=True, seed=3, osd="bfloat16", out="/tmp/unused", **kw):
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    g = torch.Generator().manual_seed(1)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (40,), generator=g).tolist(), "attention_mask": [1] * 41} for _ in range(16)]
    m = _tiny_model(sd)
    if fuse is not None:
        m.engine.set_option("fuse_adamw_t", fuse)
    a = SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=steps, warmup_steps=1, warmup_ratio=0.0, logging_steps=0,
                              output_dir=str(out), num_train_epochs=8, optim_state_dtype=osd, optim_stochastic_rounding=sr,
                              optim_sr_seed=seed, **kw)
    tr = SLAMTrainer(model=m, args=a, data_collator=DataCollatorForLanguageModeling(pad_token_id=0), train_dataset=TokenDataset(rows))
    return m, tr


def test_real_steps_16_byte_tile_kernel_against_the_flat_kernel():
    """Trainer steps in the recipe's precision end to end (bf16 parameters, moments AND final gradients): the update runs in
    the 16-byte-access tile kernel (one Philox call per thread and array) with "fuse_adamw_t" 1 and in the flat bf16 kernel +
    transpose pass with 0. Same bits after 4 steps, images included."""
    sd = O.init_weights(O.TINY, seed=9)
    res = []
    for fuse in (1, 0):
        m, tr = _train(sd, 4, fuse)
        assert tr._final_mode == 2
        tr.train()
        torch.cuda.synchronize()
        if fuse:
            _assert_images_are_transposes(m)
        res.append((m.flat_params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), m.flat_params_t.clone()))
    for a, b, what in zip(res[0], res[1], ("params", "exp_avg", "exp_avg_sq", "params_t")):
        assert torch.equal(a, b), what


def _real_steps(fuse, path=None):
    """4 trainer steps in the recipe's precision with stochastic rounding; the four flat buffers (saved to `path` if given)."""
    sd = O.init_weights(O.TINY, seed=9)
    m, tr = _train(sd, 4, fuse)
    tr.train()
    torch.cuda.synchronize()
    out = {"params": m.flat_params.cpu(), "exp_avg": tr.exp_avg.cpu(), "exp_avg_sq": tr.exp_avg_sq.cpu(), "params_t": m.flat_params_t.cpu()}
    if path:
        torch.save(out, path)
    return out


@pytest.mark.parametrize("env", [{"SLAM_ADAMW_X8": "0"}, {"SLAM_ADAMW_TILE_COLS": "64"}])
def test_real_steps_other_tile_kernels_in_a_child_process(env, tmp_path):
    """The tile kernel's other instantiations are picked by environment knobs read once per process (SLAM_ADAMW_X8=0: the
    8-byte-access kernel on bf16 gradients; SLAM_ADAMW_TILE_COLS=64: 64-column tiles): a child process runs the same 4 steps
    under the knob - the same bits as the 16-byte kernel here."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "child.pt")
    r = subprocess.run([sys.executable, "-c", f"from tests.test_gpu_sr import _real_steps; _real_steps(1, {out!r})"], cwd=root,
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = torch.load(out, map_location="cpu")
    mine = _real_steps(1)
    for k in mine:
        assert torch.equal(mine[k], child[k]), (env, k, int((mine[k] != child[k]).sum()))


# ---- 5. seeded and reproducible -------------------------------------------------------------------------------------------------
def test_seeded_and_reproducible():
    sd = O.init_weights(O.TINY, seed=4, bias_std=0.02, norm_jitter=0.05)

    def one_step(sr, seed=7, toggle=False):
        m = _tiny_model(sd)
        tr = _trainer(m, "bfloat16", sr, seed=seed, weight_decay=0.01, max_grad_norm=0.5)
        if toggle:  # on and off again: the bits of an engine that never set it
            m.engine.set_option("adamw_sr", 1)
            m.engine.set_option("adamw_sr", 0)
        m.flat_grads.copy_(torch.randn(m.engine.n_params, generator=torch.Generator().manual_seed(0)) * 1e-2)
        tr._clip_and_update(1e-3, zero_grad=False)
        torch.cuda.synchronize()
        return [_bits(t) for t in (m.flat_params, tr.exp_avg, tr.exp_avg_sq)]

    a, b, c = one_step(True), one_step(True), one_step(True, seed=8)
    rtn, rtn2 = one_step(False), one_step(False, toggle=True)
    n = a[0].size
    for x, y, z, r, r2, what in zip(a, b, c, rtn, rtn2, "pmv"):
        assert np.array_equal(x, y), what                                   # one seed: the same bits
        assert np.array_equal(r, r2), what                                  # 1 and back to 0: as if never set
        # every element is the round-to-nearest result or its bf16 neighbour
        assert int(np.abs(x.astype(np.int32) - r.astype(np.int32)).max()) <= 1, what
        # another seed changes more than 1 % of ALL elements (the elements whose fp32 result is not representable are fewer)
        changed = float((x != z).mean())
        print(f"[parity] adamw_sr, array {what}: another seed changes {100 * changed:.1f} % of {n} elements; "
              f"{100 * float((x != r).mean()):.1f} % differ from round-to-nearest")
        assert changed > 0.01, what
    # the step number is part of the counter: on one input, another step changes more than 1 % of the inexact elements
    g = np.random.default_rng(1)
    x = g.standard_normal(2 ** 20).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    inexact = (x.view(np.uint32) & 0xffff) != 0
    s1, s2, s1b = _sr_round(xd, 7, 1, 0, 0), _sr_round(xd, 7, 2, 0, 0), _sr_round(xd, 7, 1, 0, 0)
    assert np.array_equal(s1, s1b)
    assert float((s1[inexact] != s2[inexact]).mean()) > 0.01
    assert float((s1[inexact] != _sr_round(xd, 8, 1, 0, 0)[inexact]).mean()) > 0.01
    assert float((s1[inexact] != _sr_round(xd, 7, 1, 0, 1)[inexact]).mean()) > 0.01  # and so does the array


# ---- 6. trainer-level tracking ---------------------------------------------------------------------------------------------
TRACK_STEPS = 600  # the issue asks for >= 300 and to lengthen rather than loosen: three epochs of the 200-batch stream


def test_sr_run_tracks_the_fp32_master_run():
    """The tiny golden model on the tests/traj_stream data at the recipe's final learning rate (constant 5e-5 after a 5-step
    warm-up), TRACK_STEPS optimizer steps, three runs from ONE bf16-representable state: fp32 master (the reference), bf16
    state with round-to-nearest, bf16 state with stochastic rounding. err(X) = |p_X - p_fp32| / |p_fp32 - p0| over all
    parameters. Asserted: err(SR) <= 0.5 err(RTN) - the issue's bound, set before anything was measured."""
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests import traj_stream as TS
    sd = {k: v.to(torch.bfloat16).float() for k, v in O.init_weights(O.TINY, seed=11, bias_std=0.0, norm_jitter=0.0).items()}
    ds, coll = TS.dataset(), TS.collator()
    out, curves = {}, {}
    for name, osd, sr in (("fp32", "float32", False), ("rtn", "bfloat16", False), ("sr", "bfloat16", True)):
        args = SLAMTrainingArguments(per_device_train_batch_size=TS.BS, gradient_accumulation_steps=1, num_train_epochs=4,
                                     max_steps=TRACK_STEPS, warmup_steps=5, warmup_ratio=0.0, learning_rate=5e-5,
                                     lr_scheduler_type="constant_with_warmup", logging_steps=20, max_grad_norm=TS.CLIP,
                                     weight_decay=0.0, seed=TS.SEED, output_dir="/tmp/unused", optim_state_dtype=osd,
                                     optim_stochastic_rounding=sr)
        m = _tiny_model(sd)
        tr = SLAMTrainer(model=m, args=args, data_collator=coll, train_dataset=ds)
        state = tr.train()
        assert state.global_step == TRACK_STEPS
        out[name] = m.state_dict(torch.float32)
        curves[name] = [r["loss"] for r in state.log_history if "loss" in r]
    keys = list(sd)
    cat = lambda d: torch.cat([d[k].flatten().double() for k in keys])  # noqa: E731
    p0, pf, pr, ps = cat(sd), cat(out["fp32"]), cat(out["rtn"]), cat(out["sr"])
    drift = float((pf - p0).norm())
    err_rtn, err_sr = float((pr - pf).norm()) / drift, float((ps - pf).norm()) / drift
    frozen = {k: float((v == p0).double().mean()) for k, v in (("fp32", pf), ("rtn", pr), ("sr", ps))}
    for name in ("fp32", "rtn", "sr"):
        print(f"[parity] sr tracking, {name} loss every 100 steps: {[round(x, 4) for x in curves[name][4::5]]}")
    print(f"[parity] sr tracking, {TRACK_STEPS} steps at lr 5e-5: err(RTN) {err_rtn:.4f}, err(SR) {err_sr:.4f}, ratio {err_sr / err_rtn:.4f}; "
          f"share of parameters that never moved: fp32 {frozen['fp32']:.4f}, RTN {frozen['rtn']:.4f}, SR {frozen['sr']:.4f}")
    assert err_sr <= 0.5 * err_rtn, (err_sr, err_rtn)


# ---- 7. resume -------------------------------------------------------------------------------------------------------------------
def test_resumed_sr_run_repeats_the_uninterrupted_one(tmp_path):
    """k steps with stochastic rounding, checkpoint, resume, k more: parameters and moments equal the uninterrupted 2k-step
    run bit for bit. Nothing about the generator is in the checkpoint: it is keyed on the optimizer step."""
    sd = O.init_weights(O.TINY, seed=9)
    k = 3
    m_full, tr_full = _train(sd, 2 * k, None, out=tmp_path / "a", save_steps=k)
    tr_full.train()
    assert os.path.isdir(tmp_path / "a" / f"checkpoint-{k}")
    assert set(torch.load(tmp_path / "a" / f"checkpoint-{k}" / "optimizer.pt", map_location="cpu")) == {"master", "exp_avg", "exp_avg_sq", "opt_step"}
    m_res, tr_res = _train(sd, 2 * k, None, out=tmp_path / "b")
    tr_res.train(resume_from_checkpoint=str(tmp_path / "a" / f"checkpoint-{k}"))
    assert tr_res.state.global_step == 2 * k and tr_res.opt_step == 2 * k
    torch.cuda.synchronize()
    for a, b, what in ((m_full.flat_params, m_res.flat_params, "params"), (tr_full.exp_avg, tr_res.exp_avg, "exp_avg"),
                       (tr_full.exp_avg_sq, tr_res.exp_avg_sq, "exp_avg_sq"), (m_full.flat_params_t, m_res.flat_params_t, "params_t")):
        assert torch.equal(a, b), what
    # and the rounding was on: the same run without it ends elsewhere
    m_rtn, tr_rtn = _train(sd, 2 * k, None, sr=False)
    tr_rtn.train()
    assert not torch.equal(m_rtn.flat_params, m_full.flat_params)
