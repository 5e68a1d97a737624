"""-m gpu: the no-decay set of AdamW (slam_set_decay_mask; weight_decay_rule = "hf").

Bodies, the smallest that can go wrong: a 2-layer Qwen2 with hidden 64 - ln1 (64 elements), a piece of wqkv and bqkv (192) lie
inside the 1024 / 2048 elements of one 256-thread block, so a block's threads take different answers from the table - and the
2-layer OPT of test_gpu_opt.py (eight vector kinds per layer, and pos_embed: a vector group of the optimizer's walk that IS
decayed). Both end on their final norm inside a partial block.

A masked step is defined bit for bit by two unmasked ones from the same state, A with the weight decay and B with 0: a no-decay
element goes through the same expression with wd = 0. No tolerance anywhere in the composition tests."""
import json
import os
import re

import pytest
import torch

from oracle import slam_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR, WD, STEP = 1e-2, 0.1, 3
BODIES = ["qwen2", "opt"]


def _make(body, seed=5, max_tokens=64):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    if body == "opt":
        from tests.test_gpu_opt import TINY
        base = dict(model_type="opt", **TINY)
    else:
        base = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=1, num_key_value_heads=1, head_dim=64,
                    intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=502, max_tokens=max_tokens), seed=seed)
    assert m.flat_params_t is not None  # the fused walk needs the transposed images
    return m


def _perturbed(body, seed=5):
    """Non-trivial norm weights and biases (the init has ones and zeros), bf16-representable."""
    m = _make(body, seed)
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "norm" in k:
            sd[k] = (v + 0.05 * torch.randn(v.shape, generator=g)).bfloat16().float()
    m.load_state_dict(sd)
    return m


def _ranges(m):
    """(name, lo, hi) per engine tensor, in layout order: a tensor owns the elements up to the next tensor's offset"""
    specs = list(m.engine.tensors.values())
    assert [t.offset for t in specs] == sorted(t.offset for t in specs)
    his = [t.offset for t in specs[1:]] + [m.engine.n_params]
    return [(t.name, t.offset, hi) for t, hi in zip(specs, his)]


def _decayed_elements(m, flags):
    d = torch.zeros(m.engine.n_params, dtype=torch.bool)
    for (_, lo, hi), f in zip(_ranges(m), flags):
        d[lo:hi] = bool(f)
    return d.cuda()


def _fixture_flags(m, body):
    """The decay flag of every engine tensor from tests/golden/decay_names.json (HF's own answer), layer index folded to 0."""
    from tests.test_decay_rule_host import _names_by_tensor
    with open(os.path.join(GOLDEN, "decay_names.json")) as f:
        fx = json.load(f)["models"]["opt" if body == "opt" else "qwen2_tied"]
    decay, known = set(fx["decay"]), set(fx["parameters"])
    flags = []
    for name, names in _names_by_tensor(m).items():
        canon = [re.sub(r"layers\.\d+\.", "layers.0.", n) for n in names]
        assert canon and all(c in known for c in canon), (name, canon)
        inside = {c in decay for c in canon}
        assert len(inside) == 1, name
        flags.append(inside.pop())
    assert list(_names_by_tensor(m)) == list(m.engine.tensors)
    return flags


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------- composition (tests 1 and 2)
class Bench:
    """One model per body for the composition tests, a fixed random optimizer state, and the step in every mode and path."""

    def __init__(self, body):
        self.body = body
        self.m = m = _make(body)
        self.n = n = m.engine.n_params
        self.flags = m.hf_decay_flags()
        assert self.flags == _fixture_flags(m, body)
        self.decayed = _decayed_elements(m, self.flags)
        g = torch.Generator().manual_seed(3)
        r = lambda s: (torch.randn(n, generator=g) * s)  # noqa: E731
        self.p0 = r(0.5).bfloat16().cuda()
        self.w0 = (self.p0.float().cpu() + r(1e-3)).cuda()   # fp32 master beside its bf16 working copy
        self.m0, self.v0, self.g0 = r(1e-2).cuda(), r(1e-2).abs().cuda(), r(1e-2).cuda()
        self.clip = torch.tensor([2.0, 0.5], dtype=torch.float32, device="cuda")  # gradients scaled by clip[1]
        self.gmode = False  # a fresh engine reads the fp32 buffer
        rg = {name: (lo, hi) for name, lo, hi in _ranges(m)}
        nd, dc = ("layers.0.ln1_b", "layers.1.w1") if body == "opt" else ("layers.0.bqkv", "layers.1.wqkv")
        assert not self.flags[list(m.engine.tensors).index(nd)] and self.flags[list(m.engine.tensors).index(dc)]
        # shard cuts inside a no-decay tensor and inside a decayed one: multiples of 4 that are no multiples of 8 where the
        # kernel goes 4 elements a thread (modes 0 and 1), multiples of 8 for the bf16-state kernel
        self.cuts = {4: (rg[nd][0] + 44, rg[dc][0] + 1004), 8: (rg[nd][0] + 40, rg[dc][0] + 1000)}
        for a, b in self.cuts.values():
            assert rg[nd][0] < a < rg[nd][1] and rg[dc][0] < b < rg[dc][1]

    def grad_mode(self, bf16):
        """Where the optimizer reads gradients follows the last backward: a real one, kept in bf16 only (final = 2) or not."""
        if self.gmode == bf16:
            return
        m = self.m
        ids = torch.randint(2, 502, (1, 64), generator=torch.Generator().manual_seed(1))
        ids[:, 0] = 1
        m.engine.set_option("grad_overwrite_next", 1)
        m(input_ids=ids, labels=ids)
        m.backward(final=2 if bf16 else 0)
        torch.cuda.synchronize()
        self.gmode = bf16

    def step(self, mode, g16, sr, path, wd, mask):
        m, eng, n = self.m, self.m.engine, self.n
        self.grad_mode(g16)
        eng.set_decay_mask(self.flags if mask else None)
        eng.set_option("adamw_sr", int(sr))
        eng.set_option("adamw_sr_seed", 1234)
        eng.set_option("fuse_adamw_t", 1 if path in ("fused", "overlap_fused") else 0)
        eng.set_option("overlap_adamw", 1 if path.startswith("overlap") else 0)
        m.flat_params.copy_(self.p0)
        m.flat_params_t.zero_()
        if g16:
            m.flat_grads16.copy_(self.g0)
        else:
            m.flat_grads.copy_(self.g0)
        md = torch.float32 if mode == 0 else torch.bfloat16
        w = self.w0.clone() if mode != 2 else None
        ea, eq = self.m0.to(md, copy=True), self.v0.to(md, copy=True)  # fresh arrays: the step updates them in place
        args = (self.clip, LR, 0.9, 0.999, 1e-8, wd, STEP)
        try:
            if path == "ranges":
                c1, c2 = self.cuts[8 if mode == 2 else 4]
                for lo, hi in ((c2, n), (0, c1), (c1, c2)):
                    eng.adamw_range(lo, hi - lo, w, ea, eq, *args, zero_grad=False)
                eng.refresh_transposed()
            elif mode == 2:
                eng.adamw_step_bf16(ea, eq, *args, zero_grad=True)
            else:
                eng.adamw_step(w, ea, eq, *args, zero_grad=True)
            eng.join()
            torch.cuda.synchronize()
        finally:
            eng.set_option("overlap_adamw", 0)
            eng.set_option("adamw_sr", 0)
            eng.set_option("fuse_adamw_t", 1)
            eng.set_decay_mask(None)
        out = {"params": m.flat_params.clone(), "params_t": m.flat_params_t.clone(), "exp_avg": ea, "exp_avg_sq": eq}
        if w is not None:
            out["master"] = w
        return out


_benches = {}


@pytest.fixture(params=BODIES)
def bench(request):
    if request.param not in _benches:
        _benches[request.param] = Bench(request.param)
    return _benches[request.param]


def _paths(mode):
    return ["flat", "fused", "ranges"] + (["overlap_flat", "overlap_fused"] if mode == 0 else [])


CASES = [(mode, g16, sr, path) for mode in (0, 1, 2) for g16 in (False, True) for sr in (False, True) for path in _paths(mode)]


@pytest.mark.parametrize("mode,g16,sr,path", CASES, ids=[f"mode{c[0]}-{'g16' if c[1] else 'g32'}-{'sr' if c[2] else 'rn'}-{c[3]}" for c in CASES])
def test_masked_step_is_the_composition_of_two_unmasked_steps(bench, mode, g16, sr, path):
    """One masked step (lr 1e-2, wd 0.1, random gradients and state, step 3, clip coefficient 0.5) in every state precision, with
    fp32 and bf16-kept gradients, round-to-nearest and stochastic rounding, on the flat path, the fused walk that writes the
    transposed images, the overlapped chunks (fp32 state) and three ranged shards cut inside a no-decay and inside a decayed
    tensor: every state array and the transposed images equal run A (wd 0.1, no mask) on the decayed tensors and run B (wd 0, no
    mask) on the others, bit for bit; and after the mask is cleared the step is A everywhere."""
    masked = bench.step(mode, g16, sr, path, WD, mask=True)
    a = bench.step(mode, g16, sr, path, WD, mask=False)
    b = bench.step(mode, g16, sr, path, 0.0, mask=False)
    d = bench.decayed
    assert not _same(a["params"][d], b["params"][d]) and not _same(a["params"][~d], b["params"][~d])  # A and B differ everywhere it matters
    for k in masked:
        want = torch.where(d, a[k], b[k])
        bad = _bits(masked[k]) != _bits(want)
        assert not bool(bad.any()), (k, int(bad.sum()), bad.nonzero()[:4].flatten().tolist())
    # (bench.step clears the mask on its way out: `a` above already ran behind a set-and-cleared mask of the previous case)
    bench.m.engine.set_decay_mask(bench.flags)
    cleared = bench.step(mode, g16, sr, path, WD, mask=False)
    for k in a:
        assert _same(cleared[k], a[k]), k


@pytest.mark.parametrize("path", ["flat", "fused", "ranges", "overlap_flat"])
def test_zero_gradient_step_moves_only_the_decayed_tensors(bench, path):
    """fp32 state, zero gradients and zero moments: the update term is exactly 0, so after one masked step a no-decay tensor
    keeps its bits and a decayed one is p * (1 - lr * wd) in fp32. Without the feature every tensor shrinks."""
    m, eng, n = bench.m, bench.m.engine, bench.n
    bench.grad_mode(False)
    w0 = bench.p0.float()  # bf16-representable: the working copy of an untouched tensor keeps its bits too
    saved = (bench.w0, bench.m0, bench.v0, bench.g0)
    bench.w0, bench.m0, bench.v0, bench.g0 = w0, torch.zeros_like(w0), torch.zeros_like(w0), torch.zeros_like(w0)
    try:
        out = bench.step(0, False, False, path, WD, mask=True)
    finally:
        bench.w0, bench.m0, bench.v0, bench.g0 = saved
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda")  # noqa: E731
    shrunk = w0 * (f32(1.0) - f32(LR) * f32(WD))
    d = bench.decayed
    assert _same(out["master"][~d], w0[~d]) and _same(out["params"][~d], bench.p0[~d])
    assert _same(out["master"][d], shrunk[d]) and _same(out["params"][d], shrunk.bfloat16()[d])
    assert not _same(shrunk[d], w0[d])
    assert float(out["exp_avg"].abs().max()) == 0.0 and float(out["exp_avg_sq"].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- trainer parity (test 3)
def _oracle_steps(update, p, m, n, flags, steps=5):
    """`steps` updates of the flat CPU state with the oracle, wd = 0.01 on the fixture's decay names and 0 on the rest; returns
    the gradients it drew (the engine gets the same ones)."""
    mo, vo = torch.zeros(n).bfloat16(), torch.zeros(n).bfloat16()
    gen = torch.Generator().manual_seed(0)
    grads = []
    for step in range(1, steps + 1):
        g = torch.randn(n, generator=gen) * 1e-2
        grads.append(g)
        for (_, lo, hi), f in zip(_ranges(m), flags):
            update(p[lo:hi], g[lo:hi], mo[lo:hi], vo[lo:hi], step, 1e-3, wd=0.01 if f else 0.0)
    return grads, mo, vo


def _moments_close(tr, mo, vo):
    for mine, ref in ((tr.exp_avg.cpu(), mo), (tr.exp_avg_sq.cpu(), vo)):
        tol = 2.0 ** -5 * ref.float().abs() + 2e-3 * float(ref.float().abs().max())
        err = (mine.float() - ref.float()).abs()
        bad = err > tol
        assert not bool(bad.any()), (int(bad.sum()), mine[bad][:4].tolist(), ref[bad][:4].tolist(), float(ref.float().abs().max()))


@pytest.mark.parametrize("body", BODIES)
def test_adamw_bf16_state_step_vs_oracle_under_the_hf_rule(body):
    """test_gpu_train.py::test_adamw_bf16_state_step_vs_oracle with weight_decay_rule = "hf": 5 updates against the oracle's
    restatement of torch's fused bf16 AdamW called tensor by tensor, wd = 0.01 on the names HF decays (decay_names.json) and 0
    on the others. Tolerances as there."""
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    m = _perturbed(body)
    tr = SLAMTrainer(model=m, args=SLAMTrainingArguments(optim_state_dtype="bfloat16", weight_decay=0.01, max_grad_norm=0.0,
                                                         logging_steps=0, weight_decay_rule="hf"))
    n = m.engine.n_params
    flags = _fixture_flags(m, body)
    p = m.flat_params.detach().cpu().clone()
    grads, mo, vo = _oracle_steps(O.adamw_update_bf16, p, m, n, flags)
    for g in grads:
        m.flat_grads.copy_(g)
        tr._clip_and_update(1e-3, zero_grad=True)
    torch.cuda.synchronize()
    assert float(m.flat_grads.abs().max()) == 0.0
    got = m.flat_params.cpu()
    print(f"[parity] {body}: {int((got != p).sum())} of {n} parameters differ, max abs {float((got.float() - p.float()).abs().max()):.3e}")
    assert int((got != p).sum()) <= n // 1000, int((got != p).sum())
    assert float((got.float() - p.float()).abs().max()) <= 2 ** -7 * float(p.float().abs().max())
    _moments_close(tr, mo, vo)
    # the transposed weight images follow the in-place update
    lo, hi = next((lo, hi) for name, lo, hi in _ranges(m) if name == "layers.0.wo")
    t = m.engine.tensors["layers.0.wo"]
    wt = m.flat_params_t[lo:hi].view(t.cols, t.rows)
    assert torch.equal(wt.t().contiguous(), m.flat_params[lo:hi].view(t.rows, t.cols))


@pytest.mark.parametrize("body", BODIES)
def test_adamw_bf16_moments_step_vs_oracle_under_the_hf_rule(body):
    """test_gpu_train.py::test_adamw_bf16_moments_step_vs_oracle with weight_decay_rule = "hf" (fp32 master + bf16 moments)."""
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    m = _perturbed(body)
    tr = SLAMTrainer(model=m, args=SLAMTrainingArguments(optim_state_dtype="float32_bf16_moments", weight_decay=0.01, max_grad_norm=0.0,
                                                         logging_steps=0, weight_decay_rule="hf"))
    n = m.engine.n_params
    flags = _fixture_flags(m, body)
    p = m.flat_master.detach().cpu().clone()
    grads, mo, vo = _oracle_steps(O.adamw_update_bf16_moments, p, m, n, flags)
    for g in grads:
        m.flat_grads.copy_(g)
        tr._clip_and_update(1e-3, zero_grad=True)
    torch.cuda.synchronize()
    got = m.flat_master.cpu()
    print(f"[parity] {body}: master max abs {float((got - p).abs().max()):.3e} at scale {float(p.abs().max()):.3e}")
    assert float((got - p).abs().max()) <= 2e-5 * float(p.abs().max()) + 1e-7, float((got - p).abs().max())
    assert torch.equal(m.flat_params.cpu(), got.bfloat16())  # the working copy is the rounded master
    _moments_close(tr, mo, vo)


# ------------------------------------------------------------------------------------ sharded equals replicated (test 4)
@pytest.mark.parametrize("osd", ["float32", "bfloat16", "float32_bf16_moments"])
@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("body", BODIES)
def test_sharded_update_equals_the_replicated_step_under_the_hf_rule(body, world, osd):
    """test_gpu_train.py::test_sharded_update_over_virtual_ranks_equals_the_replicated_step with the rule on: `world` virtual
    ranks update their shards of every bucket through slam_adamw_range* (the cuts fall wherever world x chunk puts them, inside
    decayed and no-decay tensors alike); norm, parameters, master, moments and the refreshed images equal the replicated masked
    step bit for bit - and differ from the unmasked one."""
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    res = []
    for sharded, rule in ((False, "hf"), (True, "hf"), (False, "all")):
        m = _perturbed(body)
        eng = m.engine
        n = eng.n_params
        tr = SLAMTrainer(model=m, args=SLAMTrainingArguments(optim_state_dtype=osd, weight_decay=0.01, max_grad_norm=0.5, logging_steps=0,
                                                             weight_decay_rule=rule))
        g2 = torch.Generator().manual_seed(0)
        norms = []
        for step in range(2):
            m.flat_grads.copy_(torch.randn(n, generator=g2) * 1e-2)
            if not sharded:
                tr._clip_and_update(1e-3, zero_grad=False)
            else:
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
                eng.grad_norm_from_chunks(cs, 0.5, tr.norm_out)
                tr.opt_step += 1
                master = None if tr.state_dtype == torch.bfloat16 else m.flat_master
                for r in reversed(range(world)):  # any order: the ranges are disjoint
                    for off, cnt in owned[r] + ([(top, n - top)] if r == 0 and top < n else []):
                        eng.adamw_range(off, cnt, master, tr.exp_avg, tr.exp_avg_sq, tr.norm_out, 1e-3, tr.args.adam_beta1, tr.args.adam_beta2,
                                        tr.args.adam_epsilon, tr.args.weight_decay, tr.opt_step, zero_grad=False)
            norms.append(float(tr.norm_out[0]))
        eng.refresh_transposed()
        torch.cuda.synchronize()
        res.append((norms, m.flat_params.clone(), (m.flat_master if m.flat_master is not None else m.flat_params).clone(),
                    tr.exp_avg.clone(), tr.exp_avg_sq.clone(), m.flat_params_t.clone()))
    assert res[0][0] == res[1][0], f"gradient norms differ: {res[0][0]} vs {res[1][0]}"
    for a, b, name in zip(res[0][1:], res[1][1:], ("params", "master", "exp_avg", "exp_avg_sq", "params_t")):
        assert torch.equal(a, b), name
    assert not torch.equal(res[0][2], res[2][2])  # the rule changes the step: the comparison above is not vacuous
