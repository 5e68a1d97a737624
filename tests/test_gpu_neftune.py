"""NEFTune (slam_set_neftune, engine option "neftune_call_next") on the GPU: the armed embedding launch against the numpy
restatement (tests/neftune_ref.py) bit for bit, the engine's own launch through identity-layer models of the three families,
arming / eval / scoring / generate, recomputation, the padding-free layout and a resumed trainer run."""
import numpy as np
import pytest
import torch

from tests import neftune_ref as R
from tests.gpu_util import lib, ptr, stream, sync

pytestmark = pytest.mark.gpu

V = 502
QWEN2 = dict(num_hidden_layers=2, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
             intermediate_size=512, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
QWEN3 = dict(QWEN2, model_type="qwen3", initializer_range=0.02)
OPT = dict(model_type="opt", num_hidden_layers=2, hidden_size=256, num_attention_heads=4, ffn_dim=512,
           max_position_embeddings=128, init_std=0.02)
FAMILIES = {"qwen2": (QWEN2, {}), "qwen2-untied": (QWEN2, dict(tie_word_embeddings=False)), "qwen3": (QWEN3, {}), "opt": (OPT, {})}


def _bits(t):
    """uint16 bits of a bf16 tensor, as numpy."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _i64(seed):
    seed &= 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def _table(rows, H, seed):
    """fp32 [rows, H] of bf16-representable values, std 0.02 - what an embedding table holds."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, H, generator=g) * 0.02).to(torch.bfloat16).float()


# --------------------------------------------------------------------------------------------------------------------- op
def _run_op(ids, E_, s, seed, call, index0=0, P=None, T=1, pos=None):
    M, H = len(ids), E_.shape[1]
    ids_d = torch.as_tensor(ids, dtype=torch.int64).cuda()
    Ed = E_.to(torch.bfloat16).cuda()
    Pd = P.to(torch.bfloat16).cuda() if P is not None else None
    pos_d = torch.as_tensor(pos, dtype=torch.int64).cuda() if pos is not None else None
    out = torch.full((M + 1, H), float("nan"), dtype=torch.bfloat16, device="cuda")  # one guard row behind the launch's
    prow = torch.full((M,), -7, dtype=torch.int64, device="cuda") if P is not None else None
    import ctypes as C
    rc = lib().slam_op_embed_noise_fwd(ptr(ids_d), ptr(pos_d), ptr(Ed), ptr(Pd), ptr(out), ptr(prow), M, H, E_.shape[0], T,
                                       P.shape[0] if P is not None else 0, C.c_float(float(s)), _i64(seed), call, index0,
                                       stream())
    assert rc == 0
    sync()
    assert bool(torch.isnan(out[M]).all())  # nothing behind the last row was written
    return _bits(out[:M]), (prow.cpu().numpy() if prow is not None else None)


@pytest.mark.parametrize("seed,call", [(0x1234_5678_9ABC_DEF0, 7), (11, 0xFFFFFFFF)], ids=["seedA", "seedB"])
@pytest.mark.parametrize("index0", [0, (1 << 35) + 64], ids=["i0", "i2p35"])
@pytest.mark.parametrize("M,H", [(1, 8), (5, 72), (300, 64)])
def test_op_matches_restatement(M, H, index0, seed, call):
    """Every output element's bits, none excluded: one lane, a ragged last block, several blocks; the counter's high word;
    ids outside [0, V) (they read row 0 and still get noise)."""
    Vt = 37
    E_ = _table(Vt, H, seed=1)
    g = np.random.default_rng(M * H)
    ids = g.integers(0, Vt, M)
    ids[::3] = [(-1, Vt, Vt + 1000, -(1 << 40))[i % 4] for i in range(len(ids[::3]))]
    s = R.scale(5.0, 16, H)
    got, _ = _run_op(ids, E_, s, seed, call, index0)
    want = R.embed(ids, E_.numpy(), s, seed, call, index0)
    assert (got == want).all(), f"{int((got != want).sum())} of {M * H} elements differ"
    plain = R.bf16_bits(E_.numpy()[R.rows(ids, Vt)])
    assert (got != plain).mean() > 0.9  # mag 0.156 / sqrt(H / 64) against entries of std 0.02: the noise is in the bits
    # another call number and another seed give other bits; s = 0 gives the plain gather
    other, _ = _run_op(ids, E_, s, seed, (call + 1) & 0xFFFFFFFF, index0)
    assert (other == R.embed(ids, E_.numpy(), s, seed, (call + 1) & 0xFFFFFFFF, index0)).all() and (other != got).any()
    other, _ = _run_op(ids, E_, s, seed ^ (1 << 40), call, index0)
    assert (other == R.embed(ids, E_.numpy(), s, seed ^ (1 << 40), call, index0)).all() and (other != got).any()
    zero, _ = _run_op(ids, E_, 0.0, seed, call, index0)
    assert (zero == plain).all()


@pytest.mark.parametrize("explicit", [False, True], ids=["m_mod_T", "position_ids"])
@pytest.mark.parametrize("M,H", [(5, 72), (300, 64)])
def test_op_opt_form_matches_restatement(M, H, explicit):
    """out = bf16((E + P) + n): default positions m % T and explicit ones, clamped ones (below 0 and beyond the table) included."""
    Vt, NP, T = 37, 21, 7
    E_, P_ = _table(Vt, H, seed=1), _table(NP, H, seed=2)
    g = np.random.default_rng(M + H)
    ids = g.integers(-2, Vt + 2, M)
    pos = None
    if explicit:
        pos = g.integers(0, NP - 2, M)
        pos[::4] = [(-5, NP, 1 << 33, -3)[i % 4] for i in range(len(pos[::4]))]
    seed, call, index0 = 0xFEDC_BA98_7654_3210, 3, 8 * 1000
    s = R.scale(5.0, 16, H)
    got, prow = _run_op(ids, E_, s, seed, call, index0, P=P_, T=T, pos=pos)
    want = R.embed(ids, E_.numpy(), s, seed, call, index0, P=P_.numpy(), T=T, position_ids=pos)
    assert (got == want).all(), f"{int((got != want).sum())} of {M * H} elements differ"
    assert (prow == R.pos_rows(M, T, NP, pos)).all()  # the backward's scatter rows, as the unarmed launch writes them
    # and the unarmed OPT launch is what s = 0 gives
    zero, _ = _run_op(ids, E_, 0.0, seed, call, index0, P=P_, T=T, pos=pos)
    ids_d, pos_d = torch.as_tensor(ids).cuda(), (torch.as_tensor(pos).cuda() if pos is not None else None)
    out = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
    assert lib().slam_op_embed_pos_fwd(ptr(ids_d), ptr(pos_d), ptr(E_.to(torch.bfloat16).cuda()), ptr(P_.to(torch.bfloat16).cuda()),
                                       ptr(out), None, M, H, Vt, T, NP, stream()) == 0
    sync()
    assert (zero == _bits(out)).all()


# ------------------------------------------------------------------------------------------------------------------ models
def _model(tag, identity=False, max_tokens=1024, seed=7):
    """A tiny model of one family. identity: wo and wd (OPT: out_proj, fc2 and their biases) are zero, so every layer is the
    identity on the residual stream and forward(return logits) is head(norm(hs[0]))."""
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base, kw = FAMILIES[tag]
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=dict(base), vocab_size=V, max_tokens=max_tokens, **kw), seed=seed)
    g = torch.Generator().manual_seed(11)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "norm" in k:  # norms and biases that matter
            sd[k] = (v + 0.05 * torch.randn(v.shape, generator=g)).to(torch.bfloat16).float()
        if identity and any(t in k for t in ("o_proj.", "down_proj.", "out_proj.", "fc2.")):
            sd[k] = torch.zeros_like(v)
    m.load_state_dict(sd)
    return m


def _head_ref(m, hs0):
    """float64 head(norm(x)) of the rows x = hs0 [M, H] (float64 of bf16 values) and the issue's tolerance per logit:
    2 * (2^-9 |logit| + (2^-9 + H 2^-23) sum_i |y_i w_i|) - the norm output's and the logits' bf16 stores plus the fp32
    accumulation, doubled because the norm's own reductions are not modelled."""
    sd = {k: v.double() for k, v in m.state_dict(torch.float32).items()}
    x = torch.from_numpy(hs0)
    H = x.shape[1]
    if m.config.is_opt:
        d = "lm.model.decoder."
        eps = float(m.config.base_config["layer_norm_eps"])
        mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        y = (x - mu) / torch.sqrt(var + eps) * sd[d + "final_layer_norm.weight"] + sd[d + "final_layer_norm.bias"]
        W = sd[d + "embed_tokens.weight"]
    else:
        eps = float(m.config.base_config["rms_norm_eps"])
        y = x / torch.sqrt(x.pow(2).mean(1, keepdim=True) + eps) * sd["lm.model.norm.weight"]
        W = sd["lm.lm_head.weight"] if "lm.lm_head.weight" in sd else sd["lm.model.embed_tokens.weight"]
    logits = y @ W.t()
    tol = 2.0 * (2.0 ** -9 * logits.abs() + (2.0 ** -9 + H * 2.0 ** -23) * (y.abs() @ W.abs().t()))
    return logits, tol


def _ratio(err, tol):
    """max of err / tol; a column whose weights are all zero (the pad row of a tied table) has tol = 0 and must have err = 0."""
    assert bool((err[tol == 0] == 0).all())
    return float((err / tol.clamp_min(1e-300)).max())


def _tables(m):
    sd = m.state_dict(torch.float32)
    if m.config.is_opt:
        return sd["lm.model.decoder.embed_tokens.weight"].numpy(), sd["lm.model.decoder.embed_positions.weight"].numpy()
    return sd["lm.model.embed_tokens.weight"].numpy(), None


def _hs0(m, ids, s, seed, call, T):
    """float64 [M, H] of the restated armed embedding of the [B, T] batch `ids` (s = None: the plain one)."""
    Ew, Pw = _tables(m)
    flat = ids.reshape(-1).numpy()
    if s is None:
        s, seed, call = np.float32(0), 0, 0
    return R.bf16_to_f32(R.embed(flat, Ew, s, seed, call, 0, P=Pw, T=T)).astype(np.float64)


B0, T0, ALPHA = 16, 4, 5.0  # T H = 1024: mag = 5 / 32 against table entries of std 0.02


def _ids(B=B0, T=T0, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, V, (B, T), generator=g)
    ids[:, 0] = 1
    return ids


@pytest.mark.parametrize("tag", list(FAMILIES))
def test_engine_launch_equals_the_op(tag):
    m = _model(tag, identity=True)
    ids = _ids()
    H = m.config.base_config["hidden_size"]
    seed, call = 0x0BAD_CAFE_1234_5678, 41
    m.set_neftune(ALPHA, seed=seed)
    m.set_neftune_state(call=call)
    m.train()
    got = m(ids).logits.double().cpu().reshape(B0 * T0, V)
    s = R.scale(ALPHA, T0, H)
    ref, tol = _head_ref(m, _hs0(m, ids, s, seed, call, T0))
    err = (got - ref).abs()
    print(f"[neftune] {tag}: armed logits against head(norm(restated hs0)): max err / tol {_ratio(err, tol):.3f}")
    assert bool((err <= tol).all()), f"{int((err > tol).sum())} logits outside the tolerance"
    # power: the same logits against the NOISE-FREE hs0 miss by more than 8 tolerances - an unarmed launch cannot pass
    ref0, tol0 = _head_ref(m, _hs0(m, ids, None, 0, 0, T0))
    miss = _ratio((got - ref0).abs(), tol0)
    print(f"[neftune] {tag}: against the noise-free hs0: max err / tol {miss:.1f}")
    assert miss > 8.0
    # and the unarmed forward is the noise-free one
    m.eval()
    plain = m(ids).logits.double().cpu().reshape(B0 * T0, V)
    assert bool(((plain - ref0).abs() <= tol0).all())


def _fresh_pair(tag):
    return _model(tag), _model(tag)


@pytest.mark.parametrize("tag", ["qwen2", "qwen3", "opt"])
def test_arming(tag):
    m, untouched = _fresh_pair(tag)
    ids = _ids(B=4, T=64)
    labels = ids.clone()

    def fwd(model):
        out = model(ids, labels=labels)
        sync()
        return out.loss.clone(), out.logits.clone()

    base = fwd(untouched)
    m.set_neftune(ALPHA, seed=11)
    m.train()
    m.set_neftune_state(call=5)
    a = fwd(m)
    b = fwd(m)  # the call number counted up: 6
    m.set_neftune_state(call=5)
    c = fwd(m)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[1], base[1])
    m.set_neftune_state(call=6)
    d = fwd(m)
    assert torch.equal(b[0], d[0]) and torch.equal(b[1], d[1])
    m.set_neftune_state(seed=11 + (1 << 32), call=5)  # the high half of the seed is part of the key
    e = fwd(m)
    assert not torch.equal(a[1], e[1]) and not torch.equal(base[1], e[1])
    # eval(), the scoring paths in either mode and a forward after set_neftune(0): the bits of a model that never had the option
    m.eval()
    f = fwd(m)
    assert torch.equal(base[0], f[0]) and torch.equal(base[1], f[1])
    m.train()
    for mean in (False, True):
        assert torch.equal(untouched.log_likelihood(ids, mean_nll=mean), m.log_likelihood(ids, mean_nll=mean))
    lp0, lp1 = untouched.sequence_logps(ids, labels), m.sequence_logps(ids, labels)
    assert torch.equal(lp0[0], lp1[0]) and torch.equal(lp0[1], lp1[1])
    # a forward the engine refuses uses the arming up as well: the next, unarmed one must not inherit it
    m.engine.arm_neftune(4)
    assert lib().slam_forward(m.engine.h, None, None, None, None, None, 3, 128, 0.0, None, None, None) == -1
    m.eval()
    g = fwd(m)
    assert torch.equal(base[0], g[0]) and torch.equal(base[1], g[1])
    m.engine.arm_neftune(4)
    fake = ptr(ids.cuda())
    assert lib().slam_forward_unpadded(m.engine.h, fake, None, fake, 2, 64, 100, fake, 1 << 20, 0.0, None, None, None) == -1
    g = fwd(m)
    assert torch.equal(base[0], g[0]) and torch.equal(base[1], g[1])
    m.train()
    m.set_neftune(0)
    h = fwd(m)
    assert torch.equal(base[0], h[0]) and torch.equal(base[1], h[1])
    m.engine.arm_neftune(4)  # ignored while alpha is 0
    h = fwd(m)
    assert torch.equal(base[0], h[0]) and torch.equal(base[1], h[1])
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="neftune_noise_alpha"):
            m.set_neftune(bad)


@pytest.mark.parametrize("tag", ["qwen2", "qwen3"])
def test_generate_after_an_armed_forward_is_untouched(tag):
    m, untouched = _fresh_pair(tag)
    ids = _ids(B=2, T=24)
    am = torch.ones_like(ids)
    want = untouched.generate(ids, attention_mask=am, max_new_tokens=8, do_sample=False).cpu()
    m.set_neftune(ALPHA, seed=3)
    m.train()
    m(ids, labels=ids)
    got = m.generate(ids, attention_mask=am, max_new_tokens=8, do_sample=False).cpu()  # in train() mode: generation never draws noise
    assert torch.equal(want, got)
    cont = _ids(B=2, T=6, seed=9)
    assert torch.equal(untouched.score_continuations(ids, attention_mask=am, continuations=cont),
                       m.score_continuations(ids, attention_mask=am, continuations=cont))


def _grads(m):
    return {k: v.detach().float().cpu().clone() for k, v in m.named_grads()}


def _step(m, ids, call, **kw):
    m.set_neftune_state(call=call)
    m.zero_grad()
    out = m(ids, labels=ids, return_logits=False, **kw)
    m.backward()
    sync()
    return out.loss.clone(), _grads(m)


@pytest.mark.parametrize("tag", ["qwen2", "qwen3", "opt"])
def test_recompute_levels_same_bits(tag):
    """No level re-runs the embedding launch (the residual streams are kept): the same loss and gradient bits."""
    m = _model(tag)
    ids = _ids(B=3, T=64)
    m.train()
    plain, _ = _step(m, ids, 2)
    m.set_neftune(ALPHA, seed=3)
    l0, g0 = _step(m, ids, 2)
    assert not torch.equal(plain, l0)  # the noise is on
    for level in (1, 2):
        m.gradient_checkpointing_enable(level=level)  # rebinds the workspace: the option stays
        l, g = _step(m, ids, 2)
        assert torch.equal(l, l0), (level, float(l), float(l0))
        for k in g0:
            assert torch.equal(g[k], g0[k]), (level, k)


@pytest.mark.parametrize("tag", ["qwen2", "opt"])
def test_padding_free_indexes_the_packed_layout(tag):
    """slam_forward_unpadded: s from the padded width T, the element index from the packed rows that are launched."""
    m = _model(tag, identity=True)
    B, T, lens = 3, 40, [40, 23, 9]
    ids = _ids(B=B, T=T)
    mask = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    ids = ids.masked_fill(mask == 0, 0)
    H = m.config.base_config["hidden_size"]
    seed, call = 77, 9
    m.set_neftune(ALPHA, seed=seed)
    m.set_neftune_state(call=call)
    m.train()
    got = m(ids, attention_mask=mask, padding_free=True).logits.double().cpu()
    assert m._last_unpadded
    s = R.scale(ALPHA, T, H)
    Ew, Pw = _tables(m)
    packed = np.concatenate([ids[b, :n].numpy() for b, n in enumerate(lens)])
    pos = np.concatenate([np.arange(n) for n in lens])  # each row's positions restart at 0
    Mp = len(packed)
    hs0 = R.bf16_to_f32(R.embed(packed, Ew, s, seed, call, 0, P=Pw, T=Mp, position_ids=pos if Pw is not None else None))
    ref, tol = _head_ref(m, hs0.astype(np.float64))
    hs_plain = R.bf16_to_f32(R.embed(packed, Ew, np.float32(0), 0, 0, 0, P=Pw, T=Mp, position_ids=pos if Pw is not None else None))
    ref0, tol0 = _head_ref(m, hs_plain.astype(np.float64))
    got_rows = torch.cat([got[b, :n] for b, n in enumerate(lens)])
    err = (got_rows - ref).abs()
    print(f"[neftune] {tag} padding-free: max err / tol {_ratio(err, tol):.3f}, "
          f"against noise-free {_ratio((got_rows - ref0).abs(), tol0):.1f}")
    assert bool((err <= tol).all())
    assert _ratio((got_rows - ref0).abs(), tol0) > 8.0
    assert all(bool((got[b, n:] == 0).all()) for b, n in enumerate(lens))  # pad positions stay zeros


def test_trainer_resume_repeats_the_run(tmp_path):
    """GA 2, six optimizer steps with neftune_noise_alpha = 5: twice from scratch, and three steps + checkpoint + resume. The
    same parameter bits; another run than without the option; evaluate() is untouched by it."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    g = torch.Generator().manual_seed(1)
    rows = [{"input_ids": [1] + torch.randint(2, V, (40,), generator=g).tolist(), "attention_mask": [1] * 41} for _ in range(32)]
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)
    ev = TokenDataset(rows[:6])

    def run(out, resume=None, save_steps=0, alpha=ALPHA):
        m = _model("qwen2")
        a = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=2, max_steps=6, warmup_steps=1,
                                  warmup_ratio=0.0, logging_steps=1, save_steps=save_steps, output_dir=str(out),
                                  num_train_epochs=4, seed=13, neftune_noise_alpha=alpha, eval_strategy="no")
        tr = SLAMTrainer(model=m, args=a, data_collator=coll, train_dataset=ds, eval_dataset=ev)
        e0 = tr.evaluate()["eval_loss"]
        tr.train(resume_from_checkpoint=resume)
        assert m._neft_alpha == 0.0  # switched off when train() returned
        return m, tr, e0

    m_a, tr_a, e_a = run(tmp_path / "a", save_steps=3)
    m_b, tr_b, _ = run(tmp_path / "b")
    m_r, tr_r, _ = run(tmp_path / "r", resume=str(tmp_path / "a" / "checkpoint-3"))
    assert tr_r.state.global_step == 6
    sa, sb, sr = (x.state_dict(torch.float32) for x in (m_a, m_b, m_r))
    for k in sa:
        assert torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sr[k]), k
    m_p, tr_p, e_p = run(tmp_path / "p", alpha=None)
    sp = m_p.state_dict(torch.float32)
    assert any(not torch.equal(sa[k], sp[k]) for k in sa)  # the noise was part of the run
    assert e_a == e_p  # equal (initial) weights: evaluate() returns the same eval_loss with and without the option
    m_p.load_state_dict(sa)  # and on the trained weights, while the option is set on one of the two models
    tr_a.model.set_neftune(ALPHA, seed=1)
    tr_a.model.train()
    assert tr_a.evaluate()["eval_loss"] == tr_p.evaluate()["eval_loss"]
