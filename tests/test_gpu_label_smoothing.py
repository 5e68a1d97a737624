"""-m gpu: label smoothing inside the loss kernels (slam_set_label_smoothing, UnitLM.forward(label_smoothing=),
SLAMTrainingArguments.label_smoothing_factor) against tests/label_smoothing_ref.py - HF's LabelSmoother restated, itself held to
HF's own output by tests/test_label_smoothing_host.py.

Op level: the bars of tests/test_gpu_ops.py::test_cross_entropy (same shape, same single bf16 store of the gradient). Engine
level: the bars of tests/test_gpu_model.py for the plain loss on the same configs (loss 5e-3 abs against the oracle on the same
bf16 weights, gradient cosine 0.999 / 0.99 and norm within 3 %), and those of tests/test_gpu_padding_free.py between the padded
and the padding-free run (loss 2e-2)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import label_smoothing_ref as R
from tests.gpu_util import check, cosine, dev_bf16, lib, ptr, rnd, stream, sync

pytestmark = pytest.mark.gpu

B_OP, T_OP = 3, 41  # test_cross_entropy's shape: 123 rows = 31 blocks of the one-wave-per-row kernel, the last one partial
# (502, 512) / (512, 512): the wave kernel with and without pad columns; (700, 768): the block kernel, a short strided loop (96
# chunks over 256 threads) and 68 pad columns; (5003, 5120): more than one chunk per thread, V not a multiple of 8
SHAPES = [(502, 512), (512, 512), (700, 768), (5003, 5120)]


@functools.lru_cache(maxsize=None)
def _op_inputs(V, Vp):
    M = B_OP * T_OP
    logits = rnd(M, Vp, seed=1, scale=3.0)  # bf16-representable: the reference sees the logits the kernel reads
    labels = torch.randint(0, V, (B_OP, T_OP), generator=torch.Generator().manual_seed(2))
    labels[0, 5:9] = -100
    labels[2, 30:] = -100
    labels[0, 1], labels[1, 1] = 0, V - 1  # rows 0 and 41: targets in the first and in the last real column
    return logits, labels


@functools.lru_cache(maxsize=None)
def _op_ref(V, Vp, num_items, eps):
    logits, labels = _op_inputs(V, Vp)
    return R.label_smoothing(logits[:, :V].view(B_OP, T_OP, V).numpy(), labels.numpy(), eps, num_items if num_items > 0 else None)


def _run_op(lg, labd, num_items, eps, V, Vp, alias, entry="smooth"):
    M = B_OP * T_OP
    src = lg.clone() if alias else lg
    dl = src if alias else torch.full((M, Vp), float("nan"), dtype=torch.bfloat16, device="cuda")
    rl = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    rs = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    sc = torch.zeros(2, dtype=torch.float32, device="cuda")
    if entry == "plain":
        rc = lib().slam_op_cross_entropy(ptr(src), ptr(labd), float(num_items), ptr(dl), ptr(rl), ptr(sc), B_OP, T_OP, Vp, V, stream())
    else:
        rc = lib().slam_op_cross_entropy_smooth(ptr(src), ptr(labd), float(num_items), ptr(dl), ptr(rl), ptr(rs), ptr(sc), B_OP,
                                                T_OP, Vp, V, eps, stream())
    sync()
    assert rc == 0
    return dl, rl, rs, sc


@pytest.mark.parametrize("alias", [True, False], ids=["inplace", "separate"])
@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("num_items", [0, 57])
@pytest.mark.parametrize("V,Vp", SHAPES)
def test_cross_entropy_smooth_op(V, Vp, num_items, eps, alias):
    logits, labels = _op_inputs(V, Vp)
    ref = _op_ref(V, Vp, num_items, eps)
    lg, labd = dev_bf16(logits), labels.cuda()
    dl, rl, rs, sc = _run_op(lg, labd, num_items, eps, V, Vp, alias)
    loss = float(ref["loss"])
    print(f"[parity] smoothed loss {float(sc[1]):.7f} ref {loss:.7f} denom {float(sc[0])} ref {ref['denom']}")
    assert float(sc[0]) == ref["denom"]
    assert abs(float(sc[1]) - loss) <= 2e-5 * max(1.0, abs(loss))
    got = dl.float().cpu().view(B_OP, T_OP, Vp)
    check("smoothed ce dlogits", got[:, :, :V], torch.from_numpy(ref["grad"]), 5e-3, 2e-2)
    if Vp > V:  # eps / V never leaks into the pad columns
        assert float(got[:, :, V:].abs().max()) == 0.0
    valid = torch.from_numpy(ref["valid"])
    assert int(valid.sum()) == B_OP * (T_OP - 1) - 4 - 11 and not valid[:, -1].any()
    rl_c, rs_c = rl.cpu().view(B_OP, T_OP), rs.cpu().view(B_OP, T_OP)
    # ignored rows: all-zero gradient, zero in both row arrays
    assert float(got[~valid].abs().max()) == 0.0 and float(rl_c[~valid].abs().max()) == 0.0 and float(rs_c[~valid].abs().max()) == 0.0
    # the per-row arrays: fp32 lse and an fp32 row sum against float64 - the relative bar of the loss itself, per row
    for name, g_, r_ in (("row_loss", rl_c, ref["nll"]), ("row_smooth", rs_c, ref["smooth"])):
        d = (g_.double() - torch.from_numpy(r_)).abs()
        assert bool((d <= 2e-5 * torch.from_numpy(r_).abs().clamp(min=1.0)).all()), (name, float(d.max()))
    # row_loss stays the PLAIN nll, bit for bit what the plain entry writes
    dl0, rl0, _, sc0 = _run_op(lg, labd, num_items, 0.0, V, Vp, alias, entry="plain")
    assert torch.equal(rl, rl0)
    # eps = 0 through the new entry is the plain launch: same bits everywhere
    dlz, rlz, _, scz = _run_op(lg, labd, num_items, 0.0, V, Vp, alias)
    assert torch.equal(dlz, dl0) and torch.equal(rlz, rl0) and torch.equal(scz, sc0)
    assert not torch.equal(dl, dl0) and float(sc[1]) != float(sc0[1])
    # a second run of the same call: identical bits
    dl2, rl2, rs2, sc2 = _run_op(lg, labd, num_items, eps, V, Vp, alias)
    assert torch.equal(dl2, dl) and torch.equal(rl2, rl) and torch.equal(rs2, rs) and torch.equal(sc2, sc)


# ------------------------------------------------------------------------------------------------------------------ engine level
EPS = 0.1


def _oracle_smoothed(cfg, sd_bf, ids, lab, am, eps):
    """oracle.forward_loss_grads with the smoothed loss in place of compute_loss: the oracle's forward (model_forward's stack,
    with nn.Embedding's padding_idx as forward_loss_grads has it), fp32 logits, autograd."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd_bf.items()}
    Em = params["lm.model.embed_tokens.weight"]
    pad = cfg.pad_token_id if (cfg.pad_token_id is not None and cfg.pad_token_id >= 0) else None
    logits = O.decoder_stack(cfg, params, F.embedding(ids, Em, padding_idx=pad), Em, am, None, False, False)
    loss = R.label_smoothing_torch(logits.float(), lab, eps)
    loss.backward()
    return loss.detach(), {k: v.grad.detach() for k, v in params.items()}


def _plain_run(m, ids, am, lab, **kw):
    m.zero_grad()
    out = m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False, **kw)
    m.backward()
    sync()
    return out.loss.detach().clone(), m.flat_grads.clone()


def _make(kind, golden_data, golden_npz, wide_golden):
    from tests.test_gpu_model import _mk
    if kind == "tiny":  # V 502: padded vocabulary 512, the one-wave-per-row kernel
        meta = golden_data["meta"]
        cfg = O.OracleConfig(**meta["config"])
        sd = O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"])
        g = golden_npz
    else:  # the tests' wide config, V 700: padded vocabulary beyond 512, the block-per-row kernel
        g, cfgd, seed, bias_std, jit = wide_golden
        cfg = O.OracleConfig(**cfgd)
        sd = O.init_weights(cfg, seed=seed, bias_std=bias_std, norm_jitter=jit)
    sd_bf = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    ids, am, lab = (torch.from_numpy(g[k]) for k in ("pad_ids", "pad_mask", "pad_labels"))
    m = _mk(cfg, sd)
    assert (m.engine.padded_vocab() == 512) == (kind == "tiny")
    never = _plain_run(m, ids, am, lab)  # before anything sets a smoothing value on this engine
    ref = _oracle_smoothed(cfg, sd_bf, ids, lab, am, EPS)
    return dict(cfg=cfg, m=m, ids=ids, am=am, lab=lab, ref=ref, never=never)


@pytest.fixture(scope="module")
def models(golden_data, golden_npz, wide_golden):
    """Per config: model, golden padded batch, the oracle's smoothed loss / gradients and the plain run's bits - computed once,
    shared, never modified."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = _make(kind, golden_data, golden_npz, wide_golden)
        return cache[kind]

    return get


def _grad_bars(named_grads, grads_ref):
    worst = 1.0
    for k, gv in named_grads:
        ref = grads_ref[k]
        c = cosine(gv, ref)
        worst = min(worst, c)
        small = k.endswith(".bias") or k.endswith("norm.weight")
        assert c >= (0.99 if small else 0.999), f"{k}: cosine {c:.5f}"
        assert abs(float(gv.norm()) / float(ref.norm()) - 1) <= 3e-2, k
    print("worst gradient cosine", worst)


@pytest.mark.parametrize("kind", ["tiny", "wide"])
def test_forward_backward_vs_oracle_padded_and_padding_free(models, kind):
    s = models(kind)
    m, ids, am, lab = s["m"], s["ids"], s["am"], s["lab"]
    loss_ref, grads_ref = s["ref"]
    loss, grads = _plain_run(m, ids, am, lab, label_smoothing=EPS)
    print(f"[parity] {kind}: smoothed loss engine {float(loss):.5f} oracle {float(loss_ref):.5f} plain {float(s['never'][0]):.5f}")
    assert abs(float(loss) - float(loss_ref)) <= 5e-3
    assert not torch.equal(loss, s["never"][0]) and not torch.equal(grads, s["never"][1])
    _grad_bars(m.named_grads(), grads_ref)
    Vp, H = m.engine.padded_vocab(), s["cfg"].hidden
    Eg = m.flat_grads[: Vp * H].view(Vp, H)
    assert float(Eg[s["cfg"].vocab:].abs().max()) == 0.0  # pad rows of the tied embedding image: nothing leaked through the head
    # the same bits again
    loss2, grads2 = _plain_run(m, ids, am, lab, label_smoothing=EPS)
    assert torch.equal(loss, loss2) and torch.equal(grads, grads2)
    # the padding-free run of the same batch
    loss_pf, _ = _plain_run(m, ids, am, lab, label_smoothing=EPS, padding_free=True)
    assert m._last_unpadded and m.engine.last_forward_tokens() == -(-int(am.sum()) // 64) * 64  # the pads were not run
    assert abs(float(loss_pf) - float(loss)) <= 2e-2 and abs(float(loss_pf) - float(loss_ref)) <= 5e-3
    _grad_bars(m.named_grads(), grads_ref)
    # reduction by num_items_in_batch: the same sums over another denominator
    n = int((lab[:, 1:] != -100).sum())
    out = m(input_ids=ids, attention_mask=am, labels=lab, num_items_in_batch=2 * n, return_logits=False, label_smoothing=EPS)
    assert abs(float(out.loss.detach()) - float(loss) / 2) <= 1e-5
    # setting 0 again: the bits of an engine that never set it
    loss0, grads0 = _plain_run(m, ids, am, lab)
    assert torch.equal(loss0, s["never"][0]) and torch.equal(grads0, s["never"][1])
    loss0, grads0 = _plain_run(m, ids, am, lab, label_smoothing=0.0)
    assert torch.equal(loss0, s["never"][0]) and torch.equal(grads0, s["never"][1])


@pytest.mark.parametrize("kind", ["tiny", "wide"])
def test_row_likelihoods_and_refusals_after_a_smoothed_forward(models, kind):
    s = models(kind)
    m, ids, am, lab = s["m"], s["ids"], s["am"], s["lab"]
    B = ids.shape[0]
    f32 = lambda n=B: torch.empty(n, dtype=torch.float32, device="cuda")  # noqa: E731

    def loglik(eps, pf):
        m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False, label_smoothing=eps, padding_free=pf)
        ll, cnt = f32(), f32()
        if pf:
            m.engine.seq_loglik_unpadded(B, ll, cnt)
        else:
            held = m._hold[1]  # the labels the engine ran on (token axis padded to a multiple of 64)
            m.engine.seq_loglik(held, held.shape[0], held.shape[1], ll, cnt)
        sync()
        return ll, cnt

    for pf in (False, True):
        ll0, c0 = loglik(0.0, pf)
        ll1, c1 = loglik(EPS, pf)
        assert torch.equal(ll0, ll1) and torch.equal(c0, c1) and float(ll0.abs().min()) > 0  # row_loss is the plain nll
        # ... and the sequence-objective scaling of that forward is refused
        with pytest.raises(E.EngineError, match=r"\(-2\).*label-smoothed"):
            if pf:
                m.engine.scale_loss_unpadded(torch.ones(B, device="cuda"), B)
            else:
                m.engine.scale_loss_rows(torch.ones(B, device="cuda"), B, m._hold[1].shape[1])
    # log_likelihood / sequence_logps always run the plain loss, whatever the last forward set
    base = m.log_likelihood(ids, False).clone()
    m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False, label_smoothing=EPS)
    assert torch.equal(m.log_likelihood(ids, False), base)
    m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False, label_smoothing=EPS)
    m.sequence_logps(ids, lab)
    coef = torch.ones(B, device="cuda")
    m.engine.scale_loss_rows(coef, B, ids.shape[1])  # legal again: that forward was a plain one
    sync()
    # a logit mask and smoothing together: refused, and the mask-free smoothed forward still runs afterwards
    mask = torch.zeros(m.engine.padded_vocab(), dtype=torch.uint8, device="cuda")
    mask[5] = 1
    m.engine.set_logit_mask(mask)
    try:
        with pytest.raises(E.EngineError, match=r"\(-2\).*logit mask"):
            m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False, label_smoothing=EPS)
        with pytest.raises(E.EngineError, match=r"\(-2\).*logit mask"):
            m(input_ids=ids, attention_mask=am, labels=lab, return_logits=False, label_smoothing=EPS, padding_free=True)
        m(input_ids=ids, attention_mask=am, return_logits=False, label_smoothing=EPS)  # without labels there is no loss to smooth
    finally:
        sync()
        m.engine.set_logit_mask(None)
    loss, _ = _plain_run(m, ids, am, lab, label_smoothing=EPS)
    assert abs(float(loss) - float(s["ref"][0])) <= 5e-3
    loss0, grads0 = _plain_run(m, ids, am, lab)
    assert torch.equal(loss0, s["never"][0]) and torch.equal(grads0, s["never"][1])


# ----------------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_label_smoothing_factor(golden_data, tmp_path):
    """Three optimizer steps with gradient accumulation 2 on the tiny model: the first logged loss is the sum of the two
    micro-batches' forward(label_smoothing=0.1) losses under the step's num_items_in_batch; evaluate() reports the smoothed loss;
    with the factor at 0 (explicitly, on a model whose engine smoothed before) every loss has the bits of a run that never heard
    of the field."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, TokenDataset
    from slamkit_amd.data.hf_dataset import split_into_chunks
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from slamkit_amd.trainer.dp import seeded_batches
    from tests.test_gpu_train import _tiny_model
    rows = []
    for r in golden_data["G1_tokens"]:
        enc = O.unit_tokenise(r["audio_repr"])
        rows += [{"input_ids": c, "attention_mask": [1] * len(c)} for c in split_into_chunks(enc["input_ids"], 96)]
    assert len(rows) == 8
    ds, coll = TokenDataset(rows), DataCollatorForLanguageModeling(pad_token_id=0)
    sd = O.init_weights(O.TINY, seed=5, bias_std=0.02, norm_jitter=0.05)
    common = dict(per_device_train_batch_size=2, gradient_accumulation_steps=2, max_steps=3, num_train_epochs=4, warmup_steps=1,
                  warmup_ratio=0.0, learning_rate=2e-3, logging_steps=1, save_steps=0, seed=7, per_device_eval_batch_size=4)

    def run(out, warm=False, **kw):
        m = _tiny_model(sd)
        if warm:  # the engine has smoothed before the trainer gets it
            mb = coll([ds[0], ds[1]])
            m(input_ids=mb["input_ids"], labels=mb["labels"], return_logits=False, label_smoothing=0.3)
        tr = SLAMTrainer(model=m, args=SLAMTrainingArguments(output_dir=str(out), **common, **kw), data_collator=coll,
                         train_dataset=ds, eval_dataset=ds)
        st = tr.train()
        return m, tr, [r["loss"] for r in st.log_history if "loss" in r], tr.evaluate()["eval_loss"]

    m_s, tr_s, l_s, e_s = run(tmp_path / "s", label_smoothing_factor=EPS)
    _, _, l_p, e_p = run(tmp_path / "p")
    _, _, l_z, e_z = run(tmp_path / "z", warm=True, label_smoothing_factor=0.0)
    print("smoothed", l_s, e_s, "\nplain   ", l_p, e_p)
    assert len(l_s) == len(l_p) == len(l_z) == 3
    assert l_z == l_p and e_z == e_p  # bit for bit
    assert all(a != b for a, b in zip(l_s, l_p)) and e_s != e_p
    # step 1 by hand, on a fresh model with the same weights
    m = _tiny_model(sd)
    micro = [coll([ds[i] for i in b]) for b in seeded_batches(len(ds), 2, 7, 0)[:2]]
    n_items = float(sum(int((mb["labels"] != -100).sum()) for mb in micro))
    acc = torch.zeros(1, dtype=torch.float32, device=m.device)
    with torch.no_grad():
        for mb in micro:
            acc += m(input_ids=mb["input_ids"], attention_mask=mb["attention_mask"], labels=mb["labels"],
                     num_items_in_batch=n_items, return_logits=False, label_smoothing=EPS).loss
    assert float(acc) == l_s[0], (float(acc), l_s[0])
    # ... and against the float64 formula on the logits the engine hands out - the bf16 values its loss kernel read: the
    # op-level bar
    tot = 0.0
    with torch.no_grad():
        for mb in micro:
            lg = m(input_ids=mb["input_ids"], attention_mask=mb["attention_mask"]).logits.float().cpu().numpy()
            r = R.label_smoothing(lg, mb["labels"].numpy(), EPS, n_items)
            tot += float(r["loss"])
    assert abs(tot - l_s[0]) <= 2e-5 * max(1.0, tot)
    # evaluate(): the smoothed loss of the trained model, batch by batch as evaluate() sums it
    tot, cnt = torch.zeros(1, dtype=torch.float64, device=m_s.device), 0.0
    with torch.no_grad():
        for i in range(0, len(ds), 4):
            mb = coll([ds[j] for j in range(i, min(i + 4, len(ds)))])
            tot += m_s(input_ids=mb["input_ids"], labels=mb["labels"], num_items_in_batch=1.0, return_logits=False,
                       label_smoothing=EPS).loss.double()
            cnt += float((mb["labels"][:, 1:] != -100).sum())
    assert float(tot) / cnt == e_s
