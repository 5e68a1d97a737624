"""-m gpu: span batches - left- and both-side-padded attention masks (slam_forward_unpadded_spans, UnitLM.forward /
sequence_logps with a span mask or starts= / lengths=). The pack and scatter doors bit for bit against tests/span_ref.py; a span
batch against the same rows right-padded under padding_free, bit for bit (the same launches on the same packed arrays); parity
with the reference's fp32 outputs (tests/golden/span_mask.npz) at the bars of tests/test_gpu_padding_free.py (SURVEY.md section
8c: loss abs <= 2e-2, logits rel-RMS <= 2e-2, gradient norms within 3e-2); sequence_logps on generate's own output; one trainer
step; the refusals."""
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from slamkit_amd import engine as E
from tests import span_ref as S
from tests.gpu_util import check, sync

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]


def _scratch(B, T):
    nbytes = E.unpadded_scratch_bytes(B, T)
    raw = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    off = (-raw.data_ptr()) % 256
    return raw, off, raw[off:off + nbytes]


def _i32(x):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=torch.int32).cuda()


def _check_pack(ids, lab, starts, lens, Mp):
    B, T = ids.shape
    ref = S.pack(ids.numpy(), None if lab is None else lab.numpy(), starts, lens, Mp)
    raw, off, scratch = _scratch(B, T)
    E.unpad_pack_spans(ids.cuda(), None if lab is None else lab.cuda(), _i32(starts), _i32(lens), B, T, Mp, 0, scratch)
    sync()
    v = {k: t.cpu().numpy() for k, t in E.unpadded_scratch_views(scratch, B, T).items()}
    for k in ("ids", "position_ids", "seg_start", "seg_end", "row"):
        assert np.array_equal(v[k][:Mp], ref[k]), k
    assert np.array_equal(v["off"], ref["off"])
    if lab is not None:
        assert np.array_equal(v["labels"][:Mp], ref["labels"])
    else:
        assert (v["labels"] == CANARY).all()  # without labels the array is left alone
    assert (v["ids"][Mp:] == CANARY).all() and (raw[:off] == 0xA5).all() and (raw[off + scratch.numel():] == 0xA5).all()
    return ref, scratch


# ------------------------------------------------------------------------------------------------- pack and scatter doors
@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("B,T", [(1, 7), (3, 64), (257, 5), (300, 7)])  # 257 and 300 cross the 256-row scan chunk
def test_pack_door_equals_span_ref(B, T, tail, with_labels):
    g = torch.Generator().manual_seed(B * 131 + T)
    ids, lab = torch.randint(1, 502, (B, T), generator=g), torch.randint(1, 502, (B, T), generator=g)
    starts, lens = S.spans_for(B, T, seed=B + T)
    if B == 3:
        starts, lens = np.array([0, 47, 20]), np.array([64, 17, 1])  # right edge, left padding, one token in the middle
    mmax = -(-(B * T) // 64) * 64
    Mp = min(S.m_packed(lens) + 64, mmax) if tail else S.m_packed(lens)
    _check_pack(ids, lab if with_labels else None, starts, lens, Mp)


def test_pack_door_clamps_spans_that_break_their_contract():
    """starts to [0, T], lens to [0, T - starts]: nothing is read past its row, the rows behind keep their places."""
    g = torch.Generator().manual_seed(4)
    ids, lab = torch.randint(1, 502, (4, 64), generator=g), torch.randint(1, 502, (4, 64), generator=g)
    ref, _ = _check_pack(ids, lab, [40, 70, -3, 60], [40, 5, 100, 4], 256)
    assert ref["off"].tolist() == [0, 24, 24, 88, 92]


@pytest.mark.parametrize("B,T", [(3, 64), (300, 7)])
def test_null_starts_is_the_right_padded_pack_byte_for_byte(B, T):
    g = torch.Generator().manual_seed(9)
    ids, lab = torch.randint(1, 502, (B, T), generator=g), torch.randint(1, 502, (B, T), generator=g)
    _, lens = S.spans_for(B, T, seed=2)
    Mp = S.m_packed(lens)
    raws = []
    for how in ("plain", "null", "zeros"):
        raw, off, scratch = _scratch(B, T)
        if how == "plain":
            E.unpad_pack(ids.cuda(), lab.cuda(), _i32(lens), B, T, Mp, 0, scratch)
        else:
            E.unpad_pack_spans(ids.cuda(), lab.cuda(), None if how == "null" else _i32(np.zeros(B)), _i32(lens), B, T, Mp, 0, scratch)
        sync()
        raws.append(scratch.cpu())
    assert torch.equal(raws[0], raws[1]) and torch.equal(raws[0], raws[2])


@pytest.mark.parametrize("V", [502, 504])  # the element path and the 16-byte path
@pytest.mark.parametrize("B,T,broken", [(3, 64, False), (300, 7, False), (1, 7, False), (4, 64, True)])
def test_scatter_door_equals_span_ref(B, T, V, broken):
    if broken:
        starts, lens = np.array([40, 70, -3, 60]), np.array([40, 5, 100, 4])
    else:
        starts, lens = S.spans_for(B, T, seed=B * 7 + T)
    _, ln = S.clamp_spans(starts, lens, T)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    Mp = S.m_packed(ln)
    g = torch.Generator().manual_seed(V + B)
    src = torch.randn(Mp, 512, generator=g).to(torch.bfloat16)
    want = S.scatter_rows(src[:, :V].contiguous().view(torch.int16).numpy(), off, starts, B, T)
    dst = torch.full((B, T, V), 7.0, dtype=torch.bfloat16, device="cuda")
    E.unpad_logits_spans(src.cuda(), dst, _i32(off), _i32(starts), B, T, Mp)
    sync()
    got = dst.view(torch.int16).cpu().numpy()
    assert np.array_equal(got, want)
    real = np.zeros((B, T), bool)
    st, _ = S.clamp_spans(starts, lens, T)
    for b in range(B):
        real[b, st[b]:st[b] + ln[b]] = True
    assert (got[~real] == 0).all() and int(real.sum()) == int(off[-1])  # +0 bits at every masked position
    if not broken:  # starts = NULL is slam_op_unpad_logits
        a = torch.full((B, T, V), 7.0, dtype=torch.bfloat16, device="cuda")
        b_ = torch.full_like(a, 3.0)
        E.unpad_logits_spans(src.cuda(), a, _i32(off), None, B, T, Mp)
        assert E.load_library().slam_op_unpad_logits(src.cuda().data_ptr(), 512, b_.data_ptr(), V, _i32(off).data_ptr(), B, T, Mp,
                                                     E.current_stream_ptr()) == 0
        sync()
        assert torch.equal(a, b_)


# ---------------------------------------------------------------------------------------------------------------- models
def _span_batch(vocab, T, spans, seed):
    """ids / mask / labels [B, T] with row b's tokens in its span, and the same rows right-padded."""
    g = torch.Generator().manual_seed(seed)
    B = len(spans)
    ids, am, ids_r, am_r = (torch.zeros(B, T, dtype=torch.long) for _ in range(4))
    for b, (s, n) in enumerate(spans):
        row = torch.randint(2, vocab, (n,), generator=g)
        row[0] = 1
        ids[b, s:s + n], am[b, s:s + n] = row, 1
        ids_r[b, :n], am_r[b, :n] = row, 1
    lab = torch.where(am.bool(), ids, torch.full_like(ids, -100))
    lab_r = torch.where(am_r.bool(), ids_r, torch.full_like(ids_r, -100))
    return dict(input_ids=ids, attention_mask=am, labels=lab), dict(input_ids=ids_r, attention_mask=am_r, labels=lab_r)


def _step(m, batch, **kw):
    m.zero_grad()
    out = m(**batch, **kw)
    tokens = m.engine.last_forward_tokens()
    m.backward()
    sync()
    return out.loss.detach().clone(), out.logits.clone(), m.flat_grads.clone(), tokens


def _body(name):
    if name == "qwen2":
        from tests.test_gpu_model import _mk
        return _mk(O.TINY, O.init_weights(O.TINY, seed=5, bias_std=0.02, norm_jitter=0.05), max_tokens=512)
    if name == "opt":
        from tests.test_gpu_recompute import _opt
        return _opt(max_tokens=512)
    from tests.test_gpu_qwen3 import _unit_lm
    return _unit_lm("B", max_tokens=512)[0]


SPANS = [(0, 96), (29, 67), (40, 7), (95, 1)]  # full, left-padded, both sides, one token at the right edge: 171 tokens


@pytest.mark.parametrize("recompute", [0, 2])
@pytest.mark.parametrize("body", ["qwen2", "opt", "qwen3"])
def test_span_batch_is_the_right_padded_batch_bit_for_bit(body, recompute):
    m = _body(body)
    m.eval()  # (no dropout call numbering between the two runs)
    if recompute:
        m.gradient_checkpointing_enable(level=recompute)
    span, right = _span_batch(502, 96, SPANS, seed=3)
    with pytest.raises(ValueError, match="right-padded"):  # span masks are opt-in
        m(**span)
    a = _step(m, span, span_masks=True)  # padding_free is off: a span batch runs packed whatever that switch says
    assert m.padding_free is False and m.span_masks is False and a[3] == 192
    b = _step(m, right, padding_free=True)
    assert b[3] == 192
    assert torch.equal(a[0], b[0]) and bool(torch.isfinite(a[0]))
    va, vb = span["attention_mask"].bool(), right["attention_mask"].bool()
    assert torch.equal(a[1].cpu()[va], b[1].cpu()[vb])
    assert float(a[1].float().abs().cpu()[~va].max()) == 0.0 and int((~va).sum()) == 4 * 96 - 171
    assert torch.equal(a[2], b[2]) and float(a[2].abs().max()) > 0
    # device tensors with host starts / lengths: the same call
    dev = {k: v.cuda() for k, v in span.items() if k != "attention_mask"}
    c = _step(m, dev, starts=[s for s, _ in SPANS], lengths=torch.tensor([n for _, n in SPANS]))
    assert all(torch.equal(x, y) for x, y in zip(a[:3], c[:3])) and c[3] == 192
    # num_items_in_batch and no logits
    m.span_masks = True  # the model-wide switch instead of the argument
    n1 = m(**span, num_items_in_batch=50, return_logits=False)
    n2 = m(**right, num_items_in_batch=50, return_logits=False, padding_free=True)
    assert n1.logits is None and torch.equal(n1.loss.detach(), n2.loss.detach())


def _golden():
    return dict(np.load(os.path.join(GOLDEN, "span_mask.npz")))


@pytest.mark.parametrize("body", ["qwen2", "opt"])
def test_span_batch_matches_the_reference_golden(body, golden_data):
    """The reference's fp32 logits at the real positions, mean loss, loss with num_items_in_batch and per-tensor gradient norms
    of the 3 x 40 batch with spans (0, 40), (23, 17), (9, 12). OPT's k_proj.bias gradient is zero in exact arithmetic (softmax
    is invariant to a constant key shift) and is left out, as tests/test_gpu_padding_free.py leaves it out."""
    g = _golden()
    if body == "qwen2":
        from tests.test_gpu_model import _mk
        meta = golden_data["meta"]
        cfg = O.OracleConfig(**meta["config"])
        m = _mk(cfg, O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"]), max_tokens=512)
    else:
        from slamkit_amd.model import UnitLM
        m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_opt_ckpt"), max_tokens=512)
    ids, mask, labels = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels"))
    m.span_masks = True
    m.zero_grad()
    out = m(ids, attention_mask=mask, labels=labels)
    assert m.engine.last_forward_tokens() == 128  # 69 real tokens
    m.backward()
    sync()
    lg, real = out.logits.float().cpu(), mask.bool()
    assert lg.shape == (3, 40, 502)
    check(f"{body} logits vs the reference (fp32)", lg[real], torch.from_numpy(g[body + "_logits_real"]), 2e-2)
    assert float(lg[~real].abs().max()) == 0.0 and int((~real).sum()) == 51  # exact zeros at every masked position
    loss = float(out.loss.detach())
    print(f"{body} loss engine / reference: {loss} {float(g[body + '_loss'])}")
    assert abs(loss - float(g[body + "_loss"])) <= 2e-2
    grads = dict(m.named_grads())
    worst = 0.0
    for k, want in zip(g[body + "_grad_names"], g[body + "_grad_norms"]):
        k = str(k)
        if body == "opt" and k.endswith("k_proj.bias"):
            continue
        got = float(grads[k].norm())
        worst = max(worst, abs(got - want) / want)
        assert abs(got - want) <= 3e-2 * want + 1e-7, (k, got, want)
    print(f"{body} worst gradient-norm deviation {worst:.3e}")
    out2 = m(ids, attention_mask=mask, labels=labels, num_items_in_batch=100, return_logits=False)
    assert abs(float(out2.loss.detach()) - float(g[body + "_loss_num_items"])) <= 2e-2
    # labels that are not -100 at pad positions or at a row's first real token add nothing
    out3 = m(ids, attention_mask=mask, labels=ids.clone(), return_logits=False)
    assert torch.equal(out3.loss.detach(), out.loss.detach())
    if body == "opt":  # positions count from each row's first real token: no position row beyond the longest span is touched
        assert float(grads["lm.model.decoder.embed_positions.weight"][42:].abs().max()) == 0.0


def test_sequence_logps_on_generate_output():
    """generate returns left-padded prompts followed by continuations: sequence_logps on that batch with its mask equals
    score_continuations on the same rows."""
    from tests.test_gpu_generate import _mk, _tiny
    cfg, sd = _tiny()
    m = _mk(cfg, sd, max_tokens=512, seed=7)
    g = torch.Generator().manual_seed(23)
    lens, T, NEW = [37, 20, 5], 37, 12
    ids, am = torch.zeros(3, T, dtype=torch.long), torch.zeros(3, T, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, T - n:], am[b, T - n:] = torch.randint(2, cfg.vocab, (n,), generator=g), 1
    seq = m.generate(ids, attention_mask=am, max_new_tokens=NEW, eos_token_id=[], pad_token_id=0).cpu()
    assert seq.shape == (3, T + NEW) and torch.equal(seq[:, :T], ids)
    cont = seq[:, T:]
    want = m.score_continuations(ids, am, continuations=cont).cpu().double().sum(1).numpy()
    mask = torch.cat([am, torch.ones(3, NEW, dtype=torch.long)], 1)
    labels = torch.cat([torch.full((3, T), -100), cont], 1)
    with pytest.raises(ValueError, match="right-padded"):
        m.sequence_logps(seq, labels, attention_mask=mask)
    ll, cnt = m.sequence_logps(seq, labels, attention_mask=mask, span_masks=True)
    assert m.engine.last_forward_tokens() == 128  # 62 prompt + 36 new tokens, where the batch holds 3 x 49 positions
    assert cnt.tolist() == [float(NEW)] * 3
    print("sequence_logps / score_continuations:", ll.tolist(), want.tolist())
    assert np.allclose(ll.cpu().numpy(), want, rtol=5e-3, atol=2e-2)
    # device batch with starts / lengths: the same bits; and forward itself takes generate's output
    ll2, _ = m.sequence_logps(seq.cuda(), labels.cuda(), starts=[T - n for n in lens], lengths=[n + NEW for n in lens])
    assert torch.equal(ll2, ll)
    out = m(input_ids=seq, attention_mask=mask, labels=labels, span_masks=True)
    assert bool(torch.isfinite(out.loss)) and m.engine.last_forward_tokens() == 128


def test_trainer_step_from_a_left_padded_batch():
    """One SLAMTrainer.optimizer_step from a left-padded host batch against the right-padded step (dense route) from the same
    state: loss within 2e-2, every gradient norm within 3e-2; against the right-padded step under padding_free: the same bits."""
    from slamkit_amd.data import DataCollatorForLanguageModeling
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    from tests.test_gpu_train import _tiny_model
    sd = O.init_weights(O.TINY, seed=5, bias_std=0.02, norm_jitter=0.05)
    g = torch.Generator().manual_seed(2)
    rows = [{"input_ids": [1] + torch.randint(2, 502, (n - 1,), generator=g).tolist(), "attention_mask": [1] * n} for n in (70, 33, 9, 1)]
    right = DataCollatorForLanguageModeling(pad_token_id=0)(rows)
    left = {k: torch.stack([torch.roll(v[b], 70 - len(rows[b]["input_ids"])) for b in range(4)]) for k, v in right.items()}
    assert left["attention_mask"][1].tolist() == [0] * 37 + [1] * 33 and int(left["labels"][2, 60]) == -100
    res = {}
    for name, mb, pf in (("left", left, False), ("right", right, False), ("right_pf", right, True)):
        m = _tiny_model(sd)
        m.span_masks = True
        tr = SLAMTrainer(model=m, args=SLAMTrainingArguments(per_device_train_batch_size=4, max_steps=1, logging_steps=1, warmup_steps=0,
                                                             warmup_ratio=0.0, learning_rate=1e-3, output_dir="/tmp/unused", padding_free=pf))
        snap = {}
        update = tr._update
        tr._update = lambda lr, zero_grad: (snap.update(g={k: v.clone() for k, v in m.named_grads()},
                                                        tokens=m.engine.last_forward_tokens()), update(lr, zero_grad=zero_grad))
        m.zero_grad()
        tr.optimizer_step([mb], 1e-3)
        sync()
        res[name] = (float(tr._loss_acc), snap["g"], snap["tokens"], m.state_dict(torch.float32))
    assert res["left"][2] == 128 and res["right"][2] == 4 * 128 and res["right_pf"][2] == 128  # 113 real tokens
    print("trainer step loss left / right / right padding-free:", res["left"][0], res["right"][0], res["right_pf"][0])
    assert abs(res["left"][0] - res["right"][0]) <= 2e-2
    for k, gv in res["left"][1].items():
        want = float(res["right"][1][k].norm())
        assert abs(float(gv.norm()) - want) <= 3e-2 * want + 1e-7, k
        assert torch.equal(gv, res["right_pf"][1][k]), k
    assert res["left"][0] == res["right_pf"][0]
    for k, v in res["left"][3].items():  # and the updated weights
        assert torch.equal(v, res["right_pf"][3][k]), k


def test_refusals():
    from tests.test_gpu_model import _mk
    m = _mk(O.TINY, None, max_tokens=256)
    ids = torch.randint(2, 502, (2, 8), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="right-padded"):  # off by default: what it always raised
        m(input_ids=ids, attention_mask=torch.tensor([[1] * 8, [0, 0, 0, 1, 1, 1, 1, 1]]), labels=ids)
    m.span_masks = True
    for pf in (False, True):
        with pytest.raises(ValueError, match="hole"):
            m(input_ids=ids, attention_mask=torch.tensor([[1] * 8, [1, 1, 0, 1, 1, 0, 0, 0]]), labels=ids, padding_free=pf)
        with pytest.raises(ValueError, match="all zeros"):
            m(input_ids=ids, attention_mask=torch.tensor([[1] * 8, [0] * 8]), labels=ids, padding_free=pf)
    left = torch.tensor([[1] * 8, [0, 0, 0, 1, 1, 1, 1, 1]])
    pos = torch.arange(8)[None].expand(2, 8).contiguous()
    with pytest.raises(ValueError, match="position_ids"):
        m(input_ids=ids, attention_mask=left, position_ids=pos, labels=ids)
    with pytest.raises(ValueError, match="position_ids"):
        m(input_ids=ids, position_ids=pos, labels=ids, starts=[0, 3], lengths=[8, 5])
    with pytest.raises(ValueError, match="host"):
        m(input_ids=ids, labels=ids, starts=torch.tensor([0, 3]).cuda(), lengths=[8, 5])
    with pytest.raises(ValueError, match="span batch"):
        m(input_ids=ids, labels=ids, starts=[0, 4], lengths=[8, 5])
    with pytest.raises(ValueError, match="hole"):
        m.sequence_logps(ids, ids, attention_mask=torch.tensor([[1] * 8, [1, 0, 1, 1, 1, 1, 1, 1]]))
    # a device mask is still not read back: taken as right padding, the dense route
    m(input_ids=ids.cuda(), attention_mask=left.cuda(), labels=ids.cuda(), return_logits=False)
    assert m.engine.last_forward_tokens() == 128 and m._last_unpadded is False  # 2 rows of 8, rounded up to 64 each
    # and a right-padded host mask keeps its routes: dense without the switch, packed with it
    right = torch.tensor([[1] * 8, [1, 1, 1, 1, 1, 0, 0, 0]])
    m(input_ids=ids, attention_mask=right, labels=ids, return_logits=False)
    assert m.engine.last_forward_tokens() == 128 and m._last_unpadded is False
    m(input_ids=ids, attention_mask=right, labels=ids, return_logits=False, padding_free=True)
    assert m.engine.last_forward_tokens() == 64 and m._last_unpadded is True
    sync()
