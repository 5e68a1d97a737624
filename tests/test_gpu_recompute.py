"""-m gpu: activation recomputation in backward (engine option "recompute", UnitLM.gradient_checkpointing_enable).

The central claim is derived, not measured: backward re-runs the forward's own deterministic kernels on the forward's own
inputs, so every result at level 1 (selective) and level 2 (full layer) is BIT-IDENTICAL to level 0 under the same options.
Everything here compares with torch.equal; the one tolerance-based test is the independent anchor against the CPU oracle,
which restates the bars tests/test_gpu_model.py applies to the same fixture."""
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests.gpu_util import check, cosine, rel_err, sync

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 6 layers of head_dim 64 (bias + RoPE fused into the QKV projection; the three slots wrap twice), 4 layers of head_dim 128
# (separate RoPE launch), the tiny 2-layer shape with an untied head (fewer layers than slots), 5 OPT layers
Q6 = O.OracleConfig(n_layers=6, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, intermediate=512)
W4 = O.OracleConfig(n_layers=4, hidden=256, n_heads=2, n_kv_heads=1, head_dim=128, intermediate=512, vocab=700, rope_theta=1e6)
OPT5 = dict(model_type="opt", num_hidden_layers=5, hidden_size=256, num_attention_heads=4, ffn_dim=512,
            max_position_embeddings=256, init_std=0.02)
LEVELS = (1, 2)


def _qwen(cfg, sd=None, max_tokens=1024, untied=False, seed=3):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base = dict(num_hidden_layers=cfg.n_layers, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads,
                num_key_value_heads=cfg.n_kv_heads, head_dim=cfg.head_dim, intermediate_size=cfg.intermediate,
                rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, tie_word_embeddings=not untied)
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=max_tokens), seed=seed)
    if sd is not None:
        m.load_state_dict(sd)
    return m


def _opt(max_tokens=1024):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    m = UnitLM(UnitLMConfig(base_model_name="local-opt", base_config=dict(OPT5), vocab_size=502, max_tokens=max_tokens), seed=7)
    g = torch.Generator().manual_seed(11)  # HF's init has unit norms and zero biases: make them count
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or "layer_norm" in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


def _perturbed(m, seed=11):
    """Non-zero q / k / v biases and non-unit norms for a randomly initialised Qwen2 body."""
    g = torch.Generator().manual_seed(seed)
    sd = m.state_dict(torch.float32)
    for k, v in sd.items():
        if k.endswith(".bias") or k.endswith("norm.weight"):
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd)
    return m


BODIES = {
    "qwen6_hd64": lambda: _perturbed(_qwen(Q6)),
    "qwen4_hd128": lambda: _perturbed(_qwen(W4)),
    "untied_tiny": lambda: _perturbed(_qwen(O.TINY, untied=True)),
    "opt5": _opt,
}


def _dense(vocab, seed=0, B=3, T=96):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, vocab, (B, T), generator=g)
    ids[:, 0] = 1
    am = torch.ones(B, T, dtype=torch.long)
    for b, n in enumerate((T, T - 29, 7)[:B]):
        am[b, n:] = 0
    ids = ids * am
    lab = torch.where(am.bool(), ids, torch.full_like(ids, -100))
    return dict(input_ids=ids, attention_mask=am, labels=lab)


def _packed(vocab, seed=1, lens=(100, 37, 130, 5, 64)):
    g = torch.Generator().manual_seed(seed)
    ids, pos, lab = [], [], []
    for n in lens:
        t = torch.randint(2, vocab, (n,), generator=g)
        t[0] = 1
        l = t.clone()
        l[0] = -100
        ids.append(t), pos.append(torch.arange(n)), lab.append(l)
    cat = lambda xs: torch.cat(xs)[None]  # noqa: E731
    return dict(input_ids=cat(ids), position_ids=cat(pos), labels=cat(lab))


def _level(m, level):
    if level:
        m.gradient_checkpointing_enable(level=level)
    else:
        m.gradient_checkpointing_disable()
    assert m.is_gradient_checkpointing == bool(level)


def _step(m, batch):
    m.zero_grad()
    out = m(**batch)
    m.backward()
    sync()
    return out.loss.detach().clone(), out.logits.clone(), m.flat_grads.clone()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("loss", "logits", "grads")):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} of {x.numel()} values"


# the background K-split plans of the two-stream backward pinned to the one-stream ones (as tests/test_gpu_opt.py and
# tests/test_gpu_model.py do), so that the stream layouts can also be compared with each other
PINS = (("gemm_tn_bal_bg_max_split", 8), ("gemm_tn224_bg_min_m", 1 << 30), ("gemm_nt224", 0))


@pytest.mark.parametrize("body", list(BODIES))
def test_levels_are_bit_identical_to_level0(body):
    """Loss, logits and every gradient at levels 1 and 2 against level 0: dense and packed batches, the weight-gradient
    stream and the auxiliary side launches on and off, the SwiGLU fused into the gate|up projection and not."""
    m = BODIES[body]()
    for k, v in PINS:
        m.engine.set_option(k, v)
    vocab = m.config.vocab_size
    batches = {"dense": _dense(vocab), "packed": _packed(vocab)}
    for bname, batch in batches.items():
        for fuse in (0, 1):
            m.engine.set_option("fuse_swiglu", fuse)
            across = None
            for two, aux in ((1, 1), (1, 0), (0, 1), (0, 0)):
                m.engine.set_option("bwd_wgrad_stream", two)
                m.engine.set_option("bwd_aux_side", aux)
                _level(m, 0)
                ref = _step(m, batch)
                assert bool(torch.isfinite(ref[2]).all()) and float(ref[2].abs().max()) > 0
                _same(ref, _step(m, batch), f"{body} {bname}: level 0 repeat")
                for level in LEVELS:
                    _level(m, level)
                    tag = f"{body} {bname} fuse_swiglu={fuse} wgrad_stream={two} aux_side={aux} level={level}"
                    _same(ref, _step(m, batch), tag)
                    _same(ref, _step(m, batch), tag + " (second step)")  # back to back: the slots of one step against the next
                if across is None:
                    across = ref
                _same(across, ref, f"{body} {bname}: stream layouts against each other (pinned plans)")


@pytest.mark.parametrize("body", ["qwen6_hd64", "opt5"])
def test_accumulation_and_final_bf16_image(body):
    """Two accumulated micro-batches (the second backward adds), then the same step with the last backward final in bf16:
    the gradients, the image, both outputs of slam_grad_norm and the parameters after one AdamW step."""
    m = BODIES[body]()
    vocab = m.config.vocab_size
    mbs = [_dense(vocab, seed=4), _packed(vocab, seed=5)]
    n_items = float(sum(int((b["labels"][:, 1:] != -100).sum()) for b in mbs))
    p0 = m.flat_params.clone()
    pt0 = m.flat_params_t.clone() if m.flat_params_t is not None else None

    def run(level, final):
        _level(m, level)
        m.flat_params.copy_(p0)
        if pt0 is not None:
            m.flat_params_t.copy_(pt0)
        for i, b in enumerate(mbs):
            if i == 0:
                m.engine.set_option("grad_overwrite_next", 1)
            m(**b, num_items_in_batch=n_items, return_logits=False)
            m.backward(1.0, final=final if i == len(mbs) - 1 else 0)
        norm = torch.zeros(2, device="cuda")
        m.engine.grad_norm(0.5, norm)
        sync()
        out = [m.flat_grads.clone(), norm.clone()]
        if final == 2:
            out.append(m.flat_grads16.clone())
            ea, es = (torch.zeros(m.engine.n_params, dtype=torch.bfloat16, device="cuda") for _ in range(2))
            m.engine.adamw_step_bf16(ea, es, norm, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, zero_grad=False)
            sync()
            out += [m.flat_params.clone(), ea, es]
        return out

    for final in (0, 1, 2):
        ref = run(0, final)
        for level in LEVELS:
            got = run(level, final)
            for i, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(a, b), (body, final, level, i)
    m.flat_params.copy_(p0)


def test_level2_gradients_vs_oracle_on_the_tiny_fixture(golden_data, golden_npz):
    """The independent anchor: level-2 loss, logits and gradients on tests/golden/tiny_model.npz against the CPU oracle, with
    the checks and bars of tests/test_gpu_model.py::test_padded_batch_grads_vs_oracle (loss abs <= 5e-3, logits rel-RMS <=
    1e-2, gradient cosine >= 0.999 / >= 0.99 for bias and norm vectors, norm ratio within 3e-2, >= 0.99 against the
    reference-produced gradients, padded embedding rows exactly zero)."""
    meta = golden_data["meta"]
    cfg = O.OracleConfig(**meta["config"])
    sd = O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"])
    sd_bf = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    m = _qwen(cfg, sd, max_tokens=4096)
    g = golden_npz
    ids, am, lab = (torch.from_numpy(g[k]) for k in ("pad_ids", "pad_mask", "pad_labels"))
    loss_ref, logits_ref, grads_ref = O.forward_loss_grads(cfg, sd_bf, ids, lab, attention_mask=am)
    _level(m, 2)
    m.zero_grad()
    out = m(input_ids=ids, attention_mask=am, labels=lab)
    out.loss.backward()
    sync()
    assert abs(float(out.loss.detach()) - float(loss_ref)) <= 5e-3
    check("level 2 logits vs oracle (same bf16 weights)", out.logits.float().cpu()[am.bool()], logits_ref[am.bool()], 1e-2)
    for k, gv in m.named_grads():
        ref = grads_ref[k]
        c = cosine(gv, ref)
        small = k.endswith(".bias") or k.endswith("norm.weight")
        assert c >= (0.99 if small else 0.999), f"{k}: cosine {c:.5f} rel {rel_err(gv, ref):.3e}"
        assert abs(float(gv.norm()) / float(ref.norm()) - 1) <= 3e-2, k
    for key in [k for k in g if k.startswith("pad_gradfull/")]:
        name = key.split("/", 1)[1]
        c = cosine(dict(m.named_grads())[name], torch.from_numpy(g[key]))
        assert c >= 0.99, f"{name} vs reference golden: cosine {c:.5f}"
    E = m.flat_grads[: 512 * cfg.hidden].view(512, cfg.hidden)
    assert float(E[cfg.vocab:].abs().max()) == 0.0


@pytest.mark.parametrize("two", [1, 0])
def test_bucket_callback_at_level2(two):
    """bucket_layers = 1: the reported ranges tile the buffer exactly as at level 0, and each is complete on
    slam_bucket_stream when reported."""
    m = BODIES["qwen6_hd64"]()
    m.engine.set_option("bwd_wgrad_stream", two)
    batch = _packed(m.config.vocab_size, seed=2)

    def run(level):
        _level(m, level)
        snaps = []

        def cb(off, cnt, stream=None):
            (torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream()).synchronize()
            snaps.append((off, cnt, bool(stream), m.flat_grads[off:off + cnt].clone()))
        m.zero_grad()
        m(**batch, return_logits=False)
        m.backward(1.0, 1, cb)
        sync()
        return snaps, m.flat_grads.clone()

    s0, g0 = run(0)
    s2, g2 = run(2)
    assert torch.equal(g0, g2)
    assert [(o, c, s) for o, c, s, _ in s0] == [(o, c, s) for o, c, s, _ in s2]
    n = m.engine.n_params
    assert s2[0][0] + s2[0][1] == n and s2[-1][0] == 0 and len(s2) == Q6.n_layers
    for (o1, c1, _, _), (o2, c2, _, _) in zip(s2, s2[1:]):
        assert o2 + c2 == o1 and c1 > 0 and c2 > 0
    for off, cnt, _, snap in s2:
        assert torch.equal(snap, g2[off:off + cnt]), (off, cnt)


def _rows(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(n):
        k = int(torch.randint(20, 70, (1,), generator=g))
        ids = [1] + torch.randint(2, 502, (k,), generator=g).tolist() + [1]
        rows.append({"input_ids": ids, "attention_mask": [1] * len(ids)})
    return rows


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
@pytest.mark.parametrize("packing", [False, True])
def test_trainer_runs_are_identical(osd, packing):
    """4 optimizer steps of SLAMTrainer (GA 2, clip, AdamW, cosine schedule): gradient_checkpointing=True and recompute_level=1
    against the default run - logged losses, gradient norms and the final weights."""
    from slamkit_amd.data import DataCollatorForLanguageModeling, DataCollatorWithFlattening, TokenDataset
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    sd = O.init_weights(Q6, seed=5, bias_std=0.02, norm_jitter=0.05)
    ds = TokenDataset(_rows(16))
    coll = DataCollatorWithFlattening() if packing else DataCollatorForLanguageModeling(pad_token_id=0)

    def run(**kw):
        args = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=2, num_train_epochs=1,
                                     warmup_steps=2, warmup_ratio=0.0, learning_rate=2e-3, logging_steps=1, max_grad_norm=0.5,
                                     weight_decay=0.01, seed=7, output_dir="/tmp/unused", optim_state_dtype=osd, **kw)
        m = _qwen(Q6, sd)
        tr = SLAMTrainer(model=m, args=args, data_collator=coll, train_dataset=ds)
        assert m.is_gradient_checkpointing == bool(kw)
        st = tr.train()
        sync()
        logs = [(r["loss"], r["grad_norm"]) for r in st.log_history if "loss" in r]
        assert st.global_step == 4 and len(logs) == 4
        return logs, m.flat_params.clone(), m._weights.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()

    ref = run()
    assert len(set(ref[0])) == 4  # four different steps
    for kw in (dict(gradient_checkpointing=True), dict(recompute_level=1)):
        got = run(**kw)
        assert got[0] == ref[0], (kw, got[0], ref[0])
        for a, b, name in zip(ref[1:], got[1:], ("params", "weights", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a, b), (kw, name)


def test_dpo_trainer_step_is_identical():
    from slamkit_amd.tokeniser import UnitTokeniser
    from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer
    from tests.test_gpu_dpo import _pairs
    sd_pol = O.init_weights(Q6, seed=11, bias_std=0.02)
    sd_ref = O.init_weights(Q6, seed=12, bias_std=0.02)
    tok = UnitTokeniser(None, load_fe=False)

    def run(**kw):
        pol, ref = _qwen(Q6, sd_pol, 16 * 256), _qwen(Q6, sd_ref, 16 * 256)
        args = DPOConfig(per_device_train_batch_size=4, beta=0.1, logging_steps=1, max_steps=1, output_dir="/tmp/unused",
                         learning_rate=5e-5, warmup_steps=0, warmup_ratio=0.0, **kw)
        tr = SLAMDPOTrainer(model=pol, ref_model=ref, args=args, train_dataset=_pairs(4), processing_class=tok)
        assert pol.is_gradient_checkpointing == bool(kw)
        st = tr.train()
        sync()
        logs = [(r["loss"], r["grad_norm"]) for r in st.log_history if "loss" in r]
        assert len(logs) == 1
        return logs, pol.flat_params.clone(), pol._weights.clone()

    ref = run()
    for kw in (dict(gradient_checkpointing=True), dict(recompute_level=1)):
        got = run(**kw)
        assert got[0] == ref[0], (kw, got[0], ref[0])
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), kw


def _prefill(m, ids, lens, cap):
    B, T = ids.shape
    dev = m.device
    cache = torch.zeros(m.engine.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    m._ensure_workspace(max(B * T, 2 * B))
    logits = torch.empty(B, m.config.vocab_size, dtype=torch.float32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    ids_d = ids.to(dev).contiguous()
    m.engine.prefill(ids_d, lens_d, B, T, logits)
    first = logits.clone()
    nxt = first.argmax(-1).contiguous()
    m.engine.decode_step(nxt, lens_d, B, logits)
    sync()
    return first, logits.clone(), cache.clone()


@pytest.mark.parametrize("which", ["tiny_golden", "qwen6"])
def test_generation_at_level2(which, golden_data):
    """generate, the prefill logits, one decode step and the KV cache contents on the Qwen2 golden prompts: the golden tiny
    model (fewer layers than slots) and a 6-layer body, whose layers share their q|k|v buffers, so K / V leave inside the
    layer loop. A forward + backward afterwards still equals level 0."""
    gold = dict(np.load(os.path.join(GOLDEN, "generate.npz")))
    if which == "tiny_golden":
        meta = golden_data["meta"]
        cfg = O.OracleConfig(**meta["config"])
        m = _qwen(cfg, O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"]), 512)
    else:
        m = BODIES["qwen6_hd64"]()
    ids, am = torch.from_numpy(gold["tiny_ids"]), torch.from_numpy(gold["tiny_mask"])
    kw = dict(input_ids=ids, attention_mask=am, bad_words_ids=gold["bad_words"].tolist(),
              max_new_tokens=int(gold["max_new_tokens"]), eos_token_id=int(gold["tiny_eos"]), pad_token_id=0)
    # right-aligned golden prompts -> left-aligned rows for the raw prefill
    lens = am.sum(1).tolist()
    rows = torch.zeros_like(ids)
    for b, n in enumerate(lens):
        rows[b, :n] = ids[b, ids.shape[1] - n:] if int(am[b, 0]) == 0 else ids[b, :n]
    cap = -(-(ids.shape[1] + 8) // 64) * 64
    batch = _dense(m.config.vocab_size, seed=8)
    res = {}
    for level in (0, 2):
        _level(m, level)
        out = m.generate(**kw).cpu()
        res[level] = (out,) + _prefill(m, rows, lens, cap) + _step(m, batch)
    for a, b, name in zip(res[0], res[2], ("generate", "prefill logits", "decode logits", "kv cache", "loss", "logits", "grads")):
        assert torch.equal(a, b), (which, name)
    assert bool(res[2][3].any())


@pytest.mark.parametrize("body", ["qwen6_hd64", "qwen4_hd128", "opt5"])
def test_time_families_at_level2(body):
    """time_families at levels 1 and 2: the step succeeds with the same bits, and the record list holds the level-0 records
    plus the re-run launches, under the forward families' names. Level 2 re-runs, per layer: two norms, the QKV projection
    (one record, with or without a separate RoPE launch), attention, the output projection and gate|up (fc1) - not the down
    projection (fc2). Level 1 rebuilds, per layer: two norms and (Qwen2) the activation."""
    m = BODIES[body]()
    L = m.config.base_config["num_hidden_layers"]
    opt = body == "opt5"
    batch = _packed(m.config.vocab_size, seed=3)
    m.engine.set_option("time_families", 1)
    names, outs = {}, {}
    for level in (0, 1, 2):
        _level(m, level)
        outs[level] = _step(m, batch)
        names[level] = [n for n, _ in m.engine.family_ms()]
        assert all(ms >= 0.0 for _, ms in m.engine.family_ms())
    m.engine.set_option("time_families", 0)
    _same(outs[0], outs[1], "time_families level 1")
    _same(outs[0], outs[2], "time_families level 2")
    cnt = lambda lv, n: names[lv].count(n)  # noqa: E731
    assert len(names[2]) == len(names[0]) + 6 * L
    assert len(names[1]) == len(names[0]) + (2 if opt else 3) * L
    for fam, extra in (("norm_fwd", 2), ("qkv_fwd", 1), ("attn_fwd", 1), ("o_fwd", 1), ("gateup_fwd", 1), ("down_fwd", 0)):
        assert cnt(2, fam) == cnt(0, fam) + extra * L, fam
    assert cnt(1, "norm_fwd") == cnt(0, "norm_fwd") + 2 * L and cnt(1, "gateup_fwd") == cnt(0, "gateup_fwd") + (0 if opt else L)
    # the re-runs sit inside the backward part of the list: after the loss, the first one before any layer's backward
    loss_at = names[2].index("loss")
    assert names[2][:loss_at + 1] == names[0][:loss_at + 1]
    assert names[2].index("attn_fwd", loss_at) < names[2].index("down_dgrad_dswiglu")


def test_level_switch_rebinds_and_shrinks_the_workspace():
    m = BODIES["qwen6_hd64"]()
    batch = _dense(m.config.vocab_size)
    ref = _step(m, batch)
    tokens = m._ws_tokens
    sizes = {}
    for level in (2, 1, 0):
        _level(m, level)
        assert m._ws is None and m._ws_tokens == 0
        _same(ref, _step(m, batch), f"after switching to level {level}")
        assert m._ws_tokens == tokens  # bound again at the size it had
        sizes[level] = m._ws.numel()
    assert sizes[2] < sizes[1] < sizes[0]
    with pytest.raises(ValueError):
        m.gradient_checkpointing_enable(level=3)
    assert "gradient_checkpointing" not in str(m.config.to_dict()) and "recompute" not in str(m.config.to_dict())
