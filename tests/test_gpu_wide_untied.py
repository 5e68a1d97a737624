"""-m gpu: wide (2048 < hidden <= 4096), untied-head Qwen2 bodies - the Qwen2.5-7B shape.

1. the two-waves-per-row RMSNorm kernels through the single-op entries (bars of test_gpu_ops.test_rmsnorm_fwd_bwd);
2. the untied head on the tiny config: logits, loss, every gradient against the oracle (`decoder_stack(..., E_head=lm_head)`),
   the embedding gradient's single writer (zero rows, store-then-accumulate, bucket ranges);
3. two layers at the 7B widths and at the hidden-4096 limit against the oracle;
4. a checkpoint written by the reference's own UnitLM.save_pretrained (tests/golden/make_golden_untied.py), round trips, TWIST;
5. KV-cached generation against HF's greedy generations of the same checkpoint, every step teacher-forced;
6. the data-parallel step on a forced one-rank RCCL group;
7. the flat-buffer kernels beyond 2^32 elements on the full Qwen2.5-7B layout.
Tolerances are those of the tests named in each docstring."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests.gpu_util import check, cosine, dev_bf16, lib, ptr, rel_err, rnd, stream, sync
from tests.test_gpu_model import _check_all_grads, _packed_row

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD = "lm.lm_head.weight"
EMBED = "lm.model.embed_tokens.weight"
LOGITS_TOL = 2e-2

CFG_7B = dict(n_layers=2, hidden=3584, n_heads=28, n_kv_heads=4, head_dim=128, intermediate=18944, rope_theta=1000000.0)
CFG_4096 = dict(n_layers=2, hidden=4096, n_heads=32, n_kv_heads=8, head_dim=128, intermediate=11008, rope_theta=1000000.0)


def _mk(cfg: O.OracleConfig, sd, max_tokens=4096, untied=True, **kw):
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base = dict(num_hidden_layers=cfg.n_layers, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads,
                num_key_value_heads=cfg.n_kv_heads, head_dim=cfg.head_dim, intermediate_size=cfg.intermediate,
                rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, tie_word_embeddings=not untied)
    m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=max_tokens), **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m


def _normal_sd(cfg, seed):
    """Seeded normals rounded to bf16 (the hash-based golden initialiser is slow at these sizes), plus a separate head."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in O.hf_keys(cfg) + [(HEAD, (cfg.vocab, cfg.hidden))]:
        w = (1.0 + 0.1 * torch.randn(shp, generator=g)) if k.endswith("norm.weight") else 0.02 * torch.randn(shp, generator=g)
        sd[k] = w.to(torch.bfloat16).float()
    sd[EMBED][cfg.pad_token_id].zero_()
    return sd


def _oracle(cfg, sd, ids, labels, attention_mask=None, position_ids=None, packed=False, grads=True):
    """The oracle with a separate head: decoder_stack(cfg, sd, F.embedding(ids, E), E_head=sd[lm_head]) under autograd."""
    params = {k: v.clone().requires_grad_(grads) for k, v in sd.items()}
    h0 = F.embedding(ids, params[EMBED], padding_idx=cfg.pad_token_id)
    logits = O.decoder_stack(cfg, params, h0, params[HEAD], attention_mask, position_ids, packed)
    loss = O.compute_loss(logits, labels)
    if not grads:
        return loss.detach(), logits.detach(), None
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad.detach() for k, v in params.items()}


def _oracle_logits(cfg, sd, ids, bf16_acts=False, **kw):
    with torch.no_grad():
        return O.decoder_stack(cfg, sd, F.embedding(ids, sd[EMBED]), sd[HEAD], bf16_acts=bf16_acts, **kw)


# ---- 1. norm kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [5, 300, 4099, 8192])
@pytest.mark.parametrize("H", [2056, 2560, 3584, 4096])
def test_rmsnorm_wide_fwd_bwd(M, H):
    """slam_op_rmsnorm_fwd / _bwd on rows wider than one wave holds, with and without the residual-gradient input, against
    O.rms_norm under autograd (y and dx 3e-3 / 1e-2, rstd 1e-6, dw 1e-5); two runs bit-identical."""
    x, w, dy, dres = rnd(M, H, seed=1), 1 + 0.1 * rnd(H, seed=2), rnd(M, H, seed=3), rnd(M, H, seed=4)
    w = w.to(torch.bfloat16).float()
    xd, wd = dev_bf16(x), dev_bf16(w)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    yr = O.rms_norm(xr, wr, 1e-6)
    yr.backward(dy)
    dyd, dresd = dev_bf16(dy), dev_bf16(dres)
    ws = torch.empty(lib().slam_op_rmsnorm_bwd_workspace(M, H) // 4 + 16, dtype=torch.float32, device="cuda")
    runs = []
    for rep in range(2):
        y = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
        rstd = torch.empty(M, dtype=torch.float32, device="cuda")
        assert lib().slam_op_rmsnorm_fwd(ptr(xd), ptr(wd), ptr(y), ptr(rstd), M, H, 1e-6, stream()) == 0
        sync()
        if rep == 0:
            check("rmsnorm_fwd wide", y.float(), yr.detach(), 3e-3, 1e-2)
            check("rmsnorm wide rstd", rstd, torch.rsqrt(x.pow(2).mean(-1) + 1e-6), 1e-6)
        keep = [y.view(torch.int16).clone(), rstd.clone()]
        for use_res in (False, True):
            dx = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
            dw = torch.full((H,), 7.0, dtype=torch.float32, device="cuda")
            assert lib().slam_op_rmsnorm_bwd(ptr(dyd), ptr(xd), ptr(wd), ptr(rstd), ptr(dresd) if use_res else None,
                                             ptr(dx), ptr(dw), ptr(ws), M, H, stream()) == 0
            sync()
            if rep == 0:
                check(f"rmsnorm_bwd wide dx res={use_res}", dx.float(), xr.grad + (dres if use_res else 0), 3e-3, 1e-2)
                check("rmsnorm_bwd wide dw", dw, wr.grad, 1e-5)
            keep += [dx.view(torch.int16).clone(), dw.clone()]
        runs.append(keep)
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "not bit-identical run to run"


def test_rmsnorm_beyond_4096_is_refused_before_any_launch():
    M, H = 8, 4104
    x = torch.zeros(M, H, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(H, dtype=torch.bfloat16, device="cuda")
    y = torch.full((M, H), 3.0, dtype=torch.bfloat16, device="cuda")
    rstd = torch.zeros(M, dtype=torch.float32, device="cuda")
    dw = torch.zeros(H, dtype=torch.float32, device="cuda")
    ws = torch.zeros(lib().slam_op_rmsnorm_bwd_workspace(M, H) // 4 + 16, dtype=torch.float32, device="cuda")
    assert lib().slam_op_rmsnorm_fwd(ptr(x), ptr(w), ptr(y), ptr(rstd), M, H, 1e-6, stream()) != 0
    assert lib().slam_op_rmsnorm_bwd(ptr(x), ptr(x), ptr(w), ptr(rstd), None, ptr(y), ptr(dw), ptr(ws), M, H, stream()) != 0
    sync()
    assert bool((y == 3.0).all())


# ---- 2. untied head, tiny dims ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_untied(golden_data):
    meta = golden_data["meta"]
    cfg = O.OracleConfig(**meta["config"])
    sd = O.init_weights(cfg, seed=meta["seed"], bias_std=meta["bias_std"], norm_jitter=meta["norm_jitter"])
    sd[HEAD] = O._hash_uniform_t(cfg.vocab * cfg.hidden, 777, 0.02 * math.sqrt(3.0), 0.0, torch.float32).reshape(cfg.vocab, cfg.hidden)
    sd_bf = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    return cfg, sd, sd_bf, _mk(cfg, sd)


def test_untied_state_dict_and_output_embeddings(tiny_untied):
    cfg, sd, sd_bf, m = tiny_untied
    out = m.state_dict(torch.float32)
    assert set(out) == set(sd) and HEAD in dict(m.named_parameters()) and HEAD in dict(m.named_grads())
    for k in sd:
        assert torch.equal(out[k], sd[k]), k
    assert m.config.tie_word_embeddings is False and m.config.to_dict()["tie_word_embeddings"] is False
    assert torch.equal(m.get_output_embeddings().float().cpu(), sd_bf[HEAD])
    assert torch.equal(m.get_input_embeddings().float().cpu(), sd_bf[EMBED])
    t = m.engine.tensors
    assert list(t)[-1] == "lm_head" and t["lm_head"].offset + t["lm_head"].numel == m.engine.n_params
    pads = m.flat_params[t["lm_head"].offset:].view(512, cfg.hidden)[cfg.vocab:]
    assert float(pads.float().abs().max()) == 0.0
    assert m.num_parameters() == sum(v.numel() for v in sd.values())


def test_untied_init_weights_has_no_zeroed_head_row(tiny_untied):
    cfg = tiny_untied[0]
    m = _mk(cfg, None, seed=5)
    head, emb = m.get_output_embeddings().float(), m.get_input_embeddings().float()
    assert float(emb[cfg.pad_token_id].abs().max()) == 0.0 and float(head[cfg.pad_token_id].abs().max()) > 0.0
    assert abs(float(head.std()) - 0.02) < 2e-3 and not torch.equal(head, emb)


def _check_embed_zero_rows(m, cfg, ids):
    eg = dict(m.named_grads())[EMBED]
    seen = torch.zeros(cfg.vocab, dtype=torch.bool)
    seen[ids.flatten()] = True
    seen[cfg.pad_token_id] = False  # padding_idx: no gather-side gradient, and no head contribution any more
    assert float(eg[~seen.to(eg.device)].abs().max()) == 0.0, "rows of absent ids / the pad id must be exactly zero"
    assert float(eg[seen.to(eg.device)].abs().max()) > 0.0
    t = m.engine.tensors["embed"]
    img = m.flat_grads[t.offset:t.offset + t.numel].view(t.rows, t.cols)
    if t.rows > cfg.vocab:  # the pad rows of the image
        assert float(img[cfg.vocab:].abs().max()) == 0.0


def test_untied_padded_batch_vs_oracle(tiny_untied, golden_npz):
    cfg, sd, sd_bf, m = tiny_untied
    ids, am, lab = (torch.from_numpy(golden_npz[k]) for k in ("pad_ids", "pad_mask", "pad_labels"))
    loss_ref, logits_ref, grads_ref = _oracle(cfg, sd_bf, ids, lab, attention_mask=am)
    m.zero_grad()
    out = m(input_ids=ids, attention_mask=am, labels=lab)
    out.loss.backward()
    torch.cuda.synchronize()
    print("untied tiny padded loss engine/oracle", float(out.loss), float(loss_ref))
    assert abs(float(out.loss) - float(loss_ref)) <= 2e-2
    check("untied logits vs oracle", out.logits.float().cpu()[am.bool()], logits_ref[am.bool()], 2e-2)
    _check_all_grads(m, grads_ref, "untied tiny padded")
    assert float(dict(m.named_grads())[HEAD][cfg.pad_token_id].abs().max()) > 0.0  # row `pad` of lm_head gets a gradient
    assert (ids == cfg.pad_token_id).any()
    _check_embed_zero_rows(m, cfg, ids)
    # the tied model on the same weights computes something else: the head really is read from lm_head
    tied_logits = O.model_forward(cfg, sd_bf, ids)
    assert rel_err(out.logits.float().cpu()[am.bool()], tied_logits[am.bool()]) > 0.5


def test_untied_packed_row_vs_oracle(tiny_untied, golden_npz):
    cfg, sd, sd_bf, m = tiny_untied
    ids, pos, lab = (torch.from_numpy(golden_npz[k]) for k in ("pack_ids", "pack_pos", "pack_labels"))
    loss_ref, logits_ref, grads_ref = _oracle(cfg, sd_bf, ids, lab, position_ids=pos, packed=True)
    m.zero_grad()
    out = m(input_ids=ids, position_ids=pos, labels=lab)
    m.backward()
    torch.cuda.synchronize()
    assert abs(float(out.loss) - float(loss_ref)) <= 2e-2
    check("untied packed logits vs oracle", out.logits.float().cpu(), logits_ref, 2e-2)
    _check_all_grads(m, grads_ref, "untied tiny packed")
    _check_embed_zero_rows(m, cfg, ids)


def test_untied_backward_accumulates_scales_and_stores(tiny_untied, golden_npz):
    """backward(1.0) then backward(2.0) = three times the single gradient (1e-2), a repeat is bit-identical
    (test_backward_accumulates_and_scales); and a STORING backward ("grad_overwrite_next", the first micro-batch of a
    trainer step) over a dirty buffer gives the same bits: the embedding gradient's only writer stores."""
    cfg, sd, sd_bf, m = tiny_untied
    ids, lab = (torch.from_numpy(golden_npz[k]) for k in ("pad_ids", "pad_labels"))
    m.zero_grad()
    m(input_ids=ids, labels=lab, return_logits=False)
    m.backward(1.0)
    g1 = m.flat_grads.clone()
    m(input_ids=ids, labels=lab, return_logits=False)
    m.backward(2.0)
    g3 = m.flat_grads.clone()
    torch.cuda.synchronize()
    assert rel_err(g3, 3 * g1) <= 1e-2
    m.zero_grad()
    m(input_ids=ids, labels=lab, return_logits=False)
    m.backward(1.0)
    assert torch.equal(m.flat_grads, g1)
    m.flat_grads.fill_(123.0)  # what a previous step left behind
    m.engine.set_option("grad_overwrite_next", 1)
    m(input_ids=ids, labels=lab, return_logits=False)
    m.backward(1.0)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_grads, g1)
    m(input_ids=ids, labels=lab, return_logits=False)
    m.backward(2.0)  # and the next micro-batch accumulates onto the stored values
    assert torch.equal(m.flat_grads, g3)


def test_untied_bucket_ranges_tile_the_flat_gradient(tiny_untied, golden_npz):
    cfg, sd, sd_bf, m = tiny_untied
    ids, lab = (torch.from_numpy(golden_npz[k]) for k in ("pad_ids", "pad_labels"))
    got = []
    m.zero_grad()
    m(input_ids=ids, labels=lab, return_logits=False)
    m.backward(1.0, 1, lambda off, cnt, stream=None: got.append((off, cnt)))
    torch.cuda.synchronize()
    n = m.engine.n_params
    t = m.engine.tensors
    assert got[0][0] + got[0][1] == n and got[-1][0] == 0
    assert got[0][0] <= t["lm_head"].offset and t["lm_head"].offset + t["lm_head"].numel == n  # lm_head is in the first range
    for (o1, c1), (o2, c2) in zip(got, got[1:]):
        assert o2 + c2 == o1 and c1 > 0 and c2 > 0
    assert got[-1][1] == t["layers.1.ln1"].offset


def test_untied_large_vocab_scatter_path_stores_and_is_deterministic():
    """V > 512: the embedding gradient is a token-ordered scatter; with the head in its own tensor a storing backward has to
    zero the embedding first. Against the oracle, then store == zero + accumulate bit for bit."""
    cfg = O.OracleConfig(n_layers=1, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, intermediate=512, vocab=5003)
    sd = _normal_sd(cfg, 3)
    m = _mk(cfg, sd, max_tokens=1024)
    gen = torch.Generator().manual_seed(2)
    ids, pos, lab = _packed_row([200, 56, 64], cfg.vocab, 4000, gen)
    loss_ref, logits_ref, grads_ref = _oracle(cfg, sd, ids, lab, position_ids=pos, packed=True)
    m.zero_grad()
    out = m(input_ids=ids, position_ids=pos, labels=lab)
    m.backward()
    torch.cuda.synchronize()
    assert abs(float(out.loss) - float(loss_ref)) <= 2e-2
    check("untied V=5003 logits", out.logits.float().cpu(), logits_ref, 2e-2)
    _check_all_grads(m, grads_ref, "untied V=5003 scatter path")
    _check_embed_zero_rows(m, cfg, ids)
    g1 = m.flat_grads.clone()
    m.flat_grads.fill_(-5.0)
    m.engine.set_option("grad_overwrite_next", 1)
    m(input_ids=ids, position_ids=pos, labels=lab, return_logits=False)
    m.backward()
    torch.cuda.synchronize()
    assert torch.equal(m.flat_grads, g1)


# ---- 3. 7B widths, two layers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,vocab,lens", [(CFG_7B, 502, [160, 96, 64]), (CFG_7B, 152064, [300, 236, 64]),
                                             (CFG_4096, 502, [160, 96, 64])], ids=["7b-V502", "7b-V152064", "h4096-V502"])
def test_wide_layers_vs_oracle(dims, vocab, lens):
    """Two layers at the Qwen2.5-7B widths (one-hot and scatter embedding-gradient paths) and at the hidden-4096 limit, one packed
    row, against the fp32 oracle. Logit tolerance by the rule of test_configs3_full_depth_packed_vs_oracle: max(2e-2, 1.1 x
    emu), emu = the oracle's own bf16-activation path against its fp32 run on this batch. Gradients: _check_all_grads
    defaults (0.999 matrices / 0.99 vectors)."""
    cfg = O.OracleConfig(vocab=vocab, **dims)
    sd = _normal_sd(cfg, 11)
    m = _mk(cfg, sd, max_tokens=1024)
    gen = torch.Generator().manual_seed(99)
    unit_lo = vocab - 500 if vocab > 1000 else 250
    ids, pos, lab = _packed_row(lens, vocab, unit_lo, gen)
    loss_ref, logits_ref, grads_ref = _oracle(cfg, sd, ids, lab, position_ids=pos, packed=True)
    emu = _oracle_logits(cfg, sd, ids, bf16_acts=True, position_ids=pos, packed=True)
    emu_dev = rel_err(emu, logits_ref)
    del emu
    m.zero_grad()
    out = m(input_ids=ids, position_ids=pos, labels=lab)
    m.backward()
    torch.cuda.synchronize()
    print(f"wide H={cfg.hidden} V={vocab} loss engine/oracle", float(out.loss), float(loss_ref))
    assert abs(float(out.loss) - float(loss_ref)) <= 2e-2
    tol = max(2e-2, 1.1 * emu_dev)
    print(f"[parity] H={cfg.hidden} V={vocab}: bf16-path emulation vs fp32 logits rel-rms {emu_dev:.3e} -> engine tolerance {tol:.3e}")
    check(f"wide H={cfg.hidden} V={vocab} logits", out.logits.float().cpu(), logits_ref, tol)
    assert len(list(m.named_grads())) == 12 * cfg.n_layers + 3
    _check_all_grads(m, grads_ref, f"wide H={cfg.hidden} V={vocab}, {sum(lens)} packed tokens")
    _check_embed_zero_rows(m, cfg, ids)
    g1 = m.flat_grads.clone()
    m.zero_grad()
    m(input_ids=ids, position_ids=pos, labels=lab, return_logits=False)
    m.backward()
    torch.cuda.synchronize()
    assert torch.equal(m.flat_grads, g1)


# ---- 4. reference-written checkpoint ------------------------------------------------------------------------------------
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "untied_model.npz")))


def test_untied_reference_checkpoint_matches_golden(tmp_path):
    """tests/golden/ref_untied_ckpt (the reference's UnitLM.save_pretrained of a tiny untied Qwen2) loads and reproduces the
    reference's fp32 outputs with the bars of test_opt_reference_checkpoint_matches_golden; save_pretrained writes
    lm.lm_head.weight and the reloaded model gives a bit-equal loss."""
    from safetensors.torch import load_file
    from slamkit_amd.model import UnitLM
    g = _golden()
    m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_untied_ckpt"), max_tokens=512)
    assert m.config.tie_word_embeddings is False and "lm_head" in m.engine.tensors
    ref_sd = load_file(os.path.join(GOLDEN, "ref_untied_ckpt", "model.safetensors"))
    assert torch.equal(m.get_output_embeddings().cpu(), ref_sd[HEAD]) and torch.equal(m.get_input_embeddings().cpu(), ref_sd[EMBED])
    ids, mask, labels = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels"))
    m.zero_grad()
    out = m(ids, attention_mask=mask, labels=labels)
    m.backward()
    torch.cuda.synchronize()
    got = out.logits.float().cpu()
    for b in range(ids.shape[0]):
        n = int(mask[b].sum())
        check(f"untied reference checkpoint logits row {b}", got[b, :n], torch.from_numpy(g["logits"][b, :n]), 2e-2)
    assert abs(float(out.loss) - float(g["loss"])) <= 2e-2, (float(out.loss), float(g["loss"]))
    grads = dict(m.named_grads())
    assert set(grads) == {str(k) for k in g["grad_names"]}
    for k, want in zip(g["grad_names"], g["grad_norms"]):
        k = str(k)
        if k.endswith("k_proj.bias"):  # zero in exact arithmetic (softmax is invariant to a constant key shift)
            continue
        got_n = float(grads[k].norm())
        assert abs(got_n - want) <= 3e-2 * want + 1e-7, (k, got_n, want)
    out2 = m(ids, attention_mask=mask, labels=labels, num_items_in_batch=100)
    assert abs(float(out2.loss) - float(g["loss_num_items"])) <= 2e-2
    for key, ignore in (("ll", None), ("ll_ignore", [3, 4, 5, 200])):
        ll = m.log_likelihood(ids, mean_nll=False, ignore_tokens=ignore).cpu()
        want = torch.from_numpy(g[key])
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(ll), fin), (key, ll, want)
        assert float((ll[fin] - want[fin]).abs().max()) <= 2e-2 * max(1.0, float(want[fin].abs().max()) / 100), (key, ll, want)
    # round trip through this engine's own save_pretrained
    loss0 = float(m(ids, attention_mask=mask, labels=labels).loss)
    d = str(tmp_path / "resaved")
    m.save_pretrained(d)
    saved = load_file(os.path.join(d, "model.safetensors"))
    assert HEAD in saved and torch.equal(saved[HEAD], ref_sd[HEAD]) and set(saved) == set(ref_sd)
    assert json.load(open(os.path.join(d, "config.json")))["tie_word_embeddings"] is False
    m2 = UnitLM.from_pretrained(d, max_tokens=512)
    assert m2.config.tie_word_embeddings is False
    assert float(m2(ids, attention_mask=mask, labels=labels).loss) == loss0


def test_untied_load_state_dict_requires_and_resizes_lm_head(tiny_untied):
    cfg, sd, sd_bf, m = tiny_untied
    m2 = _mk(cfg, None)
    with pytest.raises(KeyError):
        m2.load_state_dict({k: v for k, v in sd.items() if k != HEAD})
    tied = _mk(cfg, None, untied=False)
    tied.load_state_dict(sd)  # a tied model keeps ignoring lm_head.weight
    assert HEAD not in tied.key_map
    # longer tables are cut, shorter ones mean-filled: both tables alike (HF resize_token_embeddings resizes both)
    big = dict(sd)
    big[EMBED] = torch.cat([sd[EMBED], torch.ones(10, cfg.hidden)])
    big[HEAD] = torch.cat([sd[HEAD], torch.ones(10, cfg.hidden)])
    m2.load_state_dict(big)
    assert torch.equal(m2.state_dict(torch.float32)[HEAD], sd[HEAD]) and torch.equal(m2.state_dict(torch.float32)[EMBED], sd[EMBED])
    small = dict(sd)
    small[EMBED], small[HEAD] = sd[EMBED][:400], sd[HEAD][:400]
    m2.load_state_dict(small)
    got = m2.state_dict(torch.float32)
    for k in (EMBED, HEAD):
        assert torch.equal(got[k][:400], sd[k][:400])
        assert torch.allclose(got[k][400:], sd[k][:400].mean(0, keepdim=True).expand(cfg.vocab - 400, -1), atol=1e-6)


def test_twist_from_untied_text_lm_directory(tmp_path):
    """TWIST initialisation from a HuggingFace untied Qwen2 text LM with a larger vocabulary: embed_tokens AND lm_head equal
    the first vocab_size rows of the source; a tied / untied mismatch raises."""
    import transformers
    from safetensors.torch import load_file
    from slamkit_amd.model import UnitLM, UnitLMConfig
    torch.manual_seed(3)
    hf = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(
        vocab_size=640, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
        rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=False, max_position_embeddings=4096, pad_token_id=0,
        bos_token_id=1, eos_token_id=1))
    text = str(tmp_path / "untied_text_lm")
    hf.to(torch.bfloat16).save_pretrained(text, safe_serialization=True)
    src = load_file(os.path.join(text, "model.safetensors"))
    assert "lm_head.weight" in src and not torch.equal(src["lm_head.weight"], src["model.embed_tokens.weight"])
    tw = UnitLM(UnitLMConfig(base_model_name=text, vocab_size=502, twist_init=True, max_tokens=512))
    assert tw.config.tie_word_embeddings is False
    assert torch.equal(tw.get_input_embeddings().cpu(), src["model.embed_tokens.weight"][:502])
    assert torch.equal(tw.get_output_embeddings().cpu(), src["lm_head.weight"][:502])
    k = "model.layers.1.mlp.down_proj.weight"
    assert torch.equal(dict(tw.named_parameters())["lm." + k].cpu(), src[k])
    base = json.load(open(os.path.join(text, "config.json")))
    tied = UnitLM(UnitLMConfig(base_model_name="local", base_config={**base, "tie_word_embeddings": True}, vocab_size=502, max_tokens=512))
    with pytest.raises(ValueError, match="tie_word_embeddings"):
        tied.load_hf_text_lm(text)
    with pytest.raises(ValueError, match="tie_word_embeddings"):
        tw.load_hf_text_lm(os.path.join(GOLDEN, "hf_text_lm"))  # the tied tiny text LM


# ---- 5. generation ------------------------------------------------------------------------------------------------------
def _compact(ids, am):
    """Left-padded prompts -> right-padded rows + lengths (what UnitLM.generate does before the prefill)."""
    lens = am.sum(1).to(torch.int32)
    T = int(lens.max())
    out = torch.zeros(ids.shape[0], T, dtype=torch.long)
    for b in range(ids.shape[0]):
        out[b, :int(lens[b])] = ids[b][am[b].bool()]
    return out, lens


def test_untied_teacher_forced_decode_matches_hf_scores_every_step():
    """prefill, then decode_step fed HF's own golden tokens: the logits of EVERY step against the processed scores HF's
    generate kept (bad-word columns, which HF sets to -inf, left out): rel-RMS per row and step <= 2e-2."""
    from slamkit_amd.model import UnitLM
    g = _golden()
    m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_untied_ckpt"), max_tokens=512, allocate_grads=False)
    ids, am = torch.from_numpy(g["gen_ids"]), torch.from_numpy(g["gen_mask"])
    seq, scores = torch.from_numpy(g["gen_seq"]), torch.from_numpy(g["gen_scores"])
    NEW, Tp, V = int(g["max_new_tokens"]), ids.shape[1], scores.shape[2]
    keep = torch.ones(V, dtype=torch.bool)
    keep[torch.from_numpy(g["bad_words"]).flatten()] = False
    assert scores.shape == (ids.shape[0], NEW, V) and bool(torch.isfinite(scores[:, :, keep]).all())
    rows, lens = _compact(ids, am)
    B, T = rows.shape
    dev = m.device
    lens_d = lens.to(dev)
    cap = -(-(T + NEW) // 64) * 64
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    steps = []
    m.engine.prefill(rows.to(dev).contiguous(), lens_d, B, T, logits)
    steps.append(logits.clone())
    given = seq[:, Tp:].to(dev)
    for k in range(NEW - 1):
        m.engine.decode_step(given[:, k].contiguous(), lens_d, B, logits)
        steps.append(logits.clone())
    sync()
    dec = torch.stack(steps, 1).cpu()
    worst = 0.0
    for b in range(B):
        for k in range(NEW):
            e = rel_err(dec[b, k][keep], scores[b, k][keep])
            worst = max(worst, e)
            assert e <= LOGITS_TOL, (b, k, e)
    print(f"[parity] untied teacher-forced decode vs HF scores: worst per-step rel-rms {worst:.3e} over {B} x {NEW} steps")


def test_untied_generate_matches_hf_golden():
    """generate itself: the prompt returned as passed; each row equals HF's exactly up to its first step whose golden top-1 /
    top-2 margin is below 2 x 2e-2 x score_rms; EOS is followed by pad only. (No matched-share bar: on this model the margins
    alone do not back one; the teacher-forced test above covers the later steps.)"""
    from slamkit_amd.model import UnitLM
    g = _golden()
    m = UnitLM.from_pretrained(os.path.join(GOLDEN, "ref_untied_ckpt"), max_tokens=512, allocate_grads=False)
    ids, am = torch.from_numpy(g["gen_ids"]), torch.from_numpy(g["gen_mask"])
    want, margin, eos = torch.from_numpy(g["gen_seq"]), torch.from_numpy(g["gen_margin"]), int(g["gen_eos"])
    out = m.generate(input_ids=ids, attention_mask=am, bad_words_ids=g["bad_words"].tolist(), max_new_tokens=int(g["max_new_tokens"]),
                     eos_token_id=eos, pad_token_id=0).cpu()
    assert out.dtype == torch.int64 and out.shape == want.shape, (out.shape, want.shape)
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids)
    tol = 2 * LOGITS_TOL * float(g["gen_score_rms"])
    new, wnew = out[:, T:], want[:, T:]
    for b in range(want.shape[0]):
        low = (margin[b] < tol).nonzero()
        trust = int(low[0]) if len(low) else wnew.shape[1]
        diff = (new[b] != wnew[b]).nonzero()
        first = int(diff[0]) if len(diff) else wnew.shape[1]
        print(f"[parity] untied generate row {b}: first near-tie at step {trust}, first difference at step {first}")
        assert first >= trust, (b, "diverged at", first, "before the first near-tie", trust)
        hit = (new[b] == eos).nonzero()
        if len(hit):
            assert (new[b, int(hit[0]) + 1:] == 0).all()
    assert not torch.isin(new, torch.from_numpy(g["bad_words"]).flatten()).any()


def test_teacher_forced_decode_at_7b_widths_matches_forward_and_oracle():
    """test_teacher_forced_decode_matches_forward_and_oracle at the 7B widths (two layers, V = 502, untied): the skinny GEMMs
    at K = 3584 and K = 18944, decode attention at 7 query heads per KV head of 128."""
    cfg = O.OracleConfig(vocab=502, **CFG_7B)
    m = _mk(cfg, None, max_tokens=1024, allocate_grads=False, seed=7)
    sd_bf = {k: v.float() for k, v in m.state_dict(torch.bfloat16).items()}
    g = torch.Generator().manual_seed(3)
    lens = [37, 20, 5]
    NEW = 40
    B, T = len(lens), max(lens)
    rows = [[1] + torch.randint(2, cfg.vocab, (n - 1,), generator=g).tolist() for n in lens]
    given = torch.randint(2, cfg.vocab, (B, NEW), generator=g)
    ids = torch.zeros(B, T, dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.tensor(r)
    dev = m.device
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    cap = -(-(T + NEW) // 64) * 64
    cache = torch.empty(m.engine.kv_cache_bytes(B, cap), dtype=torch.uint8, device=dev)
    m.engine.bind_kv_cache(cache, B, cap)
    logits = torch.empty(B, cfg.vocab, dtype=torch.float32, device=dev)
    steps = []
    m.engine.prefill(ids.to(dev).contiguous(), lens_d, B, T, logits)
    steps.append(logits.clone())
    given_d = given.to(dev)
    for k in range(NEW - 1):
        m.engine.decode_step(given_d[:, k].contiguous(), lens_d, B, logits)
        steps.append(logits.clone())
    sync()
    assert lens_d.tolist() == [n + NEW - 1 for n in lens]
    dec = torch.stack(steps, 1).cpu()
    full = torch.zeros(B, T + NEW, dtype=torch.long)
    for b, r in enumerate(rows):
        full[b, :len(r)] = torch.tensor(r)
        full[b, len(r):len(r) + NEW] = given[b]
    fwd = m(input_ids=full).logits.float().cpu()
    ref = _oracle_logits(cfg, sd_bf, full)
    for b, n in enumerate(lens):
        e = rel_err(dec[b], fwd[b, n - 1:n - 1 + NEW])
        e2 = rel_err(dec[b], ref[b, n - 1:n - 1 + NEW])
        print(f"[parity] 7B-width decode row {b}: vs forward {e:.3e}, vs oracle {e2:.3e}")
        assert e <= LOGITS_TOL, (b, "decode vs forward", e)
        assert e2 <= LOGITS_TOL, (b, "decode vs oracle", e2)


# ---- 6. data parallel ---------------------------------------------------------------------------------------------------
DP_WORKER = r'''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["SLAM_ROOT"])
from oracle import slam_oracle as O
from slamkit_amd.model import UnitLM, UnitLMConfig
from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments

force = os.environ.get("SLAM_DP_FORCE") == "1"
torch.cuda.set_device(0)
if force:
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
cfg = O.TINY
base = dict(num_hidden_layers=4, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads,
            head_dim=cfg.head_dim, intermediate_size=cfg.intermediate, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
            tie_word_embeddings=False)
m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=512), seed=1)
assert "lm_head" in m.engine.tensors
args = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=2, learning_rate=1e-3,
                             max_grad_norm=0.5, logging_steps=0, ddp_bucket_layers=1, weight_decay=0.01,
                             ddp_comm_dtype=os.environ.get("COMM") or None, ddp_algo=os.environ.get("ALGO") or "all_reduce",
                             optim_state_dtype=os.environ.get("OSD") or "float32",
                             grad_norm_from_backward=os.environ.get("NORM_PARTIALS", "1") == "1")
tr = SLAMTrainer(model=m, args=args)
assert tr.reducer.force == force
head0 = m.get_output_embeddings().clone()
ranges = []
orig = tr.reducer.finish
def finish():
    r = orig()
    ranges.append(r)
    return r
tr.reducer.finish = finish
g = torch.Generator().manual_seed(0)
for step in range(3):
    micro = []
    for j in range(2):
        ids = torch.randint(2, cfg.vocab, (2, 128), generator=g)
        ids[:, 0] = 1
        lab = ids.clone()
        lab[1, 100:] = -100
        micro.append({"input_ids": ids, "labels": lab})
    tr.optimizer_step(micro, 1e-3)
torch.cuda.synchronize()
t = m.engine.tensors["lm_head"]
src = m.flat_master if m.flat_master is not None else m.flat_params
pads = src[t.offset:t.offset + t.numel].view(t.rows, t.cols)[cfg.vocab:]
pad_max = float(pads.float().abs().max()) if pads.numel() else 0.0
torch.save({"master": (m.flat_master if m.flat_master is not None else m.flat_params).cpu(), "params": m.flat_params.cpu(),
            "ranges": ranges, "n": m.engine.n_params, "head": (t.offset, t.numel), "pad_rows": int(t.rows - cfg.vocab), "pad_max": pad_max,
            "head_moved": bool((m.get_output_embeddings() != head0).any()),
            "seen": tr.state.num_input_tokens_seen, "world": dist.get_world_size() if force else 0}, os.environ["OUT"])
if force:
    dist.destroy_process_group()
'''

HW_QUEUES = str(max(8, int(os.environ.get("GPU_MAX_HW_QUEUES", "8") or 8)))  # the data-parallel step refuses fewer than 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_dp(tmp_path, name, force, comm="", algo="", osd="", **extra_env):
    out = str(tmp_path / f"{name}.pt")
    env = dict(os.environ, SLAM_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), OUT=out,
               SLAM_DP_FORCE="1" if force else "0", COMM=comm, ALGO=algo, OSD=osd, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), GPU_MAX_HW_QUEUES=HW_QUEUES, **extra_env)
    r = subprocess.run([sys.executable, "-c", DP_WORKER], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
def test_untied_rs_ag_and_all_reduce_forced_single_rank_are_bit_identical(tmp_path, osd):
    """test_rs_ag_forced_single_rank_rccl_is_bit_identical on an untied model: after three optimizer steps the parameters and
    master weights of rs_ag and of all_reduce equal the plain step bit for bit, and the ranges reported per step tile
    [0, n_params), lm_head included."""
    comm = "bfloat16" if osd == "bfloat16" else ""
    plain = _run_dp(tmp_path, "plain", False, osd=osd, NORM_PARTIALS="0")  # the chunked norm: the data-parallel summation order
    rs = _run_dp(tmp_path, "rs", True, algo="rs_ag", osd=osd, comm=comm)
    ar = _run_dp(tmp_path, "ar", True, algo="all_reduce", osd=osd, comm=comm)
    assert plain["head_moved"]
    for r in (plain, rs, ar):  # lm_head's pad rows [vocab, vpad) stay zero through three steps with weight decay
        assert r["pad_rows"] == 10 and r["pad_max"] == 0.0
    n = plain["n"]
    assert plain["head"][0] + plain["head"][1] == n
    for other, name in ((rs, "rs_ag"), (ar, "all_reduce")):
        assert other["world"] == 1 and plain["seen"] == other["seen"] > 0
        assert torch.equal(plain["master"], other["master"]), name
        assert torch.equal(plain["params"], other["params"]), name
        assert len(other["ranges"]) == 3
        for rgs in other["ranges"]:
            assert len(rgs) >= 3 and rgs[0][0] == 0
            end = 0
            for off, cnt in rgs:
                assert off == end and cnt > 0
                end = off + cnt
            assert end == n
            assert rgs[-1][0] <= other["head"][0]  # the topmost range holds all of lm_head


# ---- 7. the flat buffers beyond 2^32 elements ---------------------------------------------------------------------------
def test_flat_buffers_beyond_2_to_32_elements():
    """The full Qwen2.5-7B layout (7,615,616,512 parameters, bf16 state): a seeded gradient in three 8192-element windows -
    the first elements, one that straddles element 2^32, the last elements of lm_head - zeros elsewhere; slam_grad_norm
    equals the fp64 norm of the windows to 1e-4 (no window dropped or read twice) and one slam_adamw_step_bf16 through the
    trainer matches O.adamw_update_bf16 on the windows with the bars of test_adamw_bf16_state_step_vs_oracle; everything
    outside the windows changes by weight decay only (strided sample)."""
    free, _ = torch.cuda.mem_get_info()
    if free < 120 * 2 ** 30:
        pytest.skip(f"needs 120 GB of free device memory, {free / 2 ** 30:.0f} GB free")
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    m = UnitLM(UnitLMConfig(base_model_name="Qwen/Qwen2.5-7B", vocab_size=152064, max_tokens=64), seed=3)
    n = m.engine.n_params
    assert n == 7_615_616_512 and n > 2 ** 32 and m.flat_params_t is not None
    t = m.engine.tensors
    assert t["lm_head"].offset + t["lm_head"].numel == n
    tr = SLAMTrainer(model=m, args=SLAMTrainingArguments(optim_state_dtype="bfloat16", weight_decay=0.01, max_grad_norm=0.0,
                                                         logging_steps=0))
    assert m.flat_master is None
    W = 8192
    wins = [0, 2 ** 32 - W // 2, n - W]
    gen = torch.Generator().manual_seed(0)
    m.flat_grads.zero_()
    gw = [torch.randn(W, generator=gen) * 1e-2 for _ in wins]
    for o, g in zip(wins, gw):
        m.flat_grads[o:o + W].copy_(g)
    p0 = [m.flat_params[o:o + W].cpu().clone() for o in wins]
    stride = 1_000_003
    sample = torch.arange(W + 5, n - W, stride, device=m.device)
    sample = sample[(sample < wins[1] - 8) | (sample >= wins[1] + W + 8)]
    s0 = m.flat_params[sample].clone()
    k = "lm.model.layers.17.self_attn.o_proj.weight"
    norm_out = torch.zeros(2, device=m.device)
    m.engine.grad_norm(0.0, norm_out)
    torch.cuda.synchronize()
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in gw))
    print(f"[parity] 7.6e9-element buffer: slam_grad_norm {float(norm_out[0]):.8f}, fp64 norm of the three windows {want:.8f}")
    assert abs(float(norm_out[0]) - want) <= 1e-4 * want
    tr._clip_and_update(1e-3, zero_grad=True)
    torch.cuda.synchronize()
    for o in wins:
        assert float(m.flat_grads[o:o + W].abs().max()) == 0.0
    for o, g, p in zip(wins, gw, p0):
        mo, vo = torch.zeros(W).bfloat16(), torch.zeros(W).bfloat16()
        O.adamw_update_bf16(p, g, mo, vo, 1, 1e-3, wd=0.01)
        got = m.flat_params[o:o + W].cpu()
        assert int((got != p).sum()) <= max(W // 1000, 1), (o, int((got != p).sum()))
        assert float((got.float() - p.float()).abs().max()) <= 2 ** -7 * float(p.float().abs().max()), o
        for mine, ref in ((tr.exp_avg[o:o + W].cpu(), mo), (tr.exp_avg_sq[o:o + W].cpu(), vo)):
            tol = 2.0 ** -5 * ref.float().abs() + 2e-3 * float(ref.float().abs().max())
            assert not bool(((mine.float() - ref.float()).abs() > tol).any()), o
    # outside the windows: g = 0, so m = v = 0 and the parameter only decays: p * (1 - lr * wd), rounded once
    s1 = m.flat_params[sample]
    decayed = (s0.float() * torch.tensor(1 - 1e-3 * 0.01, dtype=torch.float32, device=m.device)).to(torch.bfloat16)
    assert torch.equal(s1, decayed)
    assert float(tr.exp_avg[sample].float().abs().max()) == 0.0 and float(tr.exp_avg_sq[sample].float().abs().max()) == 0.0
    # the transposed images follow the in-place update, also for tensors whose offsets lie beyond 2^32 elements
    for key in (k, HEAD):
        off, shp = m.key_map[key][0], m.key_map[key][1]
        rows = t["lm_head"].rows if key == HEAD else shp[0]
        wt = m.flat_params_t[off:off + rows * shp[1]].view(shp[1], rows)
        assert torch.equal(wt[:, :shp[0]].t().contiguous(), dict(m.named_parameters())[key]), key
    assert m.key_map[HEAD][0] > 2 ** 32
