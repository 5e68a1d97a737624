"""Plain-torch restatement of the Qwen3 family for the tests (CPU only, no test functions).

* the contracts of the three per-head q / k RMSNorm kernels (include/slam_engine.h: slam_op_qknorm_rope_fwd,
  slam_op_qknorm_bwd, slam_op_qknorm_rows_f32) in fp64;
* a Qwen3 forward in fp32 that autograd can differentiate - the Qwen2 body of oracle/slam_oracle.py without q/k/v biases and
  with an RMSNorm over head_dim on every q and k head before RoPE (HF Qwen3Attention: q_norm(q_proj(x).view(.., hd)));
* seeded, machine-independent weights: the oracle's counter-hash stream per tensor, every norm-type weight (the two layer
  norms, the final norm, q_norm, k_norm) at 1 + 0.1 x a unit-variance draw so that it matters, everything rounded to bf16.

tests/golden/make_golden_qwen3.py pins `forward` to HF Qwen3ForCausalLM on the same weights (tests/golden/qwen3.npz)."""
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import slam_oracle as O

LOG2E = 1.4426950408889634

# the two tiny bodies (2 layers, vocabulary 502). A: n_heads * head_dim = 512 != hidden. B: head_dim 64 with hidden % 64 == 0
# and QKV % 128 == 0 - the shape at which the Qwen2 family switches to the fused bias + RoPE projection epilogue
CFG_A = dict(model_type="qwen3", num_hidden_layers=2, hidden_size=256, num_attention_heads=4, num_key_value_heads=2,
             head_dim=128, intermediate_size=512, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True,
             initializer_range=0.02)
CFG_B = dict(CFG_A, head_dim=64)
VOCAB = 502
SEED = {"A": 31, "B": 32}
CFGS = {"A": CFG_A, "B": CFG_B}


def hf_keys(cfg: dict, vocab: int = VOCAB, prefix: str = "lm.") -> List[Tuple[str, Tuple[int, ...]]]:
    """State-dict layout of UnitLM(Qwen3ForCausalLM) (tied head: no lm_head.weight)."""
    H, I, hd = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    nH, nKV = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    out = [(prefix + "model.embed_tokens.weight", (vocab, H))]
    for l in range(cfg["num_hidden_layers"]):
        p = f"{prefix}model.layers.{l}."
        out += [(p + "self_attn.q_proj.weight", (nH * hd, H)), (p + "self_attn.k_proj.weight", (nKV * hd, H)),
                (p + "self_attn.v_proj.weight", (nKV * hd, H)), (p + "self_attn.o_proj.weight", (H, nH * hd)),
                (p + "self_attn.q_norm.weight", (hd,)), (p + "self_attn.k_norm.weight", (hd,)),
                (p + "mlp.gate_proj.weight", (I, H)), (p + "mlp.up_proj.weight", (I, H)), (p + "mlp.down_proj.weight", (H, I)),
                (p + "input_layernorm.weight", (H,)), (p + "post_attention_layernorm.weight", (H,))]
    out.append((prefix + "model.norm.weight", (H,)))
    return out


def weights(cfg: dict, seed: int, vocab: int = VOCAB, std: float = 0.02, pad_id: int = 0) -> Dict[str, torch.Tensor]:
    """fp32 tensors holding bf16-representable values, from the oracle's counter hash (no RNG library state)."""
    sd = {}
    for i, (k, shp) in enumerate(hf_keys(cfg, vocab)):
        n = math.prod(shp)
        if k.endswith("norm.weight"):
            t = O._hash_uniform_t(n, seed * 1000 + i, 0.1 * math.sqrt(3.0), 1.0, torch.float32)
        else:
            t = O._hash_uniform_t(n, seed * 1000 + i, std * math.sqrt(3.0), 0.0, torch.float32)
        t = t.reshape(shp)
        if k.endswith("embed_tokens.weight") and pad_id is not None and pad_id >= 0:
            t[pad_id].zero_()
        sd[k] = t.to(torch.bfloat16).float()
    return sd


# ---- kernel contracts (fp64) ----------------------------------------------------------------------------------------------
def _tables(pos: torch.Tensor, hd: int, theta: float):
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    a = pos.double()[:, None] * inv[None]
    a = torch.cat([a, a], -1)
    return a.cos(), a.sin()  # [M, hd]


def head_norm(x: torch.Tensor, w: torch.Tensor, eps: float):
    """x [..., hd] -> (x rstd w, rstd)."""
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return x * rstd * w, rstd[..., 0]


def qknorm_rope_fwd_ref(qkv: torch.Tensor, wq, wk, pos, nH: int, nKV: int, hd: int, theta: float, eps: float):
    """qkv [M, (nH + 2 nKV) hd] (bf16-representable): (the whole row after the call in fp64 - q heads normed, rotated and
    times hd^-0.5 log2(e), k heads normed and rotated, v untouched -, rstd [M, nH + nKV])."""
    M = qkv.shape[0]
    x = qkv.double()
    qk = x[:, :(nH + nKV) * hd].view(M, nH + nKV, hd)
    w = torch.cat([wq.double()[None].expand(nH, hd), wk.double()[None].expand(nKV, hd)])
    y, rstd = head_norm(qk, w[None], eps)
    cos, sin = _tables(pos, hd, theta)
    y = y * cos[:, None] + O.rotate_half(y) * sin[:, None]
    y[:, :nH] *= LOG2E / math.sqrt(hd)
    return torch.cat([y.reshape(M, -1), x[:, (nH + nKV) * hd:]], 1), rstd


def qknorm_bwd_ref(dy: torch.Tensor, raw: torch.Tensor, wq, wk, nH: int, nKV: int, hd: int, eps: float):
    """dy [M, (nH + nKV) hd] = the gradient of y = x rstd w; raw = x: (dx, dw_q [hd], dw_k [hd]) in fp64."""
    M = dy.shape[0]
    x = raw.double().view(M, nH + nKV, hd)
    d = dy.double().view(M, nH + nKV, hd)
    w = torch.cat([wq.double()[None].expand(nH, hd), wk.double()[None].expand(nKV, hd)])[None]
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh = x * rstd
    g = d * w
    dx = rstd * (g - xh * (g * xh).mean(-1, keepdim=True))
    dw = d * xh
    return dx.reshape(M, -1), dw[:, :nH].sum((0, 1)), dw[:, nH:].sum((0, 1))


def qknorm_rows_ref(qkv: torch.Tensor, wq, wk, nH: int, nKV: int, hd: int, eps: float):
    """fp32 rows [B, (nH + 2 nKV) hd]: q and k heads replaced by x rstd w (fp64), v untouched."""
    B = qkv.shape[0]
    x = qkv.double()
    w = torch.cat([wq.double()[None].expand(nH, hd), wk.double()[None].expand(nKV, hd)])[None]
    y, _ = head_norm(x[:, :(nH + nKV) * hd].view(B, nH + nKV, hd), w, eps)
    return torch.cat([y.reshape(B, -1), x[:, (nH + nKV) * hd:]], 1)


# ---- model (fp32, differentiable) -----------------------------------------------------------------------------------------
def forward(cfg: dict, sd: Dict[str, torch.Tensor], input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
            position_ids: Optional[torch.Tensor] = None, packed: bool = False) -> torch.Tensor:
    """Logits [B, T, V] of HF Qwen3ForCausalLM (tied head) under the `lm.` prefix."""
    hd, nH, nKV = cfg["head_dim"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    eps = cfg["rms_norm_eps"]
    E = sd["lm.model.embed_tokens.weight"]
    h = F.embedding(input_ids, E)
    B, T, _ = h.shape
    if position_ids is None:
        position_ids = torch.arange(T)[None].expand(B, T)
    cos, sin = O.rope_cos_sin(position_ids, hd, cfg["rope_theta"], h.dtype)
    mask = O.attention_mask_bool(B, T, attention_mask, position_ids, packed)
    for l in range(cfg["num_hidden_layers"]):
        p = f"lm.model.layers.{l}."
        x = O.rms_norm(h, sd[p + "input_layernorm.weight"], eps)
        q = F.linear(x, sd[p + "self_attn.q_proj.weight"]).view(B, T, nH, hd)
        k = F.linear(x, sd[p + "self_attn.k_proj.weight"]).view(B, T, nKV, hd)
        v = F.linear(x, sd[p + "self_attn.v_proj.weight"]).view(B, T, nKV, hd).transpose(1, 2)
        q = O.rms_norm(q, sd[p + "self_attn.q_norm.weight"], eps).transpose(1, 2)
        k = O.rms_norm(k, sd[p + "self_attn.k_norm.weight"], eps).transpose(1, 2)
        q, k = O.apply_rope(q, k, cos, sin)
        a = O.attention(q, k, v, mask, hd ** -0.5).reshape(B, T, nH * hd)
        h = h + F.linear(a, sd[p + "self_attn.o_proj.weight"])
        x = O.rms_norm(h, sd[p + "post_attention_layernorm.weight"], eps)
        h = h + F.linear(F.silu(F.linear(x, sd[p + "mlp.gate_proj.weight"])) * F.linear(x, sd[p + "mlp.up_proj.weight"]),
                         sd[p + "mlp.down_proj.weight"])
    return F.linear(O.rms_norm(h, sd["lm.model.norm.weight"], eps), E)


def batch():
    """The batch of tests/test_gpu_opt.py::_batch: 3 x 100, lengths 100 / 61 / 17, right-padded with 0."""
    g = torch.Generator().manual_seed(5)
    B, T = 3, 100
    ids = torch.randint(2, VOCAB, (B, T), generator=g)
    lens = [100, 61, 17]
    mask = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    ids = ids.masked_fill(mask == 0, 0)
    labels = ids.masked_fill(mask == 0, -100)
    return ids, mask, labels, lens


def loss_of(logits: torch.Tensor, labels: torch.Tensor, num_items=None) -> torch.Tensor:
    lg, lb = logits[:, :-1].reshape(-1, logits.shape[-1]).float(), labels[:, 1:].reshape(-1)
    if num_items:
        return F.cross_entropy(lg, lb, ignore_index=-100, reduction="sum") / num_items
    return F.cross_entropy(lg, lb, ignore_index=-100)


def loss_and_grads(cfg: dict, sd: Dict[str, torch.Tensor], ids, mask, labels):
    """(logits, loss, {name: gradient}) of `forward` by autograd (leaf copies of sd)."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits = forward(cfg, leaf, ids, attention_mask=mask)
    loss = loss_of(logits, labels)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in leaf.items()}
