"""Engine-backed UnitLM: the plugin surface of /root/reference slamkit/model/unit_lm.py
(UnitLMConfig :32-79, UnitLM :82-212, compute_loss :13-29) with the HuggingFace Qwen2 forward /
autograd backward replaced by the gfx950 HIP engine (include/slam_engine.h).

Same call shapes: `model(input_ids, attention_mask, position_ids, labels, num_items_in_batch=...)`
returns an object with `.loss` (fp32 scalar, `.backward()` works) and `.logits [B,T,V]` (bf16);
`log_likelihood`, `generate`, `save_pretrained / from_pretrained` (HF state-dict key layout
`lm.model.layers.{i}.self_attn.q_proj.weight` ..., SURVEY.md §5 checkpoint row) and
`get_input_embeddings / get_output_embeddings` exist. There is no eager fallback: without the
HIP library or a GPU, construction fails.
"""
from __future__ import annotations

import bisect
import json
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from .. import engine as E
from . import generation
from .generation import GenerateOutput, _constraint_plan, _warp  # noqa: F401 - tests and tools import them from here
from .token_lm import TokenLM

# Qwen2.5-0.5B body (config/model/slam.yaml:7 base_model_name) - the hub is unreachable from a
# training box, so the dims the reference pulls via AutoConfig.from_pretrained (unit_lm.py:64)
# are carried here.
KNOWN_BASE_CONFIGS = {
    "Qwen/Qwen2.5-0.5B": dict(num_hidden_layers=24, hidden_size=896, num_attention_heads=14, num_key_value_heads=2,
                              head_dim=64, intermediate_size=4864, rms_norm_eps=1e-6, rope_theta=1000000.0,
                              tie_word_embeddings=True, initializer_range=0.02),
    # interleaved speech-text scale-up body (BASELINE.json configs[3]; dims restated in SURVEY.md §8a-note)
    "Qwen/Qwen2.5-1.5B": dict(num_hidden_layers=28, hidden_size=1536, num_attention_heads=12, num_key_value_heads=2,
                              head_dim=128, intermediate_size=8960, rms_norm_eps=1e-6, rope_theta=1000000.0,
                              tie_word_embeddings=True, initializer_range=0.02),
    # the rest of the Qwen2.5 family the reference's interleaved scaling work uses (docs/SIMS.md: up to SIMS-7B). 7B unties
    # its head and is wider than 2048: the engine's "lm_head" tensor and its two-waves-per-row RMSNorm kernels
    "Qwen/Qwen2.5-3B": dict(num_hidden_layers=36, hidden_size=2048, num_attention_heads=16, num_key_value_heads=2,
                            head_dim=128, intermediate_size=11008, rms_norm_eps=1e-6, rope_theta=1000000.0,
                            tie_word_embeddings=True, initializer_range=0.02),
    "Qwen/Qwen2.5-7B": dict(num_hidden_layers=28, hidden_size=3584, num_attention_heads=28, num_key_value_heads=4,
                            head_dim=128, intermediate_size=18944, rms_norm_eps=1e-6, rope_theta=1000000.0,
                            tie_word_embeddings=False, initializer_range=0.02),
    # Qwen3: the current small Qwen text LMs (per-head q / k RMSNorm, no q/k/v bias, head_dim a field of its own). These
    # numbers restate the published configs and cannot be checked without the hub: a local HuggingFace directory as
    # base_model_name remains the authoritative route (its config.json is read instead)
    "Qwen/Qwen3-0.6B": dict(model_type="qwen3", num_hidden_layers=28, hidden_size=1024, num_attention_heads=16,
                            num_key_value_heads=8, head_dim=128, intermediate_size=3072, rms_norm_eps=1e-6, rope_theta=1000000.0,
                            tie_word_embeddings=True, initializer_range=0.02),
    "Qwen/Qwen3-1.7B": dict(model_type="qwen3", num_hidden_layers=28, hidden_size=2048, num_attention_heads=16,
                            num_key_value_heads=8, head_dim=128, intermediate_size=6144, rms_norm_eps=1e-6, rope_theta=1000000.0,
                            tie_word_embeddings=True, initializer_range=0.02),
    # OPT: the reference's default body (config/model/default.yaml base_model_name) and the TWIST-1.3B body
    "facebook/opt-125m": dict(model_type="opt", num_hidden_layers=12, hidden_size=768, num_attention_heads=12, ffn_dim=3072,
                              max_position_embeddings=2048, init_std=0.02, tie_word_embeddings=True),
    "facebook/opt-1.3b": dict(model_type="opt", num_hidden_layers=24, hidden_size=2048, num_attention_heads=32, ffn_dim=8192,
                              max_position_embeddings=2048, init_std=0.02, tie_word_embeddings=True),
}

ARCH_QWEN2, ARCH_OPT = 0, 1
ARCH_QWEN3 = 3  # 2 is not a family (the engine refuses it)


_HF_DIM_KEYS = ("num_hidden_layers", "hidden_size", "num_attention_heads", "num_key_value_heads", "head_dim",
                "intermediate_size", "rms_norm_eps", "rope_theta", "tie_word_embeddings", "initializer_range")


def dropout_thr16(p: float) -> int:
    """The engine's 16-bit drop threshold of a dropout probability (option "dropout_thr16"): round(p * 65536)."""
    return int(round(float(p) * 65536.0))


# transformers Trainer.get_decay_parameter_names: forbidden_name_patterns (regular expressions searched in the parameter name)
HF_NO_DECAY_PATTERNS = (r"bias", r"layernorm", r"rmsnorm", r"(?:^|\.)norm(?:$|\.)", r"_norm(?:$|\.)")


def hf_name_is_decayed(name: str, is_opt: bool) -> bool:
    """Whether HF's Trainer applies weight_decay to the parameter `name` of a Qwen2 / OPT causal LM. Besides the name patterns
    HF excludes the parameters of every nn.LayerNorm module: OPT's `*_layer_norm` (Qwen2's norms are Qwen2RMSNorm - no
    nn.LayerNorm - and go by name)."""
    if any(re.search(p, name.lower()) for p in HF_NO_DECAY_PATTERNS):
        return False
    return not (is_opt and "layer_norm." in name)


MUON_PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "out_proj", "gate_proj", "up_proj", "down_proj", "fc1", "fc2")


def hf_name_is_muon(name: str) -> bool:
    """Whether optim = "muon" gives the HF parameter `name` to Muon: `<...>.layers.<i>.<...>.<projection>.weight`."""
    parts = name.split(".")
    return "layers" in parts and len(parts) >= 2 and parts[-1] == "weight" and parts[-2] in MUON_PROJECTIONS


@dataclass(frozen=True)
class HFParamSegment:
    """One HF parameter over the engine's flat buffer (UnitLM.hf_param_segments). pattern 0: `rows` contiguous rows of `cols`
    elements at `offset`; 1 / 2: groups of 32 rows every 64 behind `offset`, phase 0 / 32 (gate_proj / up_proj inside wgu)."""
    name: str
    shape: Tuple[int, ...]
    offset: int
    rows: int
    cols: int
    factored: bool
    pattern: int

    @property
    def entry(self) -> Tuple[int, int, int, int, int]:
        return (self.offset, self.rows, self.cols, int(self.factored), self.pattern)

    @property
    def muon_entry(self) -> Tuple[int, int, int, int]:
        return (self.offset, self.rows, self.cols, self.pattern)

    @property
    def state_floats(self) -> int:
        return self.rows + self.cols if self.factored else self.cols


def _opt_base_config(c: dict) -> dict:
    """Engine-side `base_config` of a HuggingFace OPTConfig dict (or of an already converted one: idempotent). Only pre-LN
    OPT as OPTForCausalLM computes it is supported (OPT-125m, OPT-1.3B); OPT-350m's post-LN + project_in/out layout,
    other activations, untied heads and hidden > 2048 are refused. `dropout` (HF OPTConfig's residual dropout, 0.1 by default
    there) is carried, absent meaning 0.0; `attention_dropout`, `activation_dropout` and `layerdrop` are not implemented and
    stay ignored (all three default to 0.0 in HF's OPTConfig)."""
    H = int(c["hidden_size"])
    nH = int(c["num_attention_heads"])
    if not c.get("do_layer_norm_before", True):
        raise ValueError("OPT with do_layer_norm_before=False (post-LN, e.g. OPT-350m) is not supported")
    if c.get("word_embed_proj_dim", H) not in (None, H):
        raise ValueError(f"OPT with word_embed_proj_dim={c['word_embed_proj_dim']} != hidden_size={H} (project_in/out) "
                         "is not supported")
    if not c.get("enable_bias", True):
        raise ValueError("OPT without biases (enable_bias=False) is not supported")
    if not c.get("layer_norm_elementwise_affine", True):
        raise ValueError("OPT LayerNorm without elementwise affine parameters is not supported")
    if c.get("activation_function", "relu") != "relu":
        raise ValueError(f"unsupported OPT activation_function {c.get('activation_function')!r} (relu only)")
    if c.get("_remove_final_layer_norm", False):
        raise ValueError("OPT with _remove_final_layer_norm=True is not supported")
    if not c.get("tie_word_embeddings", True):
        raise ValueError("the engine supports tied embeddings only; this OPT config unties lm_head")
    if H > 2048:
        raise ValueError(f"OPT hidden_size {H} > 2048 is not supported")
    if H % nH or H // nH != 64:
        raise ValueError(f"OPT head_dim {H / nH:g} is not supported (64 only)")
    ffn = c.get("ffn_dim", c.get("intermediate_size"))
    eps = c.get("layer_norm_eps", 1e-5)  # OPTDecoderLayer's nn.LayerNorm default
    p = float(c.get("dropout", 0.0) or 0.0)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"OPT dropout {p} outside [0, 1)")
    return dict(model_type="opt", num_hidden_layers=int(c["num_hidden_layers"]), hidden_size=H, num_attention_heads=nH,
                num_key_value_heads=nH, head_dim=64, intermediate_size=int(ffn),
                max_position_embeddings=int(c["max_position_embeddings"]), layer_norm_eps=float(eps),
                initializer_range=float(c.get("init_std", c.get("initializer_range", 0.02))), tie_word_embeddings=True,
                dropout=p)


def base_config_from_hf(c: dict) -> dict:
    """Engine-side `base_config` from a HuggingFace Qwen2, Qwen3 or OPT config dict (a text-LM `config.json`, or the
    `base_config` object the reference's UnitLMConfig serialises, unit_lm.py:63-73). transformers 4.x stores `rope_theta` at
    the top level, 5.x under `rope_parameters`. OPT and Qwen3 configs keep their model_type ("opt", "qwen3") in the result.
    Qwen3 (dense only: `qwen3_moe` is refused): no q/k/v bias (`attention_bias=True` is refused), full attention in every
    layer, `head_dim` from the config (hidden_size // num_attention_heads when absent)."""
    mt = c.get("model_type", "qwen2")
    if mt == "opt":
        return _opt_base_config(c)
    if mt not in ("qwen2", "qwen3"):
        raise ValueError(f"the engine implements the Qwen2 and OPT decoder families, and Qwen3, only (model_type={mt!r})")
    if c.get("hidden_act", "silu") != "silu":
        raise ValueError(f"unsupported hidden_act {c.get('hidden_act')!r}")
    if c.get("use_sliding_window"):
        raise ValueError("sliding-window attention is not supported")
    out = {k: c[k] for k in _HF_DIM_KEYS if k in c and c[k] is not None}
    if mt == "qwen3":
        if c.get("attention_bias"):
            raise ValueError("Qwen3 with attention_bias=True is not supported (the engine's Qwen3 layers have no q/k/v bias)")
        other = sorted({str(t) for t in (c.get("layer_types") or []) if t != "full_attention"})
        if other:
            raise ValueError(f"Qwen3 layer_types other than 'full_attention' are not supported: {other}")
        out["model_type"] = "qwen3"
        out.setdefault("head_dim", int(c["hidden_size"]) // int(c["num_attention_heads"]))
    rp = c.get("rope_parameters") or c.get("rope_scaling") or {}
    if "rope_theta" not in out and isinstance(rp, dict) and rp.get("rope_theta") is not None:
        out["rope_theta"] = rp["rope_theta"]
    if isinstance(rp, dict) and rp.get("rope_type", rp.get("type", "default")) not in ("default", None):
        raise ValueError(f"unsupported rope scaling {rp}")
    return out


def read_hf_weights(path: str) -> Dict[str, torch.Tensor]:
    """All tensors of a HuggingFace checkpoint directory: `model.safetensors`, the sharded form behind
    `model.safetensors.index.json`, or `pytorch_model.bin`."""
    from safetensors.torch import load_file
    one = os.path.join(path, "model.safetensors")
    idx = one + ".index.json"
    if os.path.exists(one):
        return load_file(one)
    if os.path.exists(idx):
        with open(idx) as f:
            shards = sorted(set(json.load(f)["weight_map"].values()))
        sd: Dict[str, torch.Tensor] = {}
        for sh in shards:
            sd.update(load_file(os.path.join(path, sh)))
        return sd
    b = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(b):
        return torch.load(b, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no model.safetensors / model.safetensors.index.json / pytorch_model.bin under {path}")


@dataclass
class UnitLMConfig:
    """unit_lm.py:32-79. `base_config` is a dict of Qwen2Config-named fields (or None to look
    `base_model_name` up in KNOWN_BASE_CONFIGS); extra kwargs such as `rope_theta` override it the
    way the reference forwards **kwargs into AutoConfig.from_pretrained (config/model/slam.yaml:8)."""
    base_model_name: str = "Qwen/Qwen2.5-0.5B"
    base_config: Optional[dict] = None
    vocab_size: int = 502
    twist_init: bool = False
    use_cache: bool = False
    pad_token_id: int = 0
    bos_token_id: int = 1
    eos_token_id: int = 1
    torch_dtype: Optional[str] = "bfloat16"
    attn_implementation: Optional[str] = "flash_attention_2"  # the engine's attention is varlen-capable
    max_tokens: int = 8192          # engine workspace capacity (B*T per micro-batch)
    extra: dict = field(default_factory=dict)

    def __init__(self, base_model_name="Qwen/Qwen2.5-0.5B", base_config=None, vocab_size=502, twist_init=False,
                 use_cache=False, pad_token_id=0, bos_token_id=1, eos_token_id=1, torch_dtype="bfloat16",
                 attn_implementation="flash_attention_2", max_tokens=8192, tie_word_embeddings=None, **kwargs):
        self.base_model_name = base_model_name
        local_dir = isinstance(base_model_name, str) and os.path.isfile(os.path.join(base_model_name, "config.json"))
        if base_config is None:
            if local_dir:  # "could use a huggingface model name or a path to a model" (unit_lm.py:47)
                with open(os.path.join(base_model_name, "config.json")) as f:
                    base_config = base_config_from_hf(json.load(f))
            elif base_model_name in KNOWN_BASE_CONFIGS:
                base_config = dict(KNOWN_BASE_CONFIGS[base_model_name])
                if base_config.get("model_type") == "opt":
                    base_config = base_config_from_hf(base_config)
            else:
                raise ValueError(f"unknown base model {base_model_name!r}: pass a local HuggingFace directory or "
                                 f"base_config=dict(...) (no hub access); known: {sorted(KNOWN_BASE_CONFIGS)}")
        elif "model_type" in base_config or "rope_parameters" in base_config:
            base_config = base_config_from_hf(base_config)  # the reference's serialised Qwen2Config
        base_config = dict(base_config)
        for k in list(kwargs):
            if k in ("rope_theta", "rms_norm_eps", "initializer_range", "layer_norm_eps"):
                base_config[k] = kwargs.pop(k)
        if "dropout" in kwargs:  # model.config_args.dropout=0.1: the reference's config_args reach OPTConfig the same way
            base_config["dropout"] = float(kwargs.pop("dropout"))
        p_drop = float(base_config.get("dropout", 0.0) or 0.0)
        if base_config.get("model_type") == "opt":
            if not 0.0 <= p_drop < 1.0 or dropout_thr16(p_drop) > 65535:
                raise ValueError(f"dropout {p_drop} outside [0, 65535.5 / 65536)")
            base_config["dropout"] = p_drop
        elif p_drop != 0.0:
            raise ValueError(f"dropout={p_drop}: the Qwen2 family has no residual dropout (OPT only)")
        base_config.setdefault("head_dim", base_config["hidden_size"] // base_config["num_attention_heads"])
        base_config.setdefault("rms_norm_eps", 1e-6)
        base_config.setdefault("rope_theta", 10000.0)
        base_config.setdefault("initializer_range", 0.02)
        if tie_word_embeddings is not None:  # forwarded into the base config, as the reference's **kwargs are
            base_config["tie_word_embeddings"] = bool(tie_word_embeddings)
        base_config.setdefault("tie_word_embeddings", True)
        base_config["tie_word_embeddings"] = bool(base_config["tie_word_embeddings"])
        base_config.update(pad_token_id=pad_token_id, bos_token_id=bos_token_id, eos_token_id=eos_token_id)
        if not base_config["tie_word_embeddings"] and base_config.get("model_type") == "opt":
            raise ValueError("the engine supports tied embeddings only for OPT; this config unties lm_head")
        self.base_config = base_config
        self.vocab_size = vocab_size
        self.twist_init = twist_init
        if twist_init and not local_dir:
            raise ValueError(f"twist_init=True loads the text LM's weights (unit_lm.py:94-98): base_model_name must be a "
                             f"local HuggingFace checkpoint directory (the hub is unreachable), got {base_model_name!r}")
        self.use_cache = use_cache
        self.pad_token_id, self.bos_token_id, self.eos_token_id = pad_token_id, bos_token_id, eos_token_id
        self.torch_dtype = torch_dtype
        self.attn_implementation = attn_implementation
        self._attn_implementation = attn_implementation  # read at cli/train.py:43
        self.max_tokens = max_tokens
        self.tie_word_embeddings = base_config["tie_word_embeddings"]
        self.extra = kwargs

    def to_dict(self):
        return dict(model_type="speech_language_model", engine="slamkit_amd", base_model_name=self.base_model_name,
                    base_config=self.base_config, vocab_size=self.vocab_size, twist_init=False, pad_token_id=self.pad_token_id,
                    bos_token_id=self.bos_token_id, eos_token_id=self.eos_token_id, torch_dtype=self.torch_dtype,
                    max_tokens=self.max_tokens, tie_word_embeddings=self.tie_word_embeddings)

    @property
    def is_opt(self) -> bool:
        return self.base_config.get("model_type") == "opt"

    @property
    def is_qwen3(self) -> bool:
        return self.base_config.get("model_type") == "qwen3"

    def engine_arch(self) -> Tuple[int, int]:
        """(arch, n_positions) of slam_engine_create_arch: Qwen2 = (0, 0), OPT = (1, max_position_embeddings), Qwen3 = (3, 0)."""
        if self.is_opt:
            return ARCH_OPT, int(self.base_config["max_position_embeddings"])
        return (ARCH_QWEN3 if self.is_qwen3 else ARCH_QWEN2), 0

    @property
    def dropout(self) -> float:
        """Residual dropout probability (OPT's `config.dropout`; 0.0 for Qwen2)."""
        return float(self.base_config.get("dropout", 0.0) or 0.0)

    def engine_flags(self) -> int:
        """flags of slam_engine_create_ex: the untied head is a tensor of its own."""
        return 0 if self.tie_word_embeddings else E.MODEL_UNTIED_HEAD

    def engine_desc(self) -> E.SlamModelDesc:
        b = self.base_config
        eps = b["layer_norm_eps"] if self.is_opt else b["rms_norm_eps"]  # OPT: the LayerNorm eps travels in rms_eps
        return E.SlamModelDesc(b["num_hidden_layers"], b["hidden_size"], b["num_attention_heads"],
                               b["num_key_value_heads"], b["head_dim"], b["intermediate_size"], self.vocab_size,
                               self.pad_token_id if self.pad_token_id is not None else -1,
                               float(eps), float(b["rope_theta"]))


@dataclass
class CausalLMOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None

    def __getitem__(self, k):
        return getattr(self, k)


class _EngineLoss(torch.autograd.Function):
    """Lets `out.loss.backward()` drive slam_backward (plugin-surface compatibility). The trainer's
    hot loop calls UnitLM.backward() directly and avoids the host read of grad_output."""

    @staticmethod
    def forward(ctx, anchor, model, loss):
        ctx.model = model
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        ctx.model.backward(float(grad_out))
        return torch.zeros(1, device=grad_out.device), None, None


def _right_padded(mask: torch.Tensor) -> bool:
    m = mask.to(torch.int64)
    return bool((m[:, 1:] <= m[:, :-1]).all())


def mask_spans(mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """A host attention_mask [B, T] read as spans: (starts, lens), int32 CPU tensors [B] - row b's ones are the columns
    starts[b] .. starts[b] + lens[b] - 1. One contiguous run of ones per row: right padding (starts 0), left padding
    (starts + lens = T) or both. A row of zeros or a row with a hole is a ValueError."""
    m = mask != 0
    B, T = m.shape
    lens = m.sum(1)
    if B and int(lens.min()) < 1:
        raise ValueError(f"attention_mask row {int(lens.argmin())} is all zeros: every row needs at least one real token")
    col = torch.arange(T)[None]
    starts = torch.where(m, col, T).amin(1)
    last = torch.where(m, col, -1).amax(1)
    holes = last - starts + 1 != lens
    if bool(holes.any()):
        raise ValueError(f"attention_mask row {int(holes.to(torch.int64).argmax())} has a hole: only one contiguous run of ones "
                         "per row is supported (right, left or both-side padding)")
    return starts.to(torch.int32), lens.to(torch.int32)


class UnitLM(TokenLM):
    """unit_lm.py:82-212 on the HIP engine."""
    base_model_prefix = "lm"

    def __init__(self, config: UnitLMConfig, device: Optional[str] = None, seed: int = 0, allocate_grads: bool = True,
                 _from_pretrained: bool = False):
        if not torch.cuda.is_available():
            raise RuntimeError("slamkit_amd.UnitLM needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.config = config
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        self.engine = E.Engine(config.engine_desc(), *config.engine_arch(), flags=config.engine_flags())
        n = self.engine.n_params
        with torch.cuda.device(self.device):
            self.flat_params = torch.zeros(n, dtype=torch.bfloat16, device=self.device)
            self.flat_master = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.flat_grads = torch.zeros(n, dtype=torch.float32, device=self.device) if allocate_grads else None
            self.engine.bind_params(self.flat_params, self.flat_grads)
            b = config.base_config
            dims = (b["hidden_size"], b["intermediate_size"], b["num_attention_heads"] * b["head_dim"],
                    (b["num_attention_heads"] + 2 * b["num_key_value_heads"]) * b["head_dim"])
            self.flat_params_t = None
            if allocate_grads and all(x % 64 == 0 for x in dims):
                # transposed weight images so dgrad runs on the LDS-DMA GEMM path (training only)
                self.flat_params_t = torch.zeros(n, dtype=torch.bfloat16, device=self.device)
                self.engine.bind_params_t(self.flat_params_t)
            self._ws = None
            self._ws_tokens = 0
            self._recompute = int(os.environ.get("SLAM_RECOMPUTE", "0"))  # measurement override, like the SLAM_* knobs below
            if self._recompute:
                self.engine.set_option("recompute", self._recompute)
            # residual dropout (OPT): on in train() mode only; forward() numbers its armed calls from _drop_call
            self._drop_thr = dropout_thr16(config.dropout)
            self._drop_seed = int(seed)
            self._drop_call = 0
            if self._drop_thr:
                self.engine.set_dropout(self._drop_thr, self._drop_seed)  # before the workspace is sized: it adds buffers
            # NEFTune (set_neftune): off until asked for; forward() numbers its armed calls from _neft_call
            self._neft_alpha = 0.0
            self._neft_seed = int(seed)
            self._neft_call = 0
            self._neft_engine_alpha = 0.0  # what the engine was last given (_arm_neftune)
            self._ensure_workspace(config.max_tokens)
            self._loss_buf = torch.zeros(1, dtype=torch.float32, device=self.device)
            self._anchor = torch.zeros(1, device=self.device, requires_grad=True)
            self.flat_grads16 = None       # bf16 gradients of the step's last backward (enable_bf16_grads)
            self._grads_in_bf16 = False    # the last backward left its final values there, not in flat_grads
        for opt in ("fuse_swiglu", "fuse_dswiglu", "gemm_group_rows", "gemm_glds", "gemm_tn_splits", "gemm_tn_balanced", "gemm_256", "gemm_nt224", "gemm_nt224_min_k", "gemm_256_dswiglu", "gemm_256_persist", "gemm_256_stagger", "gemm_256_stagger_dswiglu", "gemm_256_cohorts", "gemm_256_persist_cus", "gemm_group_cols_256", "gemm_group_rows_256", "gemm_mf32", "gemm_256_w4", "gemm_256_roles", "gemm_256_batch_loads", "gemm_tn224", "gemm_tn224_min_m", "gemm_tn224_max_split", "gemm_tn_bal_bg_max_split", "gemm_tn224_bg_min_m", "gemm_tn224_bg_max_split", "bwd_wgrad_stream", "bwd_aux_side", "bwd_wgrad_cus", "attn_jq", "attn_kw", "attn_nch", "attn_prio", "fuse_adamw_t"):  # tuning overrides, e.g. SLAM_FUSE_SWIGLU=0
            v = os.environ.get("SLAM_" + opt.upper())
            if v is not None:
                self.engine.set_option(opt, int(v))
        self.training = True
        # padding-free execution (HF / TRL `padding_free`): right-padded batches whose row lengths the host knows run as packed
        # segments and skip their pads (slam_forward_unpadded). Off by default; the trainers set it from their arguments.
        self.padding_free = False
        # span masks: host attention masks with left or both-side padding (generate's output, prompt-left / completion-right
        # pairs) run as packed segments from each row's first real column (slam_forward_unpadded_spans). Off by default: a mask
        # that is not right padding then raises as it always did; `forward(..., span_masks=True)` switches one call on.
        self.span_masks = False
        self._last_unpadded = False
        self._unpad_buf = None
        self._smoothing = 0.0  # the engine's label-smoothing epsilon as last set here (_set_label_smoothing)
        self._build_key_map()
        self.init_weights(seed)
        if config.twist_init and not _from_pretrained:
            # TWIST: start from the text LM's weights, keep the first vocab_size embedding rows (unit_lm.py:94-102)
            self.load_hf_text_lm(config.base_model_name)

    # ---- layout ------------------------------------------------------------------------------
    def _build_key_map(self):
        if self.config.is_opt:
            return self._build_key_map_opt()
        b, t = self.config.base_config, self.engine.tensors
        nH, nKV, hd, I = b["num_attention_heads"], b["num_key_value_heads"], b["head_dim"], b["intermediate_size"]
        H = b["hidden_size"]
        self._embed_key = "lm.model.embed_tokens.weight"
        km: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        km["lm.model.embed_tokens.weight"] = (t["embed"].offset, (self.config.vocab_size, H))
        for l in range(b["num_hidden_layers"]):
            p, q = f"lm.model.layers.{l}.", f"layers.{l}."
            o = t[q + "wqkv"].offset
            km[p + "self_attn.q_proj.weight"] = (o, (nH * hd, H))
            km[p + "self_attn.k_proj.weight"] = (o + nH * hd * H, (nKV * hd, H))
            km[p + "self_attn.v_proj.weight"] = (o + (nH + nKV) * hd * H, (nKV * hd, H))
            if self.config.is_qwen3:  # no q/k/v bias; one RMSNorm weight over head_dim for the q heads, one for the k heads
                km[p + "self_attn.q_norm.weight"] = (t[q + "q_norm"].offset, (hd,))
                km[p + "self_attn.k_norm.weight"] = (t[q + "k_norm"].offset, (hd,))
            else:
                o = t[q + "bqkv"].offset
                km[p + "self_attn.q_proj.bias"] = (o, (nH * hd,))
                km[p + "self_attn.k_proj.bias"] = (o + nH * hd, (nKV * hd,))
                km[p + "self_attn.v_proj.bias"] = (o + (nH + nKV) * hd, (nKV * hd,))
            km[p + "self_attn.o_proj.weight"] = (t[q + "wo"].offset, (H, nH * hd))
            o = t[q + "wgu"].offset  # rows interleaved in blocks of 32 gate / 32 up (slam_engine.h)
            km[p + "mlp.gate_proj.weight"] = (o, (I, H), 0)
            km[p + "mlp.up_proj.weight"] = (o, (I, H), 1)
            km[p + "mlp.down_proj.weight"] = (t[q + "wd"].offset, (H, I))
            km[p + "input_layernorm.weight"] = (t[q + "ln1"].offset, (H,))
            km[p + "post_attention_layernorm.weight"] = (t[q + "ln2"].offset, (H,))
        km["lm.model.norm.weight"] = (t["norm"].offset, (H,))
        self._head_key = None
        if not self.config.tie_word_embeddings:  # HF's lm_head.weight under the reference's `lm.` prefix
            self._head_key = "lm.lm_head.weight"
            km[self._head_key] = (t["lm_head"].offset, (self.config.vocab_size, H))
        self.key_map = km

    def _build_key_map_opt(self):
        """HF OPTForCausalLM names under the reference UnitLM's `lm.` prefix (the tied lm_head.weight is not listed)."""
        b, t = self.config.base_config, self.engine.tensors
        H, I, L = b["hidden_size"], b["intermediate_size"], b["num_hidden_layers"]
        km: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        d = "lm.model.decoder."
        self._head_key = None
        self._embed_key = d + "embed_tokens.weight"
        km[d + "embed_tokens.weight"] = (t["embed"].offset, (self.config.vocab_size, H))
        km[d + "embed_positions.weight"] = (t["pos_embed"].offset, (t["pos_embed"].rows, H))
        km[d + "final_layer_norm.weight"] = (t["norm"].offset, (H,))
        km[d + "final_layer_norm.bias"] = (t["norm_b"].offset, (H,))
        for l in range(L):
            p, q = f"{d}layers.{l}.", f"layers.{l}."
            o, ob = t[q + "wqkv"].offset, t[q + "bqkv"].offset
            for j, n in enumerate(("q_proj", "k_proj", "v_proj")):  # wqkv rows are q | k | v
                km[p + f"self_attn.{n}.weight"] = (o + j * H * H, (H, H))
                km[p + f"self_attn.{n}.bias"] = (ob + j * H, (H,))
            km[p + "self_attn.out_proj.weight"] = (t[q + "wo"].offset, (H, H))
            km[p + "self_attn.out_proj.bias"] = (t[q + "bo"].offset, (H,))
            km[p + "self_attn_layer_norm.weight"] = (t[q + "ln1"].offset, (H,))
            km[p + "self_attn_layer_norm.bias"] = (t[q + "ln1_b"].offset, (H,))
            km[p + "fc1.weight"] = (t[q + "w1"].offset, (I, H))
            km[p + "fc1.bias"] = (t[q + "b1"].offset, (I,))
            km[p + "fc2.weight"] = (t[q + "w2"].offset, (H, I))
            km[p + "fc2.bias"] = (t[q + "b2"].offset, (H,))
            km[p + "final_layer_norm.weight"] = (t[q + "ln2"].offset, (H,))
            km[p + "final_layer_norm.bias"] = (t[q + "ln2_b"].offset, (H,))
        self.key_map = km

    def hf_decay_flags(self) -> List[bool]:
        """HF Trainer's weight-decay rule per engine tensor, in `engine.tensors` order: True = decayed. Restated from
        transformers `Trainer.get_decay_parameter_names`: every parameter except those of an nn.LayerNorm and those whose name
        matches one of HF_NO_DECAY_PATTERNS. The rule is applied to the HF names the key map puts into each engine tensor; the
        parts of a fused tensor (wqkv, bqkv, wgu) must agree. Embeddings, OPT's positions and an untied lm_head are decayed."""
        by_tensor: Dict[str, List[str]] = {}
        starts = sorted((t.offset, name) for name, t in self.engine.tensors.items())
        for key, ent in self.key_map.items():
            i = bisect.bisect_right(starts, (ent[0], chr(0x10FFFF))) - 1
            by_tensor.setdefault(starts[i][1], []).append(key)
        flags = []
        for name in self.engine.tensors:
            keys = by_tensor.get(name)
            assert keys, f"engine tensor {name} has no HF name"
            decayed = {hf_name_is_decayed(k, self.config.is_opt) for k in keys}
            assert len(decayed) == 1, f"the HF names of {name} disagree about weight decay: {keys}"
            flags.append(decayed.pop())
        return flags

    def hf_param_segments(self) -> List[HFParamSegment]:
        """The HF parameters over the flat buffer, in `key_map` order: what an optimizer that reduces per HF tensor (Adafactor:
        row and column factors and an update clip of each tensor's own) needs instead of the engine's fused tensors. q_proj /
        k_proj / v_proj and the three q/k/v biases are segments of their own inside wqkv / bqkv, gate_proj / up_proj are the two
        phases of wgu's 32-row groups, the embedding is [vocab][H] without its pad rows, and a tied head is the embedding
        (HF: one parameter). A matrix is factored as HF's Adafactor does it (two or more dimensions), a vector is not.
        `HFParamSegment.entry` is the row of `Engine.adafactor_set_segments`."""
        out = []
        for key, ent in self.key_map.items():
            off, shp = int(ent[0]), tuple(int(s) for s in ent[1])
            if len(shp) == 1:
                out.append(HFParamSegment(key, shp, off, 1, shp[0], False, 0))
            else:
                assert len(shp) == 2, f"{key}: no HF decoder parameter here has more than two dimensions"
                out.append(HFParamSegment(key, shp, off, shp[0], shp[1], True, 1 + int(ent[2]) if len(ent) == 3 else 0))
        return out

    def hf_muon_segments(self) -> List[HFParamSegment]:
        """The subset of hf_param_segments() that optim = "muon" hands to Muon, chosen by HF name: the 2-D weights of the decoder
        layers - q_proj / k_proj / v_proj, o_proj (OPT: out_proj) and the MLP matrices gate_proj / up_proj / down_proj (OPT: fc1 /
        fc2). Token and position embeddings, an untied lm_head, every norm weight (q / k norms included) and every bias are not
        Muon's. `HFParamSegment.muon_entry` is the row of `Engine.muon_set_segments`."""
        return [s for s in self.hf_param_segments() if hf_name_is_muon(s.name) and len(s.shape) == 2]

    def _view(self, flat: torch.Tensor, key: str, writable: bool = False) -> torch.Tensor:
        """HF-named window of a flat engine buffer. gate_proj / up_proj live interleaved in 32-row blocks:
        `writable` returns the strided [I/32, 32, H] view (copy_ from src.view(I//32, 32, H)), otherwise
        an [I, H] copy."""
        ent = self.key_map[key]
        off, shp = ent[0], ent[1]
        if len(ent) == 3:
            I, H = shp
            v = flat[off:off + 2 * I * H].view(I // 32, 2, 32, H)[:, ent[2]]
            return v if writable else v.reshape(I, H)
        n = 1
        for s in shp:
            n *= s
        return flat[off:off + n].view(*shp)

    def _assign(self, flat: torch.Tensor, key: str, src: torch.Tensor):
        v = self._view(flat, key, writable=True)
        v.copy_(src.to(device=flat.device, dtype=flat.dtype).reshape(v.shape))

    def _ensure_workspace(self, tokens: int):
        if tokens <= self._ws_tokens:
            return
        tokens = max(tokens, getattr(self, "_ws_floor", 0))  # after a level change: the size that was bound before it
        nbytes = self.engine.workspace_bytes(tokens)
        self._ws = None
        self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._ws.data_ptr()) % 256
        self._ws_aligned = self._ws[off:off + nbytes]
        self.engine.bind_workspace(self._ws_aligned, tokens)
        self._ws_tokens = tokens

    # ---- activation recomputation (HF's names; a run-time mode: configs and checkpoints do not carry it) ------------------
    supports_gradient_checkpointing = True

    def _set_recompute(self, level: int):
        level = int(level)
        if level == getattr(self, "_recompute", 0):
            return
        torch.cuda.synchronize(self.device)  # nothing in flight may still use the workspace that is about to go
        self.engine.set_option("recompute", level)  # unbinds the workspace: its layout depends on the level
        self._recompute = level
        self._ws_floor = max(self._ws_tokens, getattr(self, "_ws_floor", 0))
        self._ws = None
        self._ws_aligned = None
        self._ws_tokens = 0  # the next forward / prefill binds a workspace of the new layout

    def gradient_checkpointing_enable(self, level: int = 2, gradient_checkpointing_kwargs=None):
        """Recompute activations in backward instead of keeping them: level 2 re-runs each layer's forward from its residual
        stream, level 1 rebuilds only the norm outputs and the MLP activation (slam_set_option "recompute"). Same bits as off."""
        if level not in (1, 2):
            raise ValueError("gradient checkpointing level is 1 (selective) or 2 (full layer)")
        self._set_recompute(level)

    def gradient_checkpointing_disable(self):
        self._set_recompute(0)

    @property
    def is_gradient_checkpointing(self) -> bool:
        return getattr(self, "_recompute", 0) != 0

    # ---- parameters ----------------------------------------------------------------------------
    @torch.no_grad()
    def init_weights(self, seed: int = 0):
        """HF `_init_weights`: N(0, initializer_range) matrices and embeddings, zero biases, unit
        norms, zero padding_idx row of the token table (an untied lm_head is a plain nn.Linear: no zeroed row)
        (unit_lm.py:114-115 -> transformers PreTrainedModel)."""
        std = float(self.config.base_config["initializer_range"])
        g = torch.Generator(device=self.device).manual_seed(seed)
        self.engine.join()
        self._weights.zero_()
        for k in self.key_map:
            v = self._view(self._weights, k, writable=True)
            if k.endswith("norm.weight"):
                v.fill_(1.0)
            elif k.endswith(".bias"):
                v.zero_()
            else:
                v.normal_(0.0, std, generator=g)
        if self.config.pad_token_id is not None and self.config.pad_token_id >= 0:
            # nn.Embedding(padding_idx): the token table only (OPT's position table has no padding row)
            self._view(self._weights, self._embed_key, True)[self.config.pad_token_id].zero_()
        self.sync_params_from_master()

    def sync_params_from_master(self):
        if self.flat_master is not None:
            self.engine.cast_params(self.flat_master)
        else:
            self.engine.refresh_transposed()

    def drop_master(self):
        """bf16-parameter training (the recipe's precision, slam.yaml:9): the bf16 buffer becomes the only copy of the
        weights; the optimizer (slam_adamw_step_bf16) updates it in place."""
        self.engine.join()
        self.flat_master = None

    # ---- decoding from FP8 weights (slam_bind_decode_w8 in the header) ------------------------------------------------------
    def _w8_matrices(self, include_head: bool):
        """(kind, offset, rows, cols) of the matrices the FP8 decode copy covers, in the engine's buffer order."""
        t = self.engine.tensors
        out = []
        for l in range(self.engine.desc.n_layers):
            for kind in ("wqkv", "wo", "wgu", "wd"):
                s = t[f"layers.{l}.{kind}"]
                out.append((kind, s.offset, s.rows, s.cols))
        if include_head:
            s = t["lm_head"] if "lm_head" in t else t["embed"]  # a tied head is the embedding table; its pad rows stay
            out.append(("head", s.offset, self.engine.desc.vocab, s.cols))
        return out

    @torch.no_grad()
    def quantize_decode_weights(self, dtype: str = "fp8_e4m3", include_head: bool = False) -> dict:
        """Replace the decode projections (q|k|v, out, gate|up, down of every layer; the LM head with `include_head`) by their
        nearest values on a per-row power-of-two-scaled e4m3 grid and keep the codes for the decode step: generate, scoring and
        speculative verification then stream one byte per weight instead of two, and every other path computes the same model
        from the bf16 parameters, which now hold those values (so does the fp32 master, if there is one, and a checkpoint saved
        afterwards is an ordinary bf16 checkpoint of the quantised model). With a tied head and `include_head` the embedding
        table is quantised, being the same tensor. Any later write of the parameters (load_state_dict, an optimizer step) drops
        the codes silently; decode goes on in bf16. Returns the relative RMS error per matrix kind and the byte counts."""
        if self.config.is_opt:
            raise ValueError("quantize_decode_weights: the OPT family has no KV-cached decode path")
        if dtype != "fp8_e4m3":
            raise ValueError(f"quantize_decode_weights: unknown dtype {dtype!r} (only 'fp8_e4m3')")
        eng = self.engine
        nbytes = eng.decode_w8_bytes(include_head)
        if nbytes == 0:
            raise ValueError("quantize_decode_weights: hidden_size, intermediate_size and num_attention_heads * head_dim must be "
                             "multiples of 64 for the FP8 decode path")
        eng.join()
        mats = self._w8_matrices(include_head)
        P = self.flat_params
        finite = torch.ones((), dtype=torch.bool, device=self.device)
        for _, off, r, c in mats:
            finite &= torch.isfinite(P[off:off + r * c]).all()
        if not bool(finite):
            raise ValueError("quantize_decode_weights: non-finite weights")
        before = P.clone()
        with torch.cuda.device(self.device):
            buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            a = (-buf.data_ptr()) % 256
            self._w8_buf = buf[a:a + nbytes]
            eng.bind_decode_w8(self._w8_buf, include_head)
            eng.quantize_decode_w8()
        err, ref, bf16_bytes, fp8_bytes = {}, {}, 0, 0
        for kind, off, r, c in mats:
            w, q = before[off:off + r * c].float(), P[off:off + r * c].float()
            err[kind] = err.get(kind, 0.0) + (q - w).double().square().sum()
            ref[kind] = ref.get(kind, 0.0) + w.double().square().sum()
            if self.flat_master is not None:
                self.flat_master[off:off + r * c].copy_(q)
            bf16_bytes += 2 * r * c
            fp8_bytes += r * c + r
        del before
        return {"dtype": dtype, "include_head": bool(include_head), "bf16_bytes": bf16_bytes, "fp8_bytes": fp8_bytes,
                "rel_rms": {k: float((err[k] / ref[k]).sqrt()) if float(ref[k]) > 0 else 0.0 for k in err}}

    def drop_decode_weights(self):
        """Unbind the FP8 codes: decode streams the bf16 parameters again, which keep the quantised values."""
        self.engine.bind_decode_w8(None)
        self._w8_buf = None

    @property
    def decode_weights(self) -> Optional[str]:
        """"fp8_e4m3" while the decode step reads valid FP8 codes, else None."""
        return "fp8_e4m3" if self.engine.decode_w8_state() == 2 else None

    @property
    def _weights(self) -> torch.Tensor:
        """The authoritative flat weight buffer: fp32 master when there is one, else the bf16 parameters."""
        return self.flat_master if self.flat_master is not None else self.flat_params

    def named_parameters(self) -> Iterator[Tuple[str, torch.Tensor]]:
        self.engine.join()  # a pending overlapped optimizer step writes these buffers on the engine's side stream
        for k in self.key_map:
            yield k, self._view(self.flat_params, k)

    def parameters(self) -> Iterator[torch.Tensor]:
        for _, v in self.named_parameters():
            yield v

    def named_grads(self) -> Iterator[Tuple[str, torch.Tensor]]:
        """(name, gradient) of the last backward: views of the fp32 buffer, or - when that backward kept its final values in
        bf16 only (`backward(final=2)`: the reference's own gradient precision) - fp32 copies of the bf16 buffer's windows."""
        self.engine.join()
        for k in self.key_map:
            if self._grads_in_bf16:
                yield k, self._view(self.flat_grads16, k).float()
            else:
                yield k, self._view(self.flat_grads, k)

    def enable_bf16_grads(self):
        """Allocate the bf16 gradient buffer `backward(final=2)` stores the step's final gradient values in."""
        if self.flat_grads16 is None:
            with torch.cuda.device(self.device):
                self.flat_grads16 = torch.zeros(self.engine.n_params, dtype=torch.bfloat16, device=self.device)
        return self.flat_grads16

    def num_parameters(self) -> int:
        return sum(v.numel() for v in self.parameters())

    def state_dict(self, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
        self.engine.join()
        src = self._weights if dtype == torch.float32 else self.flat_params
        return {k: self._view(src, k).detach().to(dtype).cpu().clone() for k in self.key_map}

    @staticmethod
    def _canonical_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Key layouts accepted: the UnitLM layout `lm.model.*` (reference and engine checkpoints) and a raw
        HuggingFace causal LM's `model.*` / `lm_head.weight` (text-LM weights for TWIST initialisation)."""
        if any(k.startswith("lm.") for k in sd):
            return dict(sd)
        if any(k.startswith("decoder.") for k in sd):  # a bare OPTModel (HF's base_model_prefix is "model")
            return {("lm.model." + k if k.startswith("decoder.") else k): v for k, v in sd.items()}
        return {("lm." + k if k.startswith(("model.", "lm_head.")) else k): v for k, v in sd.items()}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """Copies the tensors into the fp32 master and refreshes the bf16 images. A tied model accepts and ignores
        `lm_head.weight`; an untied one requires it and resizes it exactly as the embedding (HF's resize_token_embeddings
        resizes both). The embedding follows `resize_token_embeddings` (unit_lm.py:102): a longer matrix is cut to the first
        vocab_size rows; a shorter one fills the new rows with the mean of the old rows (transformers' mean-resizing
        draws them from N(mean, 1e-9 * cov): within 1e-5 of the mean). Returns (missing, unexpected); with `strict`
        either being non-empty raises."""
        self.engine.join()
        sd = self._canonical_keys(sd)
        missing = [k for k in self.key_map if k not in sd]
        extra = [k for k in sd if k not in self.key_map and not (self._head_key is None and k.endswith("lm_head.weight"))]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: {len(missing)} missing (first: {missing[:4]}), "
                           f"{len(extra)} unexpected (first: {extra[:4]})")
        for k in self.key_map:
            if k in sd:
                src = sd[k]
                shp = self.key_map[k][1]
                if k in (self._embed_key, self._head_key) and src.shape[0] != shp[0]:
                    if src.shape[0] > shp[0]:
                        src = src[:shp[0]]
                    else:
                        src = torch.cat([src.float(), src.float().mean(0, keepdim=True).expand(shp[0] - src.shape[0], -1)])
                if tuple(src.shape) != tuple(shp):
                    raise ValueError(f"{k}: checkpoint shape {tuple(src.shape)} != model shape {tuple(shp)}")
                self._assign(self._weights, k, src)
        self.sync_params_from_master()
        return missing, extra

    def load_hf_text_lm(self, path: str):
        """TWIST initialisation (unit_lm.py:94-102): every weight of a local HuggingFace Qwen2 / Qwen3 / OPT text LM, embedding rows
        resized to vocab_size (an untied text LM's `lm_head` likewise). The text LM must tie or untie its head as the
        model does: a mismatch would drop an untied `lm_head` silently, or leave one at its random initialisation."""
        with open(os.path.join(path, "config.json")) as f:
            c = json.load(f)
        if bool(c.get("tie_word_embeddings", True)) != bool(self.config.tie_word_embeddings):
            raise ValueError(f"text LM tie_word_embeddings={c.get('tie_word_embeddings', True)} does not match the model's "
                             f"({self.config.tie_word_embeddings})")
        want = base_config_from_hf(c)
        if want.get("model_type") != self.config.base_config.get("model_type"):
            raise ValueError(f"text LM model_type {c.get('model_type')!r} does not match the model's")
        keys = ("num_hidden_layers", "hidden_size", "num_attention_heads", "num_key_value_heads", "intermediate_size",
                "max_position_embeddings")
        if self.config.is_qwen3:
            keys += ("head_dim",)  # a field of its own there
        for k in keys:
            if want.get(k) != self.config.base_config.get(k):
                raise ValueError(f"text LM {k}={want.get(k)} != model {k}={self.config.base_config.get(k)}")
        self.load_state_dict(read_hf_weights(path), strict=True)
        return self

    def get_input_embeddings(self):
        return self._view(self.flat_params, self._embed_key)

    def get_output_embeddings(self):
        if self._head_key is not None:
            return self._view(self.flat_params, self._head_key)
        return self.get_input_embeddings()  # tied

    def train(self, mode: bool = True):
        """With `config.dropout` > 0 (OPT) training mode is what turns dropout on: forward() then arms the engine for that
        call. eval(), log_likelihood, sequence_logps and generate never drop. The same holds for NEFTune's noise (set_neftune)."""
        self.training = mode
        return self

    def set_dropout_state(self, seed: Optional[int] = None, call: Optional[int] = None):
        """The dropout generator's seed (64 bits) and / or the number the next training forward is armed with (it counts up
        from there, modulo 2^32). The mask is a function of (seed, call, layer, site, element) alone, so setting both replays
        a forward's mask exactly; the trainer sets `call` before every micro-batch."""
        if seed is not None:
            self._drop_seed = int(seed)
            if self._drop_thr:
                self.engine.set_dropout_seed(self._drop_seed)
        if call is not None:
            if int(call) < 0:
                raise ValueError("dropout call number must be >= 0")
            self._drop_call = int(call)

    def set_neftune(self, alpha: Optional[float], seed: Optional[int] = None):
        """NEFTune (HF `TrainingArguments.neftune_noise_alpha`): uniform noise of magnitude alpha / sqrt(T * H) on the input
        embeddings of every forward() in train() mode, drawn inside the embedding kernel (include/slam_engine.h,
        slam_set_neftune). None or 0 switches it off: the launches are then those of a model that never had the option.
        eval(), log_likelihood, sequence_logps, score_continuations and generate never add noise. `seed`: the generator's 64
        bits (default: the seed set last, initially the model's)."""
        alpha = float(alpha or 0.0)
        if not (alpha >= 0.0 and math.isfinite(alpha)):
            raise ValueError(f"neftune_noise_alpha must be finite and >= 0, got {alpha}")
        if seed is not None:
            self._neft_seed = int(seed)
        self._neft_alpha = alpha
        self._neft_engine_alpha = alpha
        self.engine.set_neftune(alpha, self._neft_seed)

    def set_neftune_state(self, seed: Optional[int] = None, call: Optional[int] = None):
        """The noise generator's seed (64 bits) and / or the number the next training forward is armed with (it counts up
        from there, modulo 2^32). The noise is a function of (seed, call, element) alone, so setting both replays a forward's
        noise exactly; the trainer sets `call` before every micro-batch."""
        if seed is not None:
            self._neft_seed = int(seed)
            self.engine.set_neftune(self._neft_engine_alpha, self._neft_seed)
        if call is not None:
            if int(call) < 0:
                raise ValueError("neftune call number must be >= 0")
            self._neft_call = int(call)

    def _arm_neftune(self, t_run: int, t_passed: int):
        """Arm the engine's next forward when training with NEFTune on. HF's magnitude is alpha / sqrt(T * H) with the T of
        the batch AS PASSED; the engine takes T from the call it runs, so a forward whose token axis was padded up to a
        multiple of 64 (t_run > t_passed) hands the engine alpha * sqrt(t_run / t_passed) for that call."""
        if not (self.training and self._neft_alpha > 0.0):
            return
        a = self._neft_alpha if t_run == t_passed else self._neft_alpha * math.sqrt(t_run / t_passed)
        if a != self._neft_engine_alpha:
            self.engine.set_neftune(a, self._neft_seed)
            self._neft_engine_alpha = a
        self.engine.arm_neftune(self._neft_call & 0xFFFFFFFF)
        self._neft_call += 1

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    # ---- forward / backward ---------------------------------------------------------------------
    def _check_positions(self, T: int, position_ids: Optional[torch.Tensor] = None):
        """OPT's learned positions: the engine clamps indices to its table (a memory guard), the range check is here - HF
        fails where a clamped row would silently give wrong outputs. Device position_ids are read back (OPT only)."""
        if not self.config.is_opt:
            return
        npos = int(self.config.base_config["max_position_embeddings"])
        if position_ids is None:
            if T > npos:
                raise ValueError(f"sequence length {T} exceeds OPT's max_position_embeddings {npos}")
        elif position_ids.numel() and (int(position_ids.min()) < 0 or int(position_ids.max()) >= npos):
            raise ValueError(f"position_ids outside [0, {npos}) (OPT's max_position_embeddings)")

    def _segments(self, position_ids: torch.Tensor):
        """Packed [1, sum T] batches (DataCollatorWithFlattening): per-token sequence bounds from
        position_ids == 0 restarts."""
        pos = position_ids.reshape(-1)
        M = pos.numel()
        idx = torch.arange(M, device=pos.device, dtype=torch.int64)
        is0 = pos == 0
        start = torch.cummax(torch.where(is0, idx, torch.zeros_like(idx)), 0).values
        nxt = torch.where(is0, idx, torch.full_like(idx, M))
        # end = position of the next restart strictly after the token
        nxt_shift = torch.cat([nxt[1:], torch.full((1,), M, device=pos.device, dtype=torch.int64)])
        end = torch.flip(torch.cummin(torch.flip(nxt_shift, [0]), 0).values, [0])
        return start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous()

    def forward(self, input_ids: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                num_items_in_batch=None, return_logits: bool = True, padding_free: Optional[bool] = None, lengths=None,
                label_smoothing: float = 0.0, starts=None, span_masks: Optional[bool] = None, **unused) -> CausalLMOutput:
        """UnitLM.forward (unit_lm.py:135-182). Right padding (what DataCollatorForLanguageModeling produces) never changes
        a real token's output under the causal mask, so the dense route does not read the mask. By default a host
        `attention_mask` that is not right padding is a ValueError, as it always was.

        Span batches: with `span_masks` on (None = `self.span_masks`, False by default) a host mask holds one contiguous run of
        ones per row (a hole or a row of zeros is a ValueError that says so), and one with left or both-side padding
        (`generate`'s output, TRL's prompt-left / completion-right pairs) runs as B packed segments whatever `padding_free`
        says; there is no dense route for it. So does any batch given `starts=` with `lengths=` (lists or CPU tensors of B
        ints: row b's real tokens are the columns starts[b] .. starts[b] + lengths[b] - 1; for device batches), with or without
        the switch. A row's real tokens count positions from 0 (HF's rule for OPT; for RoPE the same relative
        distances), so at its real positions a row gives what it gives run alone. The first real token of a row is never a
        target, pad positions are never executed (labels there add nothing) and their logits are zeros. `position_ids`
        with a span batch is a ValueError. A DEVICE mask is not read back and is taken as right padding.

        `padding_free` (None = `self.padding_free`, False by default): a [B, T] batch without `position_ids` whose row lengths
        are known ON THE HOST - from a host `attention_mask`, or from `lengths` (a list or CPU tensor of B ints in 1 .. T) -
        runs as B packed segments of sum(lengths) tokens (rounded up to 64) instead of B * T positions: the pads are never
        executed. A device mask without `lengths` keeps the padded path (the hot loop does not read it back), and so does a
        batch that carries `position_ids` (the flattening collator's, already packed). Loss, logits ([B, T, V], zeros at pad
        positions), `num_items_in_batch` and backward behave as on the padded path, within rounding. Two differences: `labels`
        that are not -100 at pad positions add loss terms for predicting pads on the padded path and none here; and OPT's
        dropout mask is keyed on the element index of the layout the forward runs, so a token's mask differs from the padded
        run's (still a pure function of seed, call, layer, site and packed index).

        `label_smoothing` (HF `TrainingArguments.label_smoothing_factor`, in [0, 1)): the loss of THIS call is HF's
        `LabelSmoother(epsilon)` over the vocab_size real columns, (1 - eps) * nll + eps * mean_v(-log p_v), summed over the
        valid targets and divided as the plain loss is; backward follows it. A per-call argument, as HF keeps smoothing in the
        trainer: a bare `model(...)` never smooths, and 0 is the plain loss kernels, bit for bit."""
        assert input_ids is not None and input_ids.dim() == 2
        B, T = input_ids.shape
        # collated batches arrive on the host (the trainer's boundary): their masks are read there. A DEVICE mask is not read
        # back - that would stall the host behind the previous step's kernels in the hot loop; callers that build masks on
        # the device (synthetic benches, DPO's padded pairs) construct right padding by definition, or pass starts / lengths.
        span = self._host_spans(B, T, attention_mask, lengths, starts, self.span_masks if span_masks is None else span_masks)
        if span is not None and position_ids is not None:
            raise ValueError("position_ids with a left- or both-side-padded batch: a span batch takes its positions from the mask")
        if position_ids is not None and B > 1 and not position_ids.is_cuda:
            # [B > 1, T] with positions is the dense layout (every row 0..T-1); a packed batch mis-shaped as several rows
            # would silently lose its segment bounds (the engine takes segments from a [1, sum T] row only)
            if not bool((position_ids == torch.arange(T, dtype=position_ids.dtype)[None]).all()):
                raise ValueError("position_ids with batch size > 1 must be plain aranges; packed batches are [1, sum T]")
        self._check_positions(T, position_ids)
        dev = self.device
        nb = not input_ids.is_cuda and input_ids.is_pinned()  # pinned host batches (the trainer's prefetch thread): async H2D
        ids = input_ids.to(dev, torch.int64, non_blocking=nb)
        lab = labels.to(dev, torch.int64, non_blocking=nb) if labels is not None else None
        self._set_label_smoothing(label_smoothing)
        if span is not None:
            return self._forward_unpadded(ids, lab, span[1], num_items_in_batch, return_logits, starts=span[0])
        if (self.padding_free if padding_free is None else padding_free) and position_ids is None:
            lens = self._host_lengths(B, T, attention_mask, lengths)
            if lens is not None:
                return self._forward_unpadded(ids, lab, lens, num_items_in_batch, return_logits)
        self._last_unpadded = False
        pos = position_ids.to(dev, torch.int64, non_blocking=nb) if position_ids is not None else None
        # The LDS-DMA wgrad path needs a token count that is a multiple of 64; collated batches have arbitrary lengths.
        # Right-pad the token axis with pad ids / ignored labels (a dummy trailing segment for packed rows): under the
        # causal mask no real token sees the padding, the loss skips it, and the extra logits rows are not returned.
        T0 = T
        if (B * T) % 64 and (pos is None or B == 1):
            T = -(-T // 64) * 64
            extra = T - T0
            ids = torch.cat([ids, ids.new_full((B, extra), int(self.config.pad_token_id or 0))], 1)
            if lab is not None:
                lab = torch.cat([lab, lab.new_full((B, extra), -100)], 1)
            if pos is not None:
                pos = torch.cat([pos, torch.arange(extra, device=dev, dtype=torch.int64)[None]], 1)
        ids = ids.contiguous()
        lab = lab.contiguous() if lab is not None else None
        self._ensure_workspace(B * T)
        seg_s = seg_e = None
        if pos is not None:
            pos = pos.contiguous()
            if B == 1:
                seg_s, seg_e = self._segments(pos)
        logits = torch.empty(B, T, self.config.vocab_size, dtype=torch.bfloat16, device=dev) if return_logits else None
        if isinstance(num_items_in_batch, torch.Tensor):
            num_items_in_batch = float(num_items_in_batch)
        self._hold = (ids, lab, pos, seg_s, seg_e)  # the engine borrows these until backward
        if self.training and self._drop_thr:  # this forward only: every other entry point runs unarmed, i.e. without dropout
            self.engine.arm_dropout(self._drop_call & 0xFFFFFFFF)
            self._drop_call += 1
        self._arm_neftune(T, T0)
        self.engine.forward(ids, lab, pos, seg_s, seg_e, B, T,
                            float(num_items_in_batch) if num_items_in_batch else 0.0,
                            self._loss_buf if lab is not None else None, logits)
        loss = None
        if lab is not None:
            loss = _EngineLoss.apply(self._anchor, self, self._loss_buf) if torch.is_grad_enabled() else self._loss_buf.clone()
        if logits is not None and T != T0:
            logits = logits[:, :T0]
        return CausalLMOutput(loss=loss, logits=logits)

    __call__ = forward

    def _set_label_smoothing(self, eps: float):
        """The engine keeps epsilon until it is changed: set it only when this call's differs from the last one set."""
        eps = float(eps or 0.0)
        if not 0.0 <= eps < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {eps}")
        if eps != self._smoothing:
            self.engine.set_label_smoothing(eps)
            self._smoothing = eps

    # ---- padding-free execution ----------------------------------------------------------------------
    @staticmethod
    def _host_lengths(B: int, T: int, attention_mask=None, lengths=None) -> Optional[torch.Tensor]:
        """Row lengths (int32 CPU tensor [B]) when the host knows them: `lengths`, else a host attention_mask (right padding
        was checked by the caller). None = unknown (a device mask is never read back)."""
        if lengths is not None:
            if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
                raise ValueError("lengths must live on the host (a list or a CPU tensor): reading them back would stall the step")
            lens = torch.as_tensor(lengths).to(torch.int64).reshape(-1)
        elif attention_mask is not None and not attention_mask.is_cuda:
            lens = (attention_mask != 0).sum(1).to(torch.int64)
        else:
            return None
        if lens.numel() != B or int(lens.min()) < 1 or int(lens.max()) > T:
            raise ValueError(f"padding_free needs {B} row lengths in 1 .. {T}")
        if isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and lengths.dim() == 1:
            return lengths  # as handed over: a pinned tensor (the trainer's prefetch pins DPO's collated lengths) stays pinned
        return lens.to(torch.int32)

    @staticmethod
    def _host_spans(B: int, T: int, attention_mask=None, lengths=None, starts=None, span_masks: bool = False):
        """(starts, lens), int32 CPU tensors [B], when the host knows a SPAN batch: some row's real tokens start past column
        0. From `starts` with `lengths`, else - with `span_masks` on - from a host attention_mask (read by mask_spans, which
        refuses holes and rows of zeros; explicit `lengths` without `starts` mean right padding). With `span_masks` off a host
        mask that is not right padding is refused. None = right padding or unknown: the dense or padding-free routes."""
        if starts is None:
            if attention_mask is None or attention_mask.is_cuda:
                return None
            if not span_masks:
                if not _right_padded(attention_mask):
                    raise ValueError("only right-padded attention_mask is supported by default: switch span masks on (UnitLM.span_masks "
                                     "= True, or span_masks=True for one call) for left- or both-side-padded rows")
                return None
            st, ln = mask_spans(attention_mask)
            if lengths is not None or ln.numel() != B:
                return None
        else:
            if lengths is None:
                raise ValueError("starts needs lengths: a span is (start, length)")
            if any(isinstance(x, torch.Tensor) and x.is_cuda for x in (starts, lengths)):
                raise ValueError("starts and lengths must live on the host (lists or CPU tensors): reading them back would stall the step")
            st = torch.as_tensor(starts).to(torch.int64).reshape(-1)
            ln = torch.as_tensor(lengths).to(torch.int64).reshape(-1)
            if st.numel() != B or ln.numel() != B or int(st.min()) < 0 or int(ln.min()) < 1 or int((st + ln).max()) > T:
                raise ValueError(f"a span batch needs {B} rows with 0 <= starts, 1 <= lengths and starts + lengths <= {T}")
        return (st.to(torch.int32), ln.to(torch.int32)) if bool(st.any()) else None

    def _unpad_scratch(self, B: int, T: int) -> torch.Tensor:
        """The packed batch's arrays live here until backward (slam_unpadded_scratch_bytes; grown, never shrunk)."""
        nbytes = E.unpadded_scratch_bytes(B, T)
        if self._unpad_buf is None or self._unpad_buf.numel() < nbytes + 256:
            self._unpad_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._unpad_buf.data_ptr()) % 256
        return self._unpad_buf[off:off + nbytes]

    def _run_unpadded(self, ids, lab, lens: torch.Tensor, num_items: float, logits=None, starts: Optional[torch.Tensor] = None):
        """slam_forward_unpadded over the device batch ids / lab [B, T] with host lengths `lens` - with host `starts` its span
        form, slam_forward_unpadded_spans. The workspace is sized by B * T (rounded up to 64), not by this step's packed
        count, so it is never rebound from step to step."""
        B, T = ids.shape
        m_packed = -(-int(lens.sum()) // 64) * 64
        self._ensure_workspace(-(-(B * T) // 64) * 64)
        scratch = self._unpad_scratch(B, T)
        # through pinned memory (the caching host allocator hands the block out again only after the copy has run): the
        # hot loop has no blocking pageable copy of its own
        lens_dev = (lens if lens.is_pinned() else lens.pin_memory()).to(self.device, non_blocking=True)
        self._hold = (ids, lab, lens_dev, scratch)  # the engine borrows these until backward
        self._last_unpadded = True
        if starts is not None:
            starts_dev = (starts if starts.is_pinned() else starts.pin_memory()).to(self.device, non_blocking=True)
            self._hold = self._hold + (starts_dev,)
            self.engine.forward_unpadded_spans(ids, lab, starts_dev, lens_dev, B, T, m_packed, scratch, num_items,
                                               self._loss_buf if lab is not None else None, logits)
            return
        self.engine.forward_unpadded(ids, lab, lens_dev, B, T, m_packed, scratch, num_items,
                                     self._loss_buf if lab is not None else None, logits)

    def _forward_unpadded(self, ids, lab, lens, num_items_in_batch, return_logits, starts=None) -> CausalLMOutput:
        B, T = ids.shape
        ids = ids.contiguous()
        lab = lab.contiguous() if lab is not None else None
        logits = torch.empty(B, T, self.config.vocab_size, dtype=torch.bfloat16, device=self.device) if return_logits else None
        if isinstance(num_items_in_batch, torch.Tensor):
            num_items_in_batch = float(num_items_in_batch)
        if self.training and self._drop_thr:  # as forward(): this call only
            self.engine.arm_dropout(self._drop_call & 0xFFFFFFFF)
            self._drop_call += 1
        self._arm_neftune(T, T)  # the engine takes s from the padded width it is given
        self._run_unpadded(ids, lab, lens, float(num_items_in_batch) if num_items_in_batch else 0.0, logits, starts)
        loss = None
        if lab is not None:
            loss = _EngineLoss.apply(self._anchor, self, self._loss_buf) if torch.is_grad_enabled() else self._loss_buf.clone()
        return CausalLMOutput(loss=loss, logits=logits)

    def _lengths_from_pad(self, ids: torch.Tensor) -> torch.Tensor:
        """Row lengths of right-padded token rows from pad_token_id: index of the last non-pad token + 1, at least 1 (pad ids
        inside a row stay in the row). One read-back when `ids` is on the device."""
        T = ids.shape[1]
        real = ids != self.config.pad_token_id
        last = torch.where(real, torch.arange(1, T + 1, device=ids.device)[None], torch.zeros_like(ids)).amax(1)
        return last.clamp_(min=1).to(torch.int32).cpu()

    def backward(self, grad_scale: float = 1.0, bucket_layers: int = 0, bucket_cb=None, final: int = 0):
        """d(loss * grad_scale)/dparams accumulated into `flat_grads` (fp32). final = 1 | 2 marks the last backward of an
        optimizer step (engine option "grad_final_next"): the gradient-norm partials come out of the final-value stores, and
        with 2 the final values are kept in bf16 only (`flat_grads16`; `named_grads` reads them there). With a bucket callback
        (data parallel) `flat_grads16` is also the buffer that crosses the wire: the exchanged gradients stay in it."""
        if final == 2:
            self.engine.set_grad_image(self.enable_bf16_grads())
        self.engine.backward(grad_scale, bucket_layers, bucket_cb, final=final)
        self._grads_in_bf16 = final == 2

    def zero_grad(self):
        self.engine.zero_grads()

    @torch.no_grad()
    def log_likelihood(self, tokens: torch.Tensor, mean_nll: bool, ignore_tokens: Optional[List[int]] = None,
                       padding_free: Optional[bool] = None) -> torch.Tensor:
        """unit_lm.py:184-194 + calc_nll (calculation_utils.py:5-29): pad -> -100, per-sequence
        sum (or mean) of target log-probs. `padding_free` (None = `self.padding_free`): the rows run as packed segments of
        their own lengths, taken from pad_token_id (one read-back per call when `tokens` is on the device)."""
        B, T = tokens.shape
        self._check_positions(T)
        self._set_label_smoothing(0.0)  # a likelihood, never a smoothed loss
        pf = self.padding_free if padding_free is None else padding_free
        lens = self._lengths_from_pad(tokens) if pf else None
        ids = tokens.to(self.device, torch.int64).contiguous()
        lab = ids.clone()
        lab[lab == self.config.pad_token_id] = -100
        if not pf:
            self._ensure_workspace(B * T)
            self._hold = (ids, lab)
            self._last_unpadded = False
        mask = None
        if ignore_tokens is not None:  # logits[:, :, ignore_tokens] = -inf (unit_lm.py:187-188), done inside the CE kernel
            mask = torch.zeros(self.engine.padded_vocab(), dtype=torch.uint8, device=self.device)
            mask[torch.as_tensor(list(ignore_tokens), dtype=torch.long, device=self.device)] = 1
            self.engine.set_logit_mask(mask)
        try:
            if pf:
                self._run_unpadded(ids, lab, lens, 0.0)
            else:
                self.engine.forward(ids, lab, None, None, None, B, T, 0.0, self._loss_buf, None)
        finally:
            if mask is not None:
                torch.cuda.current_stream(self.device).synchronize()  # the kernel reads the mask: keep it alive until done
                self.engine.set_logit_mask(None)
        ll = torch.empty(B, dtype=torch.float32, device=self.device)
        cnt = torch.empty(B, dtype=torch.float32, device=self.device)
        if pf:
            self.engine.seq_loglik_unpadded(B, ll, cnt)
        else:
            self.engine.seq_loglik(lab, B, T, ll, cnt)
        return ll / cnt if mean_nll else ll

    def sequence_logps(self, input_ids: torch.Tensor, labels: torch.Tensor, padding_free: Optional[bool] = None, lengths=None,
                       attention_mask: Optional[torch.Tensor] = None, starts=None, span_masks: Optional[bool] = None):
        """Per-sequence sums of target log-probs over the non-ignored labels (what TRL's DPOTrainer calls
        `chosen_logps` / `rejected_logps`). Leaves the engine ready for `scale_loss_rows` + `backward`:
        d(-logp_b)/dlogits is stored unscaled (num_items = 1). `padding_free` (None = `self.padding_free`) with host `lengths`
        (list or CPU tensor; without them, taken from pad_token_id when `input_ids` is on the host) runs the rows as packed
        segments; a device batch without `lengths` keeps the padded path. A host `attention_mask`, or `starts` with `lengths`,
        is read as `forward` reads it: with `span_masks` on (None = `self.span_masks`) a left- or both-side-padded batch
        (`generate`'s output with its mask) runs as a span batch whatever `padding_free` says, a right-padded mask gives the
        row lengths."""
        B, T = input_ids.shape
        self._check_positions(T)
        self._set_label_smoothing(0.0)  # sequence objectives are defined on the plain log-likelihood
        lens = None
        span = self._host_spans(B, T, attention_mask, lengths, starts, self.span_masks if span_masks is None else span_masks)
        if span is not None:
            span, lens = span
        elif self.padding_free if padding_free is None else padding_free:
            if lengths is None and attention_mask is None and not input_ids.is_cuda:
                lengths = self._lengths_from_pad(input_ids)
            lens = self._host_lengths(B, T, attention_mask, lengths)
        ids = input_ids.to(self.device, torch.int64).contiguous()
        lab = labels.to(self.device, torch.int64).contiguous()
        ll = torch.empty(B, dtype=torch.float32, device=self.device)
        cnt = torch.empty(B, dtype=torch.float32, device=self.device)
        if lens is not None:
            self._run_unpadded(ids, lab, lens, 1.0, starts=span)
            self.engine.seq_loglik_unpadded(B, ll, cnt)
            return ll, cnt
        self._ensure_workspace(B * T)
        self._hold = (ids, lab)
        self._last_unpadded = False
        self.engine.forward(ids, lab, None, None, None, B, T, 1.0, self._loss_buf, None)
        self.engine.seq_loglik(lab, B, T, ll, cnt)
        return ll, cnt

    def backward_sequence_loss(self, seq_coef: torch.Tensor, B: int, T: int, grad_scale: float = 1.0, **kw):
        """Backward of sum_b seq_coef[b] * (-logp_b): seq_coef = d loss / d(-logp_b)."""
        coef = seq_coef.to(self.device, torch.float32).contiguous()
        self._hold = self._hold + (coef,)
        if self._last_unpadded:
            self.engine.scale_loss_unpadded(coef, B)
        else:
            self.engine.scale_loss_rows(coef, B, T)
        self.engine.backward(grad_scale, kw.get("bucket_layers", 0), kw.get("bucket_cb"))
        self._grads_in_bf16 = False

    # ---- KV-cached generation: generation.py ------------------------------------------------------
    _assist_trace = None      # a list: every round appends CPU copies of (chunk, logits_all, n_new before, tgt, n_new after)
    _lookup_trace = None      # the same for prompt lookup, and n_prop behind them
    last_assist_stats = None  # {"rounds", "proposed", "accepted", "tokens"} of the last speculative generate

    @torch.no_grad()
    def generate(self, inputs: Optional[torch.Tensor] = None, generation_config=None, max_new_tokens: Optional[int] = None,
                 do_sample: Optional[bool] = None, temperature: Optional[float] = None, top_k: Optional[int] = None,
                 seed: Optional[int] = None, input_ids: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, bad_words_ids: Optional[List[List[int]]] = None,
                 top_p: Optional[float] = None, eos_token_id=None, pad_token_id: Optional[int] = None,
                 sampler: Optional[str] = None, sample_ids: Optional[torch.Tensor] = None,
                 num_return_sequences: Optional[int] = None, return_logprobs: bool = False,
                 prefill_chunk: Optional[int] = None, no_repeat_ngram_size: Optional[int] = None,
                 min_new_tokens: Optional[int] = None, min_length: Optional[int] = None,
                 begin_suppress_tokens: Optional[List[int]] = None, suppress_tokens: Optional[List[int]] = None,
                 assistant_model: Optional["UnitLM"] = None, num_assistant_tokens: Optional[int] = None,
                 prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: Optional[int] = None,
                 min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                 eta_cutoff: Optional[float] = None, guidance_scale: Optional[float] = None,
                 negative_prompt_ids: Optional[torch.Tensor] = None,
                 negative_prompt_attention_mask: Optional[torch.Tensor] = None, **kwargs):
        """HF `generate` on the engine's KV cache: [B, T_in + n_new] int64, the prompt as passed and then the new tokens, or
        GenerateOutput(sequences, logprobs) under return_logprobs. Explicit arguments override `generation_config`; any other
        keyword is a TypeError. generation.py has every argument's contract. Prompts: inputs / input_ids, attention_mask,
        eos_token_id, pad_token_id. Length: max_new_tokens, min_new_tokens, min_length. Sampling: do_sample, temperature,
        top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, seed, sampler, sample_ids. Bans: bad_words_ids,
        suppress_tokens, begin_suppress_tokens, no_repeat_ngram_size. Outputs: num_return_sequences, return_logprobs. Prefill:
        prefill_chunk. Speculative: assistant_model, num_assistant_tokens, prompt_lookup_num_tokens, max_matching_ngram_size.
        Guidance: guidance_scale, negative_prompt_ids, negative_prompt_attention_mask."""
        return generation.generate(self, generation_config, kwargs, dict(locals()))  # stays the first statement: the arguments

    @torch.no_grad()
    def score_continuations(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, continuations=None,
                            continuation_lengths=None, num_per_prompt: int = 1, score_chunk: Optional[int] = None,
                            prefill_chunk: Optional[int] = None, return_argmax: bool = False,
                            ignore_tokens: Optional[List[int]] = None):
        """This model's log-probs (and greedy choices) of given continuations of the prompts, through the KV cache: the
        scoring half of generate(num_return_sequences=n, return_logprobs=True). The contract is in generation.py."""
        return generation.score_continuations(self, input_ids, attention_mask, continuations, continuation_lengths,
                                              num_per_prompt, score_chunk, prefill_chunk, return_argmax, ignore_tokens)

    # ---- checkpoints (HF layout) ------------------------------------------------------------------
    def save_pretrained(self, save_directory: str, dtype=torch.bfloat16):
        from safetensors.torch import save_file
        os.makedirs(save_directory, exist_ok=True)
        sd = self.state_dict(dtype)
        save_file(sd, os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=1)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, **kwargs) -> "UnitLM":
        """Loads a checkpoint directory written by this engine, by the reference's `UnitLM.save_pretrained`
        (unit_lm.py:200-212: `config.json` with a serialised Qwen2Config or OPTConfig under `base_config`, weights under
        `lm.model.*`) or - as a convenience for converted text LMs - a raw HuggingFace Qwen2 or OPT directory (`model.*`
        keys, or an OPTModel's bare `decoder.*`; pass vocab_size= to resize). Every parameter must be present in the file: a mismatching layout raises instead of
        leaving the model at its random initialisation."""
        path = pretrained_model_name_or_path
        with open(os.path.join(path, "config.json")) as f:
            c = json.load(f)
        vocab = kwargs.pop("vocab_size", None)
        if "base_config" in c:
            base = c["base_config"]
            name = c.get("base_model_name", "local")
        elif c.get("model_type") in ("qwen2", "qwen3") or (c.get("model_type") == "opt" and all(
                k in c for k in ("num_hidden_layers", "hidden_size", "num_attention_heads", "ffn_dim", "max_position_embeddings"))):
            base, name = c, path
        else:
            raise ValueError(f"{path}/config.json is neither a UnitLM config (no `base_config`) nor a complete Qwen2, Qwen3 or OPT "
                             f"config (model_type={c.get('model_type')!r})")
        if not (isinstance(name, str) and (name in KNOWN_BASE_CONFIGS or os.path.isdir(name))):
            name = "local"  # e.g. a hub id or a path of the machine that wrote the checkpoint: the dims are in base_config
        cfg = UnitLMConfig(base_model_name=name, base_config=base,
                           vocab_size=vocab if vocab is not None else c["vocab_size"],
                           pad_token_id=c.get("pad_token_id", base.get("pad_token_id", 0)),
                           bos_token_id=c.get("bos_token_id", base.get("bos_token_id", 1)),
                           eos_token_id=c.get("eos_token_id", base.get("eos_token_id", 1)),
                           max_tokens=kwargs.pop("max_tokens", c.get("max_tokens", 8192)))
        m = cls(cfg, _from_pretrained=True, **kwargs)
        m.load_state_dict(read_hf_weights(path), strict=True)
        return m
