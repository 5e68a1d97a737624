"""SLAMTrainingArguments: the subset of transformers.TrainingArguments the reference's configs set
(config/training_args/default.yaml) + the two SLAM fields (slam_trainer.py:20-24)."""
import math
from dataclasses import dataclass, field
from typing import Optional


@dataclass
class SLAMTrainingArguments:
    output_dir: str = "./results"
    learning_rate: float = 1e-3
    lr_scheduler_type: str = "cosine_with_min_lr"
    lr_scheduler_kwargs: dict = field(default_factory=lambda: {"min_lr": 5e-5})
    warmup_steps: int = 100
    warmup_ratio: float = 0.01
    max_grad_norm: float = 0.5
    num_train_epochs: float = 1.0
    max_steps: int = -1
    per_device_train_batch_size: int = 8
    per_device_eval_batch_size: int = 8
    gradient_accumulation_steps: int = 1
    weight_decay: float = 0.0
    weight_decay_rule: str = "all"                 # which tensors weight_decay applies to. "all": every element of the flat parameter buffer (the engine's historical behaviour; at weight_decay 0 - every shipped recipe - the two rules coincide). "hf": HF Trainer.create_optimizer's rule - no bias, no LayerNorm / RMSNorm parameter (UnitLM.hf_decay_flags -> slam_set_decay_mask): what reproduces a reference run with a non-zero weight_decay
    optim: str = "adamw_torch"                     # HF's field. "adamw_torch" / "adamw_torch_fused": AdamW (the engine's slam_adamw_* kernels; the two names make the same calls). "adafactor": transformers.optimization.Adafactor as HF's Trainer builds it (scale_parameter = False, relative_step = False, no first moment; lr from the scheduler, clip_grad_norm_ first) on slam_adafactor_step: one fp32 number per row and per column of every HF matrix instead of two Adam moments per element. optim_state_dtype "float32" keeps the fp32 master, "bfloat16" drops it; "float32_bf16_moments", ddp_algo "rs_ag" and overlap_optimizer are refused (there are no moments; a shard cuts rows and columns). adam_beta1 / adam_beta2 / adam_epsilon are unused then
    muon_momentum: float = 0.95                    # optim = "muon" (torch.optim.Muon on slam_muon_step): the decoder layers' matrices (q/k/v/o and the MLP weights, per HF tensor) take Muon - an fp32 momentum buffer, Nesterov, five Newton-Schulz iterations on batched HIP GEMMs -, every other parameter (embeddings, an untied head, norms, biases) AdamW with adam_beta1 / adam_beta2 / adam_epsilon through slam_adamw_range*, with moments for those elements only. optim_state_dtype "float32" or "bfloat16"; "float32_bf16_moments", ddp_algo "rs_ag" and overlap_optimizer are refused
    muon_nesterov: bool = True
    muon_ns_steps: int = 5                         # Newton-Schulz iterations, 1 .. 16
    muon_adjust_lr: Optional[str] = "match_rms_adamw"  # torch's adjust_lr_fn: "match_rms_adamw" (lr * 0.2 sqrt(max(rows, cols)): a recipe tuned for AdamW keeps its lr and weight_decay), "original" (lr * sqrt(max(1, rows / cols))), None (lr as it is)
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    logging_steps: int = 10
    eval_strategy: str = "no"
    eval_steps: int = 1000
    save_steps: int = 0
    save_total_limit: int = 2
    seed: int = 42
    bf16: bool = True
    average_tokens_across_devices: bool = True   # transformers 5.x default (SURVEY.md §8c drift note)
    ddp_bucket_layers: int = 4                     # decoder layers per gradient all-reduce bucket
    ddp_comm_dtype: Optional[str] = "bfloat16"     # gradient buckets cross xGMI in bf16 (the reference's DDP precision: its gradients are bf16; half the bytes); "float32": reduce the fp32 buffer in place
    ddp_algo: str = "all_reduce"                   # "all_reduce": every rank reduces and updates everything (torch DDP's scheme); "rs_ag": reduce-scatter gradients, AdamW on the owned 1/N shard, all-gather bf16 parameters under the next forward (dp.ShardedGradReducer)
    optim_state_dtype: str = "float32"             # "float32": fp32 master weights + fp32 Adam moments (30 B/param per step); "bfloat16": the recipe's own precision (slam.yaml:9) - bf16 parameters and moments updated in place, no master (16 B/param); "float32_bf16_moments": fp32 master + bf16 moments (22 B/param)
    optim_stochastic_rounding: bool = False        # bf16 optimizer state is rounded stochastically instead of to nearest (engine option "adamw_sr"): updates below half an ulp of a bf16 weight or moment - most of them at the schedule's low-lr end - survive on average instead of vanishing; same bytes, same traffic. Needs bf16 state (optim_state_dtype bfloat16: p, m, v; float32_bf16_moments: m, v)
    optim_sr_seed: Optional[int] = None            # seed of that rounding (engine option "adamw_sr_seed"); None = `seed`. The generator is stateless and keyed on the optimizer step: nothing goes into checkpoints, a resumed run repeats the uninterrupted one
    grad_dtype: Optional[str] = None               # precision the FINAL gradients of an optimizer step are kept in for the clip and AdamW: "bfloat16" = the reference's own (bf16 parameters have bf16 .grad, slam.yaml:9): the last backward stores them in bf16 only and emits the norm partials from the same stores; "float32"; None = bfloat16 with optim_state_dtype bfloat16, else float32. Micro-batches always accumulate in fp32
    grad_norm_from_backward: bool = True           # the clip's global norm from the sums of squares the last backward's final-value stores emit (no pass over the gradient buffer); False: the chunked norm pass - the summation order data-parallel runs use (they take the norm after the exchange), for bit-exact comparisons with them
    overwrite_first_grad: bool = True               # first backward of a step stores gradients (no zeroing pass); False = zero in AdamW
    overlap_optimizer: bool = False                # AdamW of the later layers under the next step's first layers (measured neutral: 272.7 vs 273.9 k tok/s)
    gradient_checkpointing: bool = False           # HF's field: recompute each layer's forward in backward (engine option "recompute" = 2) - the activations of 3 layers instead of all; same bits, about a quarter more step time
    recompute_level: Optional[int] = None          # overrides gradient_checkpointing: 1 = selective (norm outputs and the MLP activation only), 2 = full layer
    padding_free: bool = False                     # HF / TRL's name: right-padded batches (the default collator's, DPO's pairs, evaluation) run as packed segments of their own lengths and skip the pad positions (slam_forward_unpadded; UnitLM.padding_free). True switches the models on; False (the default) leaves a model's own switch alone. Same losses within rounding; OPT's dropout masks follow the packed layout
    label_smoothing_factor: float = 0.0            # HF's field: epsilon of transformers' LabelSmoother, in [0, 1). The training loss, the logged `loss` and `eval_loss` become (1 - eps) * nll + eps * mean_v(-log p_v) over the vocab_size columns, computed inside the engine's loss kernels (UnitLM.forward(label_smoothing=), slam_set_label_smoothing). 0 (the default) is the plain loss, bit for bit. SLAMDPOTrainer refuses a non-zero value (TRL's own label_smoothing is another quantity)
    neftune_noise_alpha: Optional[float] = None    # HF's field (NEFTune; HF recommends 5 - 15): uniform noise of magnitude alpha / sqrt(T * H) on the input embeddings of the TRAINING forwards, drawn inside the embedding kernel (UnitLM.set_neftune, slam_set_neftune): no launch and no buffer more. SLAMTrainer.train() switches it on at its start and off when it returns, as HF's Trainer attaches and removes its hook; evaluate() adds none. Stateless, keyed on (seed, rank, optimizer step, micro-batch): nothing goes into checkpoints, a resumed run repeats the uninterrupted one. None or 0 (the default): every launch is what it was without the field. SLAMDPOTrainer refuses a non-zero value
    dataloader_num_workers: int = 0                # > 0: one background thread collates up to two optimizer steps ahead into pinned host memory (SLAMTrainer._micro_batches)
    min_token_id_count: Optional[int] = None
    max_token_id_count: Optional[int] = None
    # accepted for config compatibility, unused by the engine
    eval_accumulation_steps: Optional[int] = None
    use_cpu: bool = False
    ddp_find_unused_parameters: bool = False
    group_by_length: bool = False
    torch_compile: bool = False
    report_to: list = field(default_factory=list)
    run_name: Optional[str] = None

    def __post_init__(self):
        check_weight_decay_rule(self.weight_decay_rule)
        check_optim(self.optim)
        check_muon(self)
        check_label_smoothing(self.label_smoothing_factor)
        check_neftune_alpha(self.neftune_noise_alpha)
        if self.optim_stochastic_rounding and (self.optim_state_dtype or "float32") == "float32":
            raise ValueError("optim_stochastic_rounding needs bf16 optimizer state (optim_state_dtype bfloat16 or "
                             "float32_bf16_moments): with float32 state nothing is rounded")

    def get_sr_seed(self) -> int:
        """Seed of the stochastic rounding: optim_sr_seed, else `seed`."""
        return int(self.seed if self.optim_sr_seed is None else self.optim_sr_seed)

    def get_recompute_level(self) -> int:
        """Engine recomputation level these arguments ask for (0 = off)."""
        if self.recompute_level is not None:
            if self.recompute_level not in (1, 2):
                raise ValueError("recompute_level is 1 or 2 (leave it unset, with gradient_checkpointing false, for none)")
            return int(self.recompute_level)
        return 2 if self.gradient_checkpointing else 0

    def get_warmup_steps(self, num_training_steps: int) -> int:
        """TrainingArguments.get_warmup_steps: warmup_steps wins when > 0, else ceil(ratio * steps)."""
        return self.warmup_steps if self.warmup_steps > 0 else math.ceil(num_training_steps * self.warmup_ratio)


def check_weight_decay_rule(rule) -> str:
    if rule not in ("all", "hf"):
        raise ValueError(f"weight_decay_rule must be 'all' or 'hf', got {rule!r}")
    return rule


OPTIM_ADAMW = ("adamw_torch", "adamw_torch_fused")
OPTIM_NAMES = OPTIM_ADAMW + ("adafactor", "muon")
MUON_ADJUST_LR = ("match_rms_adamw", "original", None)


def check_optim(name) -> str:
    if name not in OPTIM_NAMES:
        raise ValueError(f"optim must be one of 'adamw_torch', 'adamw_torch_fused', 'adafactor' or 'muon', got {name!r}")
    return name


def check_muon(args):
    """The muon_* fields, whatever `optim` is (a typo should not wait for the day the optimizer is switched)."""
    mu = getattr(args, "muon_momentum", 0.95)
    if not (isinstance(mu, (int, float)) and 0.0 <= float(mu) < 1.0):
        raise ValueError(f"muon_momentum must lie in [0, 1), got {mu!r}")
    ns = getattr(args, "muon_ns_steps", 5)
    if not (isinstance(ns, int) and 1 <= ns <= 16):
        raise ValueError(f"muon_ns_steps must be an integer in 1 .. 16, got {ns!r}")
    adj = getattr(args, "muon_adjust_lr", "match_rms_adamw")
    if adj not in MUON_ADJUST_LR:
        raise ValueError(f"muon_adjust_lr must be 'match_rms_adamw', 'original' or None, got {adj!r}")


def check_label_smoothing(eps) -> float:
    eps = float(eps or 0.0)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing_factor must be in [0, 1), got {eps}")
    return eps


def check_neftune_alpha(alpha) -> float:
    """neftune_noise_alpha as a float, None meaning 0 (off); finite and >= 0."""
    alpha = float(alpha or 0.0)
    if not (alpha >= 0.0 and math.isfinite(alpha)):
        raise ValueError(f"neftune_noise_alpha must be finite and >= 0 (None or 0: off), got {alpha}")
    return alpha


def lr_lambda(args: SLAMTrainingArguments, step: int, num_training_steps: int) -> float:
    """Multiplier of learning_rate at optimizer step `step` (0-based, before the update).
    cosine_with_min_lr: transformers/optimization.py:326-333 - linear warmup, then
    0.5(1+cos(pi p))(1-r)+r with r = min_lr/lr; `linear` and `constant` for completeness."""
    warm = args.get_warmup_steps(num_training_steps)
    if step < warm:
        return float(step) / float(max(1, warm))
    kind = args.lr_scheduler_type
    if kind == "constant" or kind == "constant_with_warmup":
        return 1.0
    prog = float(step - warm) / float(max(1, num_training_steps - warm))
    if kind == "linear":
        return max(0.0, 1.0 - prog)
    if kind == "cosine":
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))
    if kind == "cosine_with_min_lr":
        kw = args.lr_scheduler_kwargs or {}
        if "min_lr" in kw and kw["min_lr"] is not None:
            r = kw["min_lr"] / args.learning_rate
        else:
            r = kw.get("min_lr_rate", 0.0)
        f = 0.5 * (1.0 + math.cos(math.pi * prog))
        return max(0.0, f * (1 - r) + r)
    raise ValueError(f"unsupported lr_scheduler_type {kind}")
