"""The optimizer kinds of SLAMTrainer, one class each: what a kind keeps on the device, the engine calls of its step, what it can
be combined with, and what its optimizer.pt looks like. The trainer owns everything that is not per kind (the clip, opt_step,
the state precisions, stochastic rounding, the decay mask, the overlapped form's engine option) and never asks which kind it
holds.

`state` maps the checkpoint's own key names to device tensors, in the file's order; a name the kind answers for without keeping
anything under it maps to None (Adafactor's exp_avg / exp_avg_sq). The trainer's `exp_avg`, `exp_avg_sq`, `adafactor_state` and
`muon_momentum` attributes read and write this dict."""
from __future__ import annotations

import logging

import torch

from .training_args import check_muon, check_optim

logger = logging.getLogger(__name__)


def muon_adamw_runs(entries, n_params: int):
    """The contiguous runs of [0, n_params) that no Muon matrix covers - what AdamW updates under optim = "muon" - as
    [(offset, count, state offset)]: the moments of those elements are compact, run after run. `entries` = the rows of
    Engine.muon_set_segments: (offset, rows, cols, pattern), pattern 1 / 2 = 32 rows of every 64, phase 0 / 32."""
    iv = []
    for off, rows, cols, pat in entries:
        if not pat:
            iv.append((off, off + rows * cols))
        else:
            iv.extend((off + (k * 64 + (32 if pat == 2 else 0)) * cols, off + (k * 64 + (32 if pat == 2 else 0) + 32) * cols)
                      for k in range(rows // 32))
    runs, pos, so = [], 0, 0
    for lo, hi in sorted(iv) + [(n_params, n_params)]:
        assert lo >= pos, "Muon segments overlap"
        if lo > pos:
            runs.append((pos, lo - pos, so))
            so += lo - pos
        pos = hi
    return runs


class Optimizer:
    """What the kinds share. A kind declares `options` (the `optim` names that select it, the first one is what messages print),
    what it can be combined with and why not (check_supported), and `file_keys`, the tensors that make an optimizer.pt its own."""
    kind = None
    options = ()
    shardable = False       # ddp_algo = "rs_ag": the step runs on ranges of the flat buffer (step_ranges)
    overlappable = False    # overlap_optimizer
    state_dtypes = ("float32", "bfloat16")
    segments_hook = None    # the model method that names the tensors the kind works on
    tagged = True           # optimizer.pt carries "optim": kind
    workspace_bytes = 0
    check_args = staticmethod(lambda args: None)

    def __init__(self, args, model, state_dtype, moment_dtype):
        self.args, self.model, self.state_dtype = args, model, state_dtype
        self.state = {}

    @property
    def master(self):
        """The fp32 master weights, or None where the bf16 parameters are the only copy."""
        return None if self.state_dtype == torch.bfloat16 else self.model.flat_master

    @property
    def state_bytes(self):
        """(bytes of optimizer state, bytes of workspace) on the device."""
        return sum(t.numel() * t.element_size() for t in self.state.values() if t is not None), self.workspace_bytes

    def state_dict(self):
        head = {"optim": self.kind} if self.tagged else {}
        return {**head, **{k: t.cpu() for k, t in self.state.items() if t is not None}}

    def check_state_sizes(self, st: dict, path: str = "optimizer.pt"):
        for k, t in self.state.items():
            if t is not None and st[k].numel() != t.numel():
                raise ValueError(f"{path} is {self.a_checkpoint} of another model or segment table: {k} has "
                                 f"{st[k].numel()} elements, this run's has {t.numel()}")

    def load_state_dict(self, st: dict):
        for k, t in self.state.items():
            if t is not None:
                t.copy_(st[k])


class AdamW(Optimizer):
    kind = "adamw"
    options = ("adamw_torch", "adamw_torch_fused")
    shardable = overlappable = True
    state_dtypes = ("float32", "bfloat16", "float32_bf16_moments")
    tagged = False          # AdamW's file is older than the key
    file_keys = ("exp_avg", "exp_avg_sq")
    a_checkpoint, holds = "an AdamW checkpoint", "it holds exp_avg / exp_avg_sq, no Adafactor state, no Muon momentum buffer"

    def __init__(self, args, model, state_dtype, moment_dtype):
        super().__init__(args, model, state_dtype, moment_dtype)
        n, dev = model.engine.n_params, model.device
        self.state = {"exp_avg": torch.zeros(n, dtype=moment_dtype, device=dev),
                      "exp_avg_sq": torch.zeros(n, dtype=moment_dtype, device=dev)}

    def step(self, lr, step, norm_out, zero_grad):
        a, eng, s = self.args, self.model.engine, self.state
        if self.state_dtype == torch.bfloat16:
            eng.adamw_step_bf16(s["exp_avg"], s["exp_avg_sq"], norm_out, lr, a.adam_beta1, a.adam_beta2,
                                a.adam_epsilon, a.weight_decay, step, zero_grad=zero_grad)
        else:
            eng.adamw_step(self.model.flat_master, s["exp_avg"], s["exp_avg_sq"], norm_out, lr, a.adam_beta1,
                           a.adam_beta2, a.adam_epsilon, a.weight_decay, step, zero_grad=zero_grad)

    def step_ranges(self, ranges, lr, step, norm_out):
        """The step on [(offset, count)] of the flat buffer only (the shards a rank owns); the gradients are left as they are."""
        a, eng, s, master = self.args, self.model.engine, self.state, self.master
        for off, cnt in ranges:
            eng.adamw_range(off, cnt, master, s["exp_avg"], s["exp_avg_sq"], norm_out, lr, a.adam_beta1, a.adam_beta2,
                            a.adam_epsilon, a.weight_decay, step, zero_grad=False)


class AdamW8bit(Optimizer):
    """AdamW on 8-bit block-wise moments (engine option "adamw_state8"): per moment one byte per element and one fp32 maximum
    per 256 elements of the flat buffer - 2 (1 + 4 / 256) B/param instead of 4. One uint8 allocation per moment, laid out as
    slam_engine.h says; `state` holds the two views of each (codes, absmax), which are what optimizer.pt carries. The step is
    slam_adamw_step_bf16 / _bf16_moments under the option, which is on for the length of the call only: an engine that another
    trainer steps with bf16 moments never sees it."""
    kind = "adamw_8bit"
    options = ("adamw_bnb_8bit",)
    state_dtypes = ("bfloat16", "float32_bf16_moments")
    state_reason = ("keeps both Adam moments in 8 bits: optim_state_dtype is bfloat16 (the bf16 parameters are the only copy) or "
                    "float32_bf16_moments (fp32 master weights)")
    whole_reason = "quantises whole 256-element blocks of the flat buffer"
    file_keys = ("exp_avg_codes", "exp_avg_absmax", "exp_avg_sq_codes", "exp_avg_sq_absmax")
    a_checkpoint, holds = "an 8-bit AdamW checkpoint", "it holds codes and block maxima, no bf16 or fp32 moments"

    def __init__(self, args, model, state_dtype, moment_dtype):
        super().__init__(args, model, state_dtype, moment_dtype)
        from ..engine import Engine
        n = model.engine.n_params
        nbytes, off, blocks = Engine.adam8_state_layout(n)
        self._alloc = [torch.zeros(nbytes, dtype=torch.uint8, device=model.device) for _ in range(2)]
        for name, a in zip(("exp_avg", "exp_avg_sq"), self._alloc):
            self.state[name + "_codes"] = a[:n]
            self.state[name + "_absmax"] = a[off:off + 4 * blocks].view(torch.float32)

    @property
    def state_bytes(self):
        return sum(a.numel() for a in self._alloc), 0

    def step(self, lr, step, norm_out, zero_grad):
        a, eng, (m8, v8) = self.args, self.model.engine, self._alloc
        eng.set_option("adamw_state8", 1)
        try:
            if self.state_dtype == torch.bfloat16:
                eng.adamw_step_bf16(m8, v8, norm_out, lr, a.adam_beta1, a.adam_beta2, a.adam_epsilon, a.weight_decay, step,
                                    zero_grad=zero_grad)
            else:
                eng.adamw_step(self.model.flat_master, m8, v8, norm_out, lr, a.adam_beta1, a.adam_beta2, a.adam_epsilon,
                               a.weight_decay, step, zero_grad=zero_grad)
        finally:
            eng.set_option("adamw_state8", 0)


class Adafactor(Optimizer):
    """HF's Adafactor on slam_adafactor_step. No exp_avg / exp_avg_sq - that is the point: rows + cols fp32 factors per HF matrix,
    numel per vector, and the kernels' partial sums. The table is set once; the engine keeps it."""
    kind = "adafactor"
    options = ("adafactor",)
    segments_hook, segments_what = "hf_param_segments", "HF parameter tensors"
    state_reason = ("keeps no Adam moments: optim_state_dtype is float32 (fp32 master weights) or bfloat16 (the bf16 parameters "
                    "are the only copy)")
    whole_reason = "reduces over the rows and columns of whole tensors"
    file_keys = ("adafactor_state",)
    a_checkpoint, holds = "an Adafactor checkpoint", "it holds no exp_avg / exp_avg_sq"

    def __init__(self, args, model, state_dtype, moment_dtype):
        super().__init__(args, model, state_dtype, moment_dtype)
        n_state, self.workspace_bytes = model.engine.adafactor_set_segments([s.entry for s in model.hf_param_segments()])
        self.state = {"exp_avg": None, "exp_avg_sq": None,
                      "adafactor_state": torch.zeros(n_state, dtype=torch.float32, device=model.device)}
        self._ws = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=model.device)
        model.engine.adafactor_bind_workspace(self._ws)

    def step(self, lr, step, norm_out, zero_grad):  # HF's defaults: eps1 1e-30, clip_threshold 1, decay_rate -0.8; the scheduler's lr
        self.model.engine.adafactor_step(self.master, self.state["adafactor_state"], norm_out, lr, step,
                                         weight_decay=self.args.weight_decay, zero_grad=zero_grad)


class Muon(Optimizer):
    """torch.optim.Muon on slam_muon_step for the decoder layers' matrices, AdamW (slam_adamw_range*) for the rest. 4 B of
    momentum per Muon element, and Adam moments for the OTHER elements only, compact: a full-size exp_avg / exp_avg_sq pair would
    throw away the memory Muon saves. The table and the complement (`adamw_runs`) are computed once."""
    kind = "muon"
    options = ("muon",)
    segments_hook, segments_what = "hf_muon_segments", "decoder matrices"
    state_reason = ("keeps an fp32 momentum buffer and AdamW moments for the non-Muon elements only: optim_state_dtype is float32 "
                    "or bfloat16")
    whole_reason = "orthogonalises whole matrices"
    file_keys = ("muon_momentum", "exp_avg", "exp_avg_sq")
    a_checkpoint, holds = "a Muon checkpoint", "a momentum buffer, AdamW moments for the other elements only"
    check_args = staticmethod(check_muon)

    def __init__(self, args, model, state_dtype, moment_dtype):
        super().__init__(args, model, state_dtype, moment_dtype)
        dev = model.device
        entries = [s.muon_entry for s in model.hf_muon_segments()]
        n_mom, ws_bytes = model.engine.muon_set_segments(entries)
        self.state = {"muon_momentum": torch.zeros(n_mom, dtype=torch.float32, device=dev)}
        self.workspace_bytes = ws_bytes
        self._ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        pad = (-self._ws.data_ptr()) % 256
        model.engine.muon_bind_workspace(self._ws[pad:pad + ws_bytes])
        self.adamw_runs = muon_adamw_runs(entries, model.engine.n_params)
        n_adam = sum(c for _, c, _ in self.adamw_runs)
        self.state["exp_avg"] = torch.zeros(n_adam, dtype=moment_dtype, device=dev)
        self.state["exp_avg_sq"] = torch.zeros(n_adam, dtype=moment_dtype, device=dev)
        es = self.state["exp_avg"].element_size()
        logger.info("optim=muon: %d Muon elements (%.1f MB of momentum), %d AdamW elements (%.1f MB of moments), "
                    "%.1f MB of workspace", n_mom, 4e-6 * n_mom, n_adam, 2e-6 * n_adam * es, 1e-6 * ws_bytes)

    def step(self, lr, step, norm_out, zero_grad):  # the Muon matrices, then AdamW on every run of the flat buffer between them
        a, eng, s, master = self.args, self.model.engine, self.state, self.master
        eng.muon_step(master, s["muon_momentum"], norm_out, lr, step, weight_decay=a.weight_decay,
                      momentum=a.muon_momentum, nesterov=a.muon_nesterov, ns_steps=a.muon_ns_steps,
                      adjust_lr=a.muon_adjust_lr, zero_grad=zero_grad)
        for off, cnt, so in self.adamw_runs:
            eng.adamw_range(off, cnt, master, s["exp_avg"], s["exp_avg_sq"], norm_out, lr, a.adam_beta1, a.adam_beta2,
                            a.adam_epsilon, a.weight_decay, step, zero_grad=zero_grad, state_offset=so)
        eng.refresh_transposed()  # both left the transposed weight images stale


KINDS = {c.kind: c for c in (AdamW, AdamW8bit, Adafactor, Muon)}
BY_OPTION = {o: c for c in KINDS.values() for o in c.options}


def _class_of(args):
    # (fields set after construction get past the arguments' own check)
    return BY_OPTION[check_optim(getattr(args, "optim", "adamw_torch") or "adamw_torch")]


def check_supported(args, model, optim_state_dtype: str):
    """Refuse what the kind `args.optim` names cannot be combined with, from the kind's own declarations."""
    cls = _class_of(args)
    cls.check_args(args)
    who = f"optim={cls.options[0]!r}"
    if optim_state_dtype not in cls.state_dtypes:
        raise ValueError(f"{who} {cls.state_reason}, not {optim_state_dtype}")
    if not cls.shardable and (getattr(args, "ddp_algo", "all_reduce") or "all_reduce") == "rs_ag":
        raise ValueError(f"{who} {cls.whole_reason}: a shard of the flat buffer cuts them, so ddp_algo='rs_ag' is not "
                         f"available (use all_reduce)")
    if not cls.overlappable and getattr(args, "overlap_optimizer", False):
        raise ValueError(f"{who} has no overlapped form: overlap_optimizer belongs to the fp32-state AdamW")
    if cls.segments_hook and not hasattr(model, cls.segments_hook):
        raise ValueError(f"{who} needs a model that knows its {cls.segments_what} (UnitLM.{cls.segments_hook})")


def make_optimizer(args, model, state_dtype, moment_dtype) -> Optimizer:
    """The optimizer `args.optim` names, its state allocated on the model's device and its tables handed to the engine."""
    return _class_of(args)(args, model, state_dtype, moment_dtype)


def check_checkpoint_optim(st: dict, kind: str, path: str = "optimizer.pt"):
    """An optimizer.pt holds the state of ONE optimizer kind: Adafactor's factors ("adafactor_state"), AdamW's moments
    ("exp_avg", "exp_avg_sq"), their 8-bit codes and block maxima ("optim": "adamw_8bit"), or Muon's momentum buffer with the AdamW
    moments of the other elements ("optim": "muon"). Resuming one under another is an error, not a silent zero state. `kind`:
    "adamw", "adamw_8bit", "adafactor" or "muon"."""
    want = KINDS[kind]
    found = next((c for c in (Muon, Adafactor, AdamW8bit) if st.get("optim") == c.kind or c.file_keys[0] in st), AdamW)
    if found is want and all(k in st for k in want.file_keys):
        return
    if found is want:  # the kind's mark without its tensors: what the file lacks is what another kind does not keep
        found = Adafactor if want is AdamW else AdamW
    raise ValueError(f"{path} is {found.a_checkpoint} ({found.holds}): it cannot be resumed under optim={want.options[0]!r}; "
                     f"set optim={found.options[0]!r}")
