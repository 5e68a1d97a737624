"""Evidence run for the optimizer's stochastic rounding (tools only): what does rounding the bf16 optimizer state to nearest cost at the
recipe's final learning rate, and does stochastic rounding ("adamw_sr", optim_stochastic_rounding) recover it? N optimizer steps of
Slam-358M (B 8 x T 1024, clip 0.5, 10 warm-up steps, then constant lr 5e-5 = the schedule's min_lr) on the learnable synthetic stream of
tools/grad_dtype_curve.py, three times from ONE bf16-representable initial state and the same batches:
  fp32 : optim_state_dtype float32 - fp32 master weights and moments (the reference run)
  rtn  : optim_state_dtype bfloat16 - bf16 parameters and moments, round-to-nearest
  sr   : the same with optim_stochastic_rounding
Prints a markdown table of the loss every 20 steps and, per run, |p - p_fp32| / |p_fp32 - p0| over all parameters and the share of
parameters that hold their initial bits at the end.
Usage: python tools/sr_curve.py [steps] >> profiles/stochastic_rounding.md"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slamkit_amd.model import UnitLM, UnitLMConfig
from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
from slamkit_amd.trainer.training_args import lr_lambda

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
B, T, V = 8, 1024, 502
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def batch(i):
    g = torch.Generator().manual_seed(1000 + i)
    start = torch.randint(0, 500, (B, 1), generator=g)
    stride = torch.tensor([1, 3, 7, 11])[torch.randint(0, 4, (B, 1), generator=g)]
    ids = (start + stride * torch.arange(T)[None]) % 500 + 2
    noise = torch.rand(B, T, generator=g) < 0.10
    ids = torch.where(noise, torch.randint(2, V, (B, T), generator=g), ids)
    ids[:, 0] = 1
    return {"input_ids": ids.to(dev), "labels": ids.to(dev)}


def run(osd, sr):
    model = UnitLM(UnitLMConfig(base_model_name="Qwen/Qwen2.5-0.5B", rope_theta=10000.0, vocab_size=V, max_tokens=B * T), seed=0)
    model._weights.copy_(model._weights.to(torch.bfloat16).float())  # one initial state for all three runs: bf16-representable
    model.sync_params_from_master()
    p0 = model._weights.float().clone()
    args = SLAMTrainingArguments(per_device_train_batch_size=B, learning_rate=5e-5, lr_scheduler_type="constant_with_warmup", warmup_steps=10,
                                 max_grad_norm=0.5, logging_steps=0, optim_state_dtype=osd, optim_stochastic_rounding=sr)
    tr = SLAMTrainer(model=model, args=args)
    losses = []
    n = float(B * T)
    for s in range(STEPS):
        tr._loss_acc.zero_()
        tr.optimizer_step([batch(s)], args.learning_rate * lr_lambda(args, s, STEPS), counts=(n, n))
        losses.append(float(tr._loss_acc))
    model.engine.join()
    p = model._weights.float().clone()
    del tr, model
    torch.cuda.empty_cache()
    return losses, p, p0


res = {"fp32": run("float32", False), "rtn": run("bfloat16", False), "sr": run("bfloat16", True)}
print(f"\n## tools/sr_curve.py: Slam-358M, {STEPS} steps at lr 5e-5\n")
print("| step | loss, fp32 master | loss, bf16 round-to-nearest | loss, bf16 stochastic rounding |")
print("|---|---|---|---|")
for s in [0, 9] + list(range(19, STEPS, 20)) + ([STEPS - 1] if (STEPS - 1) % 20 != 19 else []):
    print(f"| {s + 1} | {res['fp32'][0][s]:.4f} | {res['rtn'][0][s]:.4f} | {res['sr'][0][s]:.4f} |")
pf, p0 = res["fp32"][1].double(), res["fp32"][2].double()
assert torch.equal(res["rtn"][2], res["fp32"][2]) and torch.equal(res["sr"][2], res["fp32"][2])
drift = float((pf - p0).norm())
print(f"\n|p_fp32 - p0| = {drift:.4f} over {pf.numel()} parameters\n")
print("| run | \\|p - p_fp32\\| / \\|p_fp32 - p0\\| | share of parameters with their initial bits at the end |")
print("|---|---|---|")
for k in ("fp32", "rtn", "sr"):
    p = res[k][1].double()
    print(f"| {k} | {float((p - pf).norm()) / drift:.4f} | {float((p == p0).double().mean()):.4f} |")
