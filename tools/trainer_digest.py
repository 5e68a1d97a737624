"""SHA-256 digests of what SLAMTrainer leaves behind, one line per configuration: the trainer-level sibling of step_digest.py
(which drives the engine directly) - the check that a refactor of the trainer's host code trains bit for bit like its parent.

Usage: python tools/trainer_digest.py [--list] [--only TAG] [--save DIR | --resume DIR]
Run it from a checkout of each commit and diff the outputs. A line carries, after three optimizer_steps (two micro-batches each,
fixed synthetic batches) on step_digest.py's small bodies: flat_params, the fp32 master where there is one, norm_out, every
optimizer state tensor read through the trainer's attributes, and the tensors of the optimizer.pt that save_checkpoint writes.
--save keeps each optimizer kind's checkpoint under DIR/<kind>; --resume loads those into fresh trainers, runs one more step and
prints the same digests: a checkpoint of either commit must resume under the other to the lines of its own.
The rs_ag configuration needs a process group (one forced rank) and eight hardware queues: it runs in a child process."""
import argparse
import os
import subprocess
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from step_digest import batch, build, sha  # noqa: E402

STATE_NAMES = ("exp_avg", "exp_avg_sq", "adafactor_state", "muon_momentum")
KINDS = ("adamw_torch", "adafactor", "muon")
RS_AG = "q6/adamw_torch.float32.rs_ag"


def configs():
    """(tag, body, SLAMTrainingArguments fields)"""
    for optim, osds in (("adamw_torch", ("float32", "bfloat16", "float32_bf16_moments")), ("adafactor", ("float32", "bfloat16")),
                        ("muon", ("float32", "bfloat16"))):
        for osd in osds:
            yield f"q6/{optim}.{osd}", "q6", dict(optim=optim, optim_state_dtype=osd)
    for osd in ("bfloat16", "float32_bf16_moments"):
        yield f"q6/adamw_torch.{osd}.sr", "q6", dict(optim_state_dtype=osd, optim_stochastic_rounding=True)
    yield "q6/adamw_torch.float32.decay_hf", "q6", dict(weight_decay_rule="hf", weight_decay=0.1)
    yield "q6/adamw_torch.float32.overlap", "q6", dict(overlap_optimizer=True)
    yield "opt5drop/adamw_torch.float32", "opt5drop", {}
    yield RS_AG, "q6", dict(ddp_algo="rs_ag", ddp_bucket_layers=1)


def make(body, kw, out):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    m = build(body)
    m.train()
    args = SLAMTrainingArguments(logging_steps=0, max_grad_norm=0.5, seed=5, output_dir=out, **{"weight_decay": 0.01, **kw})
    return m, SLAMTrainer(model=m, args=args)


def step(m, tr, k):
    keep = ("input_ids", "attention_mask", "position_ids", "labels")
    micro = [{n: v for n, v in batch(kind, m.config.vocab_size, 10 * k + j).items() if n in keep}
             for j, kind in enumerate(("dense", "packed"))]
    tr.optimizer_step(micro, 1e-3)


def digest(m, tr):
    m.engine.join()
    torch.cuda.synchronize()
    parts = [f"step {tr.opt_step}", f"params {sha(m.flat_params)}"]
    if m.flat_master is not None:
        parts.append(f"master {sha(m.flat_master)}")
    parts.append(f"norm {sha(tr.norm_out)}")
    tr._gather_optimizer_state()
    parts += [f"{n} {sha(getattr(tr, n))}" for n in STATE_NAMES if getattr(tr, n, None) is not None]
    return parts


def file_digest(tr):
    tr.save_checkpoint()
    path = tr._ckpt_dir(tr.state.global_step)
    st = torch.load(os.path.join(path, "optimizer.pt"))
    return [f"file:{k} {sha(v) if isinstance(v, torch.Tensor) else v}" for k, v in st.items()]


def run(tag, body, kw, save):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(save, kw["optim"]) if save and tag in {f"q6/{k}.float32" for k in KINDS} else tmp
        m, tr = make(body, kw, out)
        for k in range(3):
            step(m, tr, k)
        print(tag, " ".join(digest(m, tr) + file_digest(tr)), flush=True)


def resume(kind, root):
    with tempfile.TemporaryDirectory() as tmp:
        m, tr = make("q6", dict(optim=kind), tmp)
        tr._load_checkpoint(os.path.join(root, kind, "checkpoint-3"))
        step(m, tr, 3)
        print(f"resume/{kind}", " ".join(digest(m, tr) + file_digest(tr)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--save", default=None)
    ap.add_argument("--resume", default=None)
    a = ap.parse_args()
    if a.list:
        print("\n".join(t for t, _, _ in configs()))
        return
    forced = os.environ.get("SLAM_DP_FORCE") == "1"
    torch.cuda.set_device(0)
    if forced:
        import torch.distributed as dist
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    if a.resume:
        for kind in KINDS:
            resume(kind, a.resume)
        return
    for tag, body, kw in configs():
        if a.only not in (None, tag):
            continue
        if tag == RS_AG and not forced:  # the process group is process-global state: a fresh process, with its own queues
            env = dict(os.environ, SLAM_DP_FORCE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29517"),
                       GPU_MAX_HW_QUEUES=str(max(8, int(os.environ.get("GPU_MAX_HW_QUEUES", "8") or 8))))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--only", tag], env=env, check=True, timeout=600)
        else:
            run(tag, body, kw, a.save)
    if forced:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
