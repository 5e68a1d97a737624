"""-m gpu: the data-parallel step on hardware with a 1-rank RCCL group (SLAM_DP_FORCE=1: every collective of the N>1
path runs - gloo token-count all-reduce, per-bucket RCCL all-reduce on the side stream driven by slam_bucket_cb, the
join before clip + AdamW). With one rank a SUM all-reduce is the identity, so the parameters after the steps must be
BIT-IDENTICAL to the plain single-GPU step; the reported bucket ranges must tile [0, n_params) exactly.
Runs in a subprocess: the process group is process-global state."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

WORKER = r'''
import json, os, sys
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
            tie_word_embeddings=True)
m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=512), seed=1)
args = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=2, learning_rate=1e-3,
                             max_grad_norm=0.5, logging_steps=0, ddp_bucket_layers=1,
                             ddp_comm_dtype=os.environ.get("COMM") or None, ddp_algo=os.environ.get("ALGO") or "all_reduce",
                             optim_state_dtype=os.environ.get("OSD") or "float32",
                             grad_norm_from_backward=os.environ.get("NORM_PARTIALS", "1") == "1")
tr = SLAMTrainer(model=m, args=args)
assert tr.reducer.force == force
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
torch.save({"master": (m.flat_master if m.flat_master is not None else m.flat_params).cpu(), "params": m.flat_params.cpu(),
            "params_t": m.flat_params_t.cpu() if m.flat_params_t is not None else None, "gather_ms": m.engine.param_wait_ms(),
            "owned": list(getattr(tr.reducer, "owned", []) or []), "ranges": ranges, "n": m.engine.n_params,
            "seen": tr.state.num_input_tokens_seen, "exposed_ms": tr.reducer.exposed_ms(),
            "world": dist.get_world_size() if force else 0}, os.environ["OUT"])
if force:
    dist.destroy_process_group()
'''

# The data-parallel step refuses fewer than 8 hardware queues (slamkit_amd.check_hw_queues). The workers are fresh processes:
# they get at least that many, whatever the launching environment pinned.
HW_QUEUES = str(max(8, int(os.environ.get("GPU_MAX_HW_QUEUES", "8") or 8)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(tmp_path, name, force, comm="", algo="", osd="", **extra_env):
    import torch
    out = str(tmp_path / f"{name}.pt")
    env = dict(os.environ, SLAM_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), OUT=out,
               SLAM_DP_FORCE="1" if force else "0", COMM=comm, ALGO=algo, OSD=osd, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), GPU_MAX_HW_QUEUES=HW_QUEUES, **extra_env)
    r = subprocess.run([sys.executable, "-c", WORKER], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


def test_dp_forced_single_rank_rccl_is_bit_identical(tmp_path):
    import torch
    # the plain step takes its norm from the partial sums backward emits; a data-parallel step takes it from chunk sums AFTER
    # the exchange: for the bit-exact comparison the plain run sums in that order too (grad_norm_from_backward = False)
    plain = _run(tmp_path, "plain", False, NORM_PARTIALS="0")
    dp = _run(tmp_path, "dp", True)
    assert dp["world"] == 1 and plain["seen"] == dp["seen"] > 0
    assert torch.equal(plain["master"], dp["master"]) and torch.equal(plain["params"], dp["params"])
    n = dp["n"]
    for rs in dp["ranges"]:  # every optimizer step: the reported ranges tile [0, n_params) with no gap or overlap
        assert len(rs) >= 3 and rs[0][0] == 0
        end = 0
        for off, cnt in rs:
            assert off == end and cnt > 0
            end = off + cnt
        assert end == n
    assert all(len(rs) == 0 for rs in plain["ranges"])  # no callback without a group
    assert dp["exposed_ms"] >= 0.0
    # bf16 exchange (the reference's DDP precision): gradients rounded once to bf16 -> close, not identical
    bf = _run(tmp_path, "dp_bf16", True, comm="bfloat16")
    d = (bf["master"] - plain["master"]).abs().max().item()
    print(f"[parity] bf16 gradient exchange vs fp32 after 3 steps: max |dparam| = {d:.2e}")
    assert 0 < d < 5e-3


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
def test_rs_ag_forced_single_rank_rccl_is_bit_identical(tmp_path, osd):
    """ddp_algo = rs_ag through RCCL on one rank (reduce_scatter_tensor / all_gather_into_tensor in place, the chunked
    gradient norm summed by an all-reduce, AdamW per owned range, parameter all-gather on the communication stream with
    the engine waiting per layer in the next forward, transposed weight images refreshed at the next backward): with one
    rank every collective is the identity, so parameters, master weights and transposed images must equal the plain step
    BIT FOR BIT - in both optimizer-state precisions. Round 6: with bf16 state the step's final gradients live in bf16 (the
    reference's own precision) - the matching exchange is the bf16 one, whose image IS that buffer: backward stores it, RCCL
    reduces it in place, the chunked norm and the ranged AdamW read it (no pack, no widening pass)."""
    import torch
    comm = "bfloat16" if osd == "bfloat16" else ""
    plain = _run(tmp_path, "plain", False, osd=osd, NORM_PARTIALS="0")  # the chunked norm: the data-parallel summation order
    rs = _run(tmp_path, "rs", True, algo="rs_ag", osd=osd, comm=comm)
    ar = _run(tmp_path, "ar", True, algo="all_reduce", osd=osd, comm=comm)
    partials = _run(tmp_path, "plain_partials", False, osd=osd)  # the default plain step: same gradients, norm summed in another order
    pa, pb = partials["master"].float(), plain["master"].float()
    frac = float((pa != pb).float().mean())
    rel = float(((pa - pb).abs() / pb.abs().clamp_min(1e-3)).max())
    print(f"[parity] norm from backward's partials vs chunked norm pass, {osd} state, 3 steps: {frac:.2e} of the weights differ, max relative {rel:.2e}")
    # the clip coefficient may differ in its last fp32 bit: with bf16 weights that flips the rounding of isolated elements (one ulp = 2^-7)
    assert rel <= (2.0 ** -7 if osd == "bfloat16" else 1e-5) and frac <= (1e-3 if osd == "bfloat16" else 1.0)
    for other, name in ((rs, "rs_ag"), (ar, "all_reduce")):
        assert other["world"] == 1 and plain["seen"] == other["seen"] > 0
        assert torch.equal(plain["master"], other["master"]), name
        assert torch.equal(plain["params"], other["params"]), name
    n = rs["n"]
    assert rs["owned"] and sum(c for _, c in rs["owned"]) == (n // 8192) * 8192  # world 1: the shards are the whole buckets
    assert rs["gather_ms"] >= 0.0


@pytest.mark.parametrize("algo", ["all_reduce", "rs_ag"])
def test_bf16_exchange_image_written_by_backward_equals_the_pack_pass(tmp_path, algo):
    """bf16 gradient exchange (the default ddp_comm_dtype): the communication image comes out of backward itself
    (slam_set_grad_image: weight-gradient epilogues, slab reduces and the norm / bias finish kernel store the bf16 rounding
    of every final value) - the run must leave exactly the parameters of the run that packs each bucket with a conversion
    pass (SLAM_DP_NO_IMAGE=1), with GA = 2 (the image is written by the accumulating, last micro-batch)."""
    import torch
    img = _run(tmp_path, "img", True, comm="bfloat16", algo=algo)
    pack = _run(tmp_path, "pack", True, comm="bfloat16", algo=algo, SLAM_DP_NO_IMAGE="1")
    assert torch.equal(img["master"], pack["master"]) and torch.equal(img["params"], pack["params"])
    plain = _run(tmp_path, "plain", False)
    assert not torch.equal(img["master"], plain["master"])  # the bf16 rounding of the gradients is really in the path


DPO_WORKER = r'''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["SLAM_ROOT"])
from oracle import slam_oracle as O
from slamkit_amd.model import UnitLM, UnitLMConfig
from slamkit_amd.tokeniser import UnitTokeniser
from slamkit_amd.trainer import DPOConfig, SLAMDPOTrainer

force = os.environ.get("SLAM_DP_FORCE") == "1"
torch.cuda.set_device(0)
if force:
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
cfg = O.TINY
base = dict(num_hidden_layers=3, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads,
            head_dim=cfg.head_dim, intermediate_size=cfg.intermediate, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
            tie_word_embeddings=True)
mk = lambda seed: UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=2048), seed=seed)
pol, ref = mk(1), mk(2)
g = torch.Generator().manual_seed(5)
units = lambda k: "".join(f"<Un{int(u)}>" for u in torch.randint(0, 500, (k,), generator=g))
rows = [{"prompt": units(int(torch.randint(5, 20, (1,), generator=g))), "chosen": units(int(torch.randint(10, 40, (1,), generator=g))),
         "rejected": units(int(torch.randint(10, 40, (1,), generator=g)))} for _ in range(12)]
args = DPOConfig(per_device_train_batch_size=2, gradient_accumulation_steps=2, learning_rate=1e-3, max_grad_norm=0.5, logging_steps=0,
                 max_steps=3, warmup_steps=0, warmup_ratio=0.0, ddp_bucket_layers=1, output_dir="/tmp/unused", beta=0.1,
                 ddp_comm_dtype=os.environ.get("COMM") or None, ddp_algo=os.environ.get("ALGO") or "all_reduce",
                 optim_state_dtype=os.environ.get("OSD") or "float32")
tr = SLAMDPOTrainer(model=pol, ref_model=ref, args=args, train_dataset=rows, processing_class=UnitTokeniser(None, load_fe=False))
assert tr.reducer.force == force
tr.train()
torch.cuda.synchronize()
torch.save({"master": (pol.flat_master if pol.flat_master is not None else pol.flat_params).cpu(), "params": pol.flat_params.cpu(),
            "reducer": type(tr.reducer).__name__, "steps": tr.state.global_step}, os.environ["OUT"])
if force:
    dist.destroy_process_group()
'''


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
def test_dpo_trainer_forced_single_rank_rccl_is_bit_identical(tmp_path, osd):
    """SLAMDPOTrainer through the data-parallel path on a 1-rank RCCL group (bucket callback from backward_sequence_loss,
    reducer, and - under rs_ag - the SHARDED clip + AdamW + parameter all-gather it used to skip): with one rank every
    collective is the identity, so 3 optimizer steps (GA 2) must leave the parameters of the plain DPO run bit for bit, for
    both exchange algorithms; the bf16 exchange (image written by backward) is close, not identical."""
    import torch

    def run(name, force, **env):
        out = str(tmp_path / f"{name}.pt")
        e = dict(os.environ, SLAM_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), OUT=out, OSD=osd,
                 SLAM_DP_FORCE="1" if force else "0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
                 HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), GPU_MAX_HW_QUEUES=HW_QUEUES, **env)
        r = subprocess.run([sys.executable, "-c", DPO_WORKER], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return torch.load(out)

    plain = run("plain", False)
    assert plain["steps"] == 3
    for algo, red in (("rs_ag", "ShardedGradReducer"), ("all_reduce", "GradBucketReducer")):
        got = run(algo, True, ALGO=algo, COMM="float32")
        assert got["reducer"] == red
        assert torch.equal(plain["master"], got["master"]) and torch.equal(plain["params"], got["params"]), algo
    bf = run("rs_bf16", True, ALGO="rs_ag", COMM="bfloat16")
    d = (bf["master"].float() - plain["master"].float()).abs().max().item()
    assert 0 < d < 5e-3, d


W2_WORKER = r'''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["SLAM_ROOT"])
from oracle import slam_oracle as O
from slamkit_amd.model import UnitLM, UnitLMConfig
from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)   # BOTH ranks on the one GPU: gloo moves the buckets through the host, the engine kernels are the real ones
if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
cfg = O.TINY
base = dict(num_hidden_layers=4, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads,
            head_dim=cfg.head_dim, intermediate_size=cfg.intermediate, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
            tie_word_embeddings=True)
m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=512), seed=1)
ga = int(os.environ.get("GA", "1"))
args = SLAMTrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=ga, learning_rate=1e-3,
                             max_grad_norm=0.5, logging_steps=0, ddp_bucket_layers=1,
                             ddp_comm_dtype=os.environ.get("COMM") or None, ddp_algo=os.environ.get("ALGO") or "all_reduce",
                             optim_state_dtype=os.environ.get("OSD") or "float32")
tr = SLAMTrainer(model=m, args=args)
init = (m.flat_master if m.flat_master is not None else m.flat_params).float().cpu().clone()
sd_bf = {k: v.float() for k, v in m.state_dict(torch.bfloat16).items()}   # the weights the engine computes with, HF names
snap = {}
if os.environ.get("SNAP") == "1":   # the exchanged, pre-clip gradients and the loss of optimizer step 1 (for the oracle check)
    _upd = tr._update
    def _snap_update(lr, zero_grad):
        if not snap:
            torch.cuda.synchronize()
            snap["grads"] = {k: v.float().cpu().clone() for k, v in m.named_grads()}  # wherever the exchange left them (fp32 buffer / bf16 image)
            snap["loss_local"] = float(tr._loss_acc)
        return _upd(lr, zero_grad)
    tr._update = _snap_update
g = torch.Generator().manual_seed(0)
batches = []
per_step = 2 * int(os.environ.get("MB", "1"))   # micro-batches per optimizer step over all ranks (MB per rank at world 2)
for step in range(3):
    for j in range(per_step):
        ids = torch.randint(2, cfg.vocab, (2, 128), generator=g)
        ids[:, 0] = 1
        lab = ids.clone()
        lab[1, 100 - 10 * j:] = -100
        batches.append({"input_ids": ids, "labels": lab})
for step in range(3):
    mine = batches[per_step * step + rank: per_step * (step + 1): world] if world > 1 else batches[per_step * step: per_step * (step + 1)]
    tr.optimizer_step(mine, 1e-3)
tr._gather_optimizer_state()
torch.cuda.synchronize()
torch.save({"master": (m.flat_master if m.flat_master is not None else m.flat_params).cpu(), "params": m.flat_params.cpu(),
            "exp_avg": tr.exp_avg.cpu(), "owned": list(getattr(tr.reducer, "owned", []) or []), "seen": tr.state.num_input_tokens_seen,
            "init": init, "grad_norm": float(tr.norm_out[0]), "sd_bf": sd_bf, "snap": snap,
            "step1": [{k: v.clone() for k, v in b.items()} for b in batches[:per_step]]},
           os.environ["OUT"] + f".{rank}")
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
'''


def _run_world(tmp_path, name, world, **env):
    import torch
    out = str(tmp_path / f"{name}.pt")
    port = str(_free_port())
    procs = []
    for r in range(world):
        e = dict(os.environ, SLAM_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), OUT=out, RANK=str(r),
                 WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, GLOO_SOCKET_IFNAME="lo",
                 SLAM_ALLOW_FEW_HW_QUEUES="1", **env)
        procs.append(subprocess.Popen([sys.executable, "-c", W2_WORKER], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
    return [torch.load(out + f".{r}") for r in range(world)]


def _check_step1_against_oracle(r0, r1, comm):
    """T10 against the ORACLE (round-5 verdict: the world-2 runs were only ever compared with the engine itself, so a scale
    error common to both engine paths - the global num_items divisor, `loss *= world` - would have passed): optimizer step 1 of
    the two-rank run restated on the CPU following /root/reference slamkit/trainer/slam_trainer.py:67-71 + HF Trainer
    (transformers/trainer.py num_items_in_batch gathered over ranks and micro-batches; DDP sums what each rank computed from
    ITS micro-batch with the GLOBAL count as divisor) - O.forward_loss_grads on each rank's micro-batch with the global
    `num_items_in_batch`, gradients and losses summed. The engine's exchanged, pre-clip gradient buffer (all_reduce: complete on
    every rank) must have that global norm (5e-3: see the assert), direction per tensor (cosine >= 0.999; >= 0.99 for the norm / bias vectors,
    the suite's bar for them) and the ranks' losses must add up to the oracle's loss (2e-2)."""
    import torch
    from oracle import slam_oracle as O
    from tests.gpu_util import cosine
    cfg = O.OracleConfig(**{**O.TINY.to_dict(), "n_layers": 4})   # W2_WORKER's model
    micro = r0["step1"]
    assert len(micro) == 2 and torch.equal(micro[0]["input_ids"], r1["step1"][0]["input_ids"])
    n_glob = float(sum(int((mb["labels"] != -100).sum()) for mb in micro))   # unshifted count over BOTH ranks (trainer.py:2141-2201)
    tot, loss = None, 0.0
    for mb in micro:   # rank r ran micro[r]
        l, _, g = O.forward_loss_grads(cfg, r0["sd_bf"], mb["input_ids"], mb["labels"], num_items_in_batch=n_glob)
        loss += float(l)
        tot = g if tot is None else {k: tot[k] + g[k] for k in g}
    for r in (r0, r1):
        eg = r["snap"]["grads"]
        assert set(eg) == set(tot)
        n_e = float(torch.cat([v.flatten().double() for v in eg.values()]).norm())
        n_o = float(torch.cat([tot[k].flatten().double() for k in eg]).norm())
        worst = min((cosine(eg[k], tot[k]), k) for k in eg if tot[k].dim() == 2)
        worst_v = min((cosine(eg[k], tot[k]), k) for k in eg if tot[k].dim() == 1)
        # noise of relative size e that is independent of the gradient raises the norm by e^2 / 2: at the suite's cosine bars
        # (0.999 matrices, 0.99 vectors) that is 1e-3 ... 1e-2 of upward bias; measured 2.0e-3 (fp32 wire). A normalisation error
        # (local instead of global count, a missing or doubled `world`) is a factor of ~2.
        assert abs(n_e - n_o) <= 5e-3 * n_o, (comm, n_e, n_o)
        assert worst[0] >= 0.999, (comm, worst)
        assert worst_v[0] >= 0.99, (comm, worst_v)
    loss_e = r0["snap"]["loss_local"] + r1["snap"]["loss_local"]
    print(f"[parity] world 2 step 1 vs ORACLE ({comm} wire): global grad norm engine {n_e:.6f} oracle {n_o:.6f}, worst matrix cosine "
          f"{worst[0]:.6f} ({worst[1]}), worst vector cosine {worst_v[0]:.5f}, loss engine {loss_e:.5f} oracle {loss:.5f}")
    assert abs(loss_e - loss) <= 2e-2, (loss_e, loss)
    assert torch.equal(r0["snap"]["grads"]["lm.model.norm.weight"], r1["snap"]["grads"]["lm.model.norm.weight"])


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
def test_two_ranks_on_one_gpu_real_engine_sharded_equals_replicated(tmp_path, osd):
    """WORLD SIZE 2 with the REAL engine: two processes share the one GPU and exchange over gloo (the buckets travel through
    the host; every kernel - backward with the bf16 image, pack / widen, chunked norm, ranged AdamW, weight-image rebuild - is
    the product's). Unlike the 1-rank RCCL runs the shards are real halves here. Checked after 3 optimizer steps:
      * both ranks hold identical parameters, master weights and (gathered) moments;
      * ddp_algo = rs_ag leaves exactly the bits of ddp_algo = all_reduce, for the fp32 and for the bf16 exchange;
      * the fp32 exchange reproduces the UPDATE of the single-process run that accumulates the same two micro-batches (GA 2):
        the two-rank sum adds the ranks' gradients once, the accumulation adds split-K pieces in another order, and AdamW
        turns rounding-noise gradients into +-lr steps, so the comparison is the relative L2 distance of the whole update;
      * tokens seen are the global count."""
    import torch
    res = {}
    for comm in ("float32", "bfloat16"):
        for algo in ("all_reduce", "rs_ag"):
            r0, r1 = _run_world(tmp_path, f"{comm}_{algo}", 2, COMM=comm, ALGO=algo, OSD=osd, SNAP="1")
            if algo == "all_reduce":
                _check_step1_against_oracle(r0, r1, comm)
            for k in ("master", "params", "exp_avg"):
                assert torch.equal(r0[k], r1[k]), (comm, algo, k, "ranks differ")
            res[(comm, algo)] = r0
        a, b = res[(comm, "all_reduce")], res[(comm, "rs_ag")]
        for k in ("master", "params", "exp_avg"):
            assert torch.equal(a[k], b[k]), (comm, k, float((a[k].float() - b[k].float()).abs().max()))
        own = b["owned"]
        assert own and all(c % 8192 == 0 for _, c in own)
    # two micro-batches per rank (GA 2): the bf16 image is written by an ACCUMULATING backward, the shards are still halves
    ga = {algo: _run_world(tmp_path, f"ga2_{algo}", 2, COMM="bfloat16", ALGO=algo, OSD=osd, GA="2", MB="2")[0] for algo in ("all_reduce", "rs_ag")}
    for k in ("master", "params", "exp_avg"):
        assert torch.equal(ga["all_reduce"][k], ga["rs_ag"][k]), ("GA 2", k)
    (single,) = _run_world(tmp_path, "single", 1, GA="2", OSD=osd)
    two = res[("float32", "rs_ag")]
    assert single["seen"] == two["seen"] > 0
    # AdamW divides by sqrt(v): an element whose gradient is rounding noise moves by +-lr whichever way the noise points, so
    # the comparison is on the UPDATE as a whole (relative L2), not element by element
    du_two, du_one = two["master"].float() - two["init"], single["master"].float() - single["init"]
    rel = float((du_two - du_one).norm() / du_one.norm())
    frac = float(((du_two - du_one).abs() > 1e-5).float().mean())
    print(f"[parity] world 2 on one GPU (real engine, gloo) vs single process GA 2, {osd} state: update rel-L2 {rel:.2e}, "
          f"elements off by > 1e-5: {frac:.2e}")
    assert torch.equal(two["init"], single["init"]) and float(du_one.norm()) > 0
    # AdamW and the clip are invariant to the gradient's scale: the pre-clip global norm of the last step pins the scale itself
    gn2, gn1 = two["grad_norm"], single["grad_norm"]
    print(f"[parity] global gradient norm of step 3: two ranks {gn2:.6f}, single process {gn1:.6f}")
    assert abs(gn2 - gn1) <= (2e-3 if osd == "float32" else 2e-2) * gn1, (gn2, gn1)
    assert res[("float32", "all_reduce")]["grad_norm"] == gn2
    assert rel <= (2e-2 if osd == "float32" else 1e-1), rel


ENGINE_COMM_WORKER = r'''
import os, sys
import torch
sys.path.insert(0, os.environ["SLAM_ROOT"])
from oracle import slam_oracle as O
from slamkit_amd.engine import Engine
from slamkit_amd.model import UnitLM, UnitLMConfig

torch.cuda.set_device(0)
cfg = O.TINY
base = dict(num_hidden_layers=4, hidden_size=cfg.hidden, num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads,
            head_dim=cfg.head_dim, intermediate_size=cfg.intermediate, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
            tie_word_embeddings=True)
m = UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=cfg.vocab, max_tokens=512), seed=1)
eng = m.engine
g = torch.Generator().manual_seed(0)
ids = torch.randint(2, cfg.vocab, (2, 128), generator=g)
ids[:, 0] = 1

def run(exchange, bf16, rs=False):
    m.zero_grad()
    out = m(input_ids=ids, labels=ids, return_logits=False)
    losses.append(float(out.loss))
    ranges = []
    stage = None
    if bf16:
        stage = torch.full((eng.n_params,), float("nan"), dtype=torch.bfloat16, device="cuda")
        eng.set_grad_image(stage)
    def cb(off, cnt, ready):
        ranges.append((off, cnt))
        if exchange:
            (eng.reduce_scatter_grads_async if rs else eng.allreduce_grads_async)(off, cnt, bf16, ready)
    eng.set_option("grad_overwrite_next", 1)
    eng.backward(1.0, 1, cb)
    if exchange:
        eng.comm_finish()
    torch.cuda.synchronize()
    return m.flat_grads.clone(), ranges, stage

losses = []
plain, ranges0, _ = run(False, False)
eng.comm_init(Engine.comm_unique_id(), 0, 1)   # a 1-rank RCCL communicator: SUM is the identity
f32, ranges1, _ = run(True, False)
b16, ranges2, stage = run(True, True)
# the reduce-scatter / all-gather form: with one rank the owned shard is the whole bucket and the gather is the identity
f32_rs, ranges3, _ = run(True, False, rs=True)
b16_rs, ranges4, _ = run(True, True, rs=True)
assert ranges3 == ranges4 == ranges0 and torch.equal(f32_rs, plain) and torch.equal(b16_rs, b16)
# gradients KEPT in the bf16 image (grad_final_next = 2): the exchange reduces the image in place and must not widen it back
def run_final2(rs):
    m.zero_grad()
    m(input_ids=ids, labels=ids, return_logits=False)
    stage = torch.full((eng.n_params,), float("nan"), dtype=torch.bfloat16, device="cuda")
    m.flat_grads.fill_(float("nan"))
    eng.set_grad_image(stage)
    def cb(off, cnt, ready):
        (eng.reduce_scatter_grads_async if rs else eng.allreduce_grads_async)(off, cnt, True, ready)
    eng.set_option("grad_overwrite_next", 1)
    eng.backward(1.0, 1, cb, final=2)
    eng.comm_finish()
    norm = torch.zeros(2, device="cuda")
    eng.grad_norm(0.0, norm)   # a backward that reported buckets: chunk sums over the image, not the partials
    torch.cuda.synchronize()
    return stage, m.flat_grads.clone(), float(norm[0])
for rs in (False, True):
    stage2, f32buf, nrm = run_final2(rs)
    assert torch.equal(stage2.float(), b16), ("final2", rs)
    emb = eng.tensors["embed"].numel
    assert bool(torch.isnan(f32buf[emb:]).all()), "the fp32 buffer was written behind the embedding (widening pass or fp32 final stores)"
    ref = float(b16.double().norm())
    assert abs(nrm - ref) <= 2e-6 * ref, (nrm, ref)
p0 = m.flat_params.clone()
for off, cnt in sorted(ranges0):
    eng.allgather_params_async(off, cnt)
out = m(input_ids=ids, labels=ids, return_logits=False)   # waits for every gathered bucket before its first read
torch.cuda.synchronize()
assert torch.equal(m.flat_params, p0) and float(out.loss) == losses[0], (float(out.loss), losses[0])
eng.comm_destroy()
assert ranges0 == ranges1 == ranges2 and sum(c for _, c in ranges0) == eng.n_params
assert torch.equal(plain, f32), float((plain - f32).abs().max())
assert torch.equal(b16, plain.to(torch.bfloat16).float()), float((b16 - plain).abs().max())
assert torch.equal(stage.float(), b16)
print("ENGINE_COMM_OK", len(ranges0))
'''


def test_engine_side_rccl_exchange_single_rank(tmp_path):
    """slam_comm_* / slam_allreduce_grads_async (include/slam_engine.h): the gradient exchange of a consumer WITHOUT
    torch.distributed - RCCL looked up by the engine at run time, one communicator per engine, collectives on the engine's
    communication stream behind slam_bucket_stream. On a 1-rank communicator a SUM all-reduce is the identity: the fp32
    exchange must leave the gradients of the plain backward bit for bit, the bf16 exchange (image written by backward,
    all-reduced, widened back) their bf16 rounding; the callback's ranges tile [0, n_params)."""
    w = tmp_path / "engine_comm_worker.py"
    w.write_text(ENGINE_COMM_WORKER)
    env = dict(os.environ, SLAM_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(w)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ENGINE_COMM_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
