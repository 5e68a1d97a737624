"""NEFTune's cost (slam_set_neftune): the embedding launch armed and unarmed, and the training step with and without the option.

    python tools/neftune_bench.py [--lib OTHER/libslam_engine.so] [--shapes 8192x896,16384x1536] [--no-step]

Launch: per shape `M x H` (default: the Slam-358M step's 8 x 1024 tokens at hidden 896, and 16,384 x 1536), a random bf16
table of 502 rows (and 2050 position rows for the OPT form) and random ids on the device. A sample is `--batch` launches
back to back between two stream events, divided by the batch; armed and unarmed samples ALTERNATE in one process, `--rounds`
of each after one untimed round, and the line printed is median [min, max] in microseconds per launch. Forms: `qwen` (plain
gather, slam_op_embed_fwd, against slam_op_embed_noise_fwd without a position table) and `opt` (slam_op_embed_pos_fwd against
slam_op_embed_noise_fwd with one). `--lib` names another build's library - the parent commit's has only slam_op_embed_pos_fwd,
so only the unarmed `opt` form is timed there.

Step: the benchmark's Slam-358M workload (bench.py's model, batch and optimizer settings) through SLAMTrainer.optimizer_step,
`--steps` steps per sample with the option set (alpha 5, armed before every micro-batch as train() does it) and with it off,
alternating, `--rounds` samples of each after one untimed; milliseconds per step, median [min, max]."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(v, unit):
    return f"median {statistics.median(v):8.3f} {unit} [{min(v):8.3f}, {max(v):8.3f}] n {len(v)}"


def time_batch(torch, fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / batch  # us per launch


def launches(a, torch, E):
    lib = E.load_library(a.lib)
    p = lambda t: C.c_void_p(int(t.data_ptr()))  # noqa: E731
    st = E.current_stream_ptr()
    V, NP, T = 502, 2050, 1024
    for shape in a.shapes.split(","):
        M, H = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        Ew = torch.empty(V, H, dtype=torch.bfloat16, device="cuda").normal_(0.0, 0.02, generator=g)
        Pw = torch.empty(NP, H, dtype=torch.bfloat16, device="cuda").normal_(0.0, 0.02, generator=g)
        ids = torch.randint(0, V, (M,), device="cuda", generator=g)
        out = torch.empty(M, H, dtype=torch.bfloat16, device="cuda")
        prow = torch.empty(M, dtype=torch.int64, device="cuda")
        s = C.c_float(5.0 / (T * H) ** 0.5 / 65536.0)
        forms = {}
        if hasattr(lib, "slam_op_embed_fwd"):
            forms["qwen unarmed"] = lambda: lib.slam_op_embed_fwd(p(ids), p(Ew), p(out), M, H, V, st)
        forms["opt  unarmed"] = lambda: lib.slam_op_embed_pos_fwd(p(ids), None, p(Ew), p(Pw), p(out), p(prow), M, H, V, T, NP, st)
        if hasattr(lib, "slam_op_embed_noise_fwd"):
            forms["qwen armed  "] = lambda: lib.slam_op_embed_noise_fwd(p(ids), None, p(Ew), None, p(out), None, M, H, V, T, 0, s, 7, 3, 0, st)
            forms["opt  armed  "] = lambda: lib.slam_op_embed_noise_fwd(p(ids), None, p(Ew), p(Pw), p(out), p(prow), M, H, V, T, NP, s, 7, 3, 0, st)
        for fn in forms.values():
            assert fn() == 0
        us = {k: [] for k in forms}
        for r in range(a.rounds + 1):
            for k, fn in forms.items():  # alternating: one sample of every form per round
                t = time_batch(torch, fn, a.batch)
                if r:
                    us[k].append(t)
        mb = M * H * 2 / 1e6  # the table rows are few and cached: the traffic to memory is the output
        for k in sorted(us):
            print(f"launch {M:6d} x {H:5d} ({mb:5.1f} MB out) {k}: {fmt(us[k], 'us')}")


def steps(a, torch):
    import bench
    from slamkit_amd.model import UnitLM, UnitLMConfig
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    dev = torch.device("cuda", 0)
    model = UnitLM(UnitLMConfig(base_model_name="Qwen/Qwen2.5-0.5B", rope_theta=10000.0, vocab_size=bench.V, max_tokens=bench.B * bench.T), seed=0)
    tr = SLAMTrainer(model=model, args=SLAMTrainingArguments(per_device_train_batch_size=bench.B, learning_rate=1e-3, max_grad_norm=0.5,
                                                          logging_steps=0, optim_state_dtype="bfloat16"))
    n = float(bench.B * bench.T)
    batches = [bench.synth_batch(0, i, dev) for i in range(4)]
    model.train()

    def sample(alpha):
        tr._neftune = alpha
        model.set_neftune(alpha, seed=5)
        torch.cuda.synchronize()
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for i in range(a.steps):
            tr.optimizer_step([batches[i % 4]], 1e-3, counts=(n, n))
        b0.record()
        b0.synchronize()
        return a0.elapsed_time(b0) / a.steps

    ms = {0.0: [], 5.0: []}
    for r in range(a.rounds + 1):
        for alpha in (0.0, 5.0):
            t = sample(alpha)
            if r:
                ms[alpha].append(t)
    model.set_neftune(0.0)
    print(f"step Slam-358M {bench.B} x {bench.T}, option off      : {fmt(ms[0.0], 'ms')}")
    print(f"step Slam-358M {bench.B} x {bench.T}, neftune alpha 5 : {fmt(ms[5.0], 'ms')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build's libslam_engine.so (launches only)")
    ap.add_argument("--shapes", default="8192x896,16384x1536")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    import torch
    from slamkit_amd import engine as E
    torch.cuda.set_device(0)
    launches(a, torch, E)
    if not a.no_step and a.lib is None:
        steps(a, torch)


if __name__ == "__main__":
    main()
