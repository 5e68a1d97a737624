"""The loss launch on its own (count_valid + ce_kernel / ce_big_kernel + loss_finish), in place as the engine runs it, for a
kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/loss_launch_bench.py --eps 0.1 [--lib OTHER.so]
    python tools/loss_launch_bench.py --summarise DIR [DIR ...]

A run: for each shape `M x Vp : V` (default: the two regimes of the training step, 8192 x 512 : 502 and 16384 x 152576 : 152167),
random bf16 logits (3 N(0, 1)) and random targets on the device; `--reps` launches after `--warmup` untimed ones, the logits
restored from a copy before each (the launch overwrites them with the gradient). `--eps 0` calls slam_op_cross_entropy, which
every build has, so `--lib` can name the library of another commit; `--eps > 0` calls slam_op_cross_entropy_smooth. It prints
nothing but the loss of each shape: the times are the trace's. `--summarise` reads the kernel-trace CSVs under each directory and
prints median [min, max] in microseconds of the row kernel and of loss_finish, per grid size in blocks (= per shape), without
the first `--warmup` launches of each."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarise(dirs, warmup):
    for d in dirs:
        launches = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                if name.startswith(("ce_", "loss_finish")):
                    launches.append((int(r["Start_Timestamp"]), name, int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])),
                                     (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        rows, blocks = {}, 0
        for _, name, grid, us in sorted(launches):  # loss_finish is one block whatever M: filed under its row kernel's grid
            blocks = grid if name.startswith("ce_") else blocks
            rows.setdefault((blocks, name), []).append(us)
        print(d)
        for (grid, name), v in sorted(rows.items()):
            us = v[warmup:]  # in launch order, without the warm-up launches
            print(f"  rows kernel of {grid:6d} blocks: {name:28s} n {len(us):3d}  median {statistics.median(us):9.2f} us "
                  f"[{min(us):9.2f}, {max(us):9.2f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--lib", default=None, help="another build's libslam_engine.so (eps 0 only unless it has the smoothing entry)")
    ap.add_argument("--shapes", default="8192x512:502,16384x152576:152167")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--summarise", nargs="+", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.warmup)
    import ctypes as C

    import torch
    from slamkit_amd import engine as E
    lib = E.load_library(a.lib)
    p = lambda t: C.c_void_p(int(t.data_ptr()))  # noqa: E731
    st = E.current_stream_ptr()
    for shape in a.shapes.split(","):
        mv, v = shape.split(":")
        M, Vp, V = int(mv.split("x")[0]), int(mv.split("x")[1]), int(v)
        g = torch.Generator(device="cuda").manual_seed(1)
        src = torch.empty(M, Vp, dtype=torch.bfloat16, device="cuda").normal_(0.0, 3.0, generator=g)
        labels = torch.randint(0, V, (M,), device="cuda", generator=g)
        buf = torch.empty_like(src)
        rl = torch.empty(M, dtype=torch.float32, device="cuda")
        rs = torch.empty(M, dtype=torch.float32, device="cuda")
        sc = torch.zeros(2, dtype=torch.float32, device="cuda")
        for _ in range(a.warmup + a.reps):
            buf.copy_(src)
            if a.eps > 0:
                rc = lib.slam_op_cross_entropy_smooth(p(buf), p(labels), float(M), p(buf), p(rl), p(rs), p(sc), 1, M, Vp, V, a.eps, st)
            else:
                rc = lib.slam_op_cross_entropy(p(buf), p(labels), float(M), p(buf), p(rl), p(sc), 1, M, Vp, V, st)
            assert rc == 0, rc
        torch.cuda.synchronize()
        print(f"{shape} eps {a.eps}: loss {float(sc[1]):.6f}")


if __name__ == "__main__":
    main()
