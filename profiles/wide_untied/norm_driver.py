"""Driver for the RMSNorm measurement of profiles/wide_untied.md: the single-op entries at M = 16,384 for H = 2048 (the
one-wave-per-row <4> instantiation: the yardstick), 3584 and 4096 (two waves per row), in a fixed order - per H: 25 forward
launches, 25 backward launches without and 25 with the residual-gradient input. Run it under
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d OUT -o norm --output-format csv -- python profiles/wide_untied/norm_driver.py
and summarise the trace with norm_trace_summary.py (which relies on this order; the first 5 launches of each kind are warm-up)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.gpu_util import lib, ptr, stream  # noqa: E402

M, REPS = 16384, 25
for H in (2048, 3584, 4096):
    g = torch.Generator(device="cuda").manual_seed(H)
    x, dy, dres = (torch.randn(M, H, device="cuda", generator=g).to(torch.bfloat16) for _ in range(3))
    w = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(torch.bfloat16)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(M, dtype=torch.float32, device="cuda")
    dw = torch.empty(H, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib().slam_op_rmsnorm_bwd_workspace(M, H) // 4 + 16, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(REPS):
        assert lib().slam_op_rmsnorm_fwd(ptr(x), ptr(w), ptr(y), ptr(rstd), M, H, 1e-6, stream()) == 0
    for res in (None, dres):
        for _ in range(REPS):
            assert lib().slam_op_rmsnorm_bwd(ptr(dy), ptr(x), ptr(w), ptr(rstd), ptr(res), ptr(dx), ptr(dw), ptr(ws), M, H, stream()) == 0
    torch.cuda.synchronize()
print("norm driver done")
