"""Median device time and achieved bytes/s of the launches of norm_driver.py from a rocprofv3 kernel-trace csv:
    python profiles/wide_untied/norm_trace_summary.py OUT/.../norm_kernel_trace.csv
Bytes per element as elementwise.hip counts them: forward 4, backward 6, backward with the residual-gradient input 8."""
import csv
import re
import statistics
import sys

M, REPS, WARM = 16384, 25, 5
rows = [r for r in csv.DictReader(open(sys.argv[1])) if "rmsnorm_" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
assert len(rows) == 3 * 3 * REPS, len(rows)
i = 0
for H in (2048, 3584, 4096):
    for kind, bpe in (("fwd", 4), ("bwd", 6), ("bwd+dres", 8)):
        grp = rows[i:i + REPS][WARM:]
        i += REPS
        us = statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in grp)
        name = re.search(r"rmsnorm_\w+(<[^>]*>)?", grp[0]["Kernel_Name"]).group(0)
        print(f"H {H:5d} {kind:9s} {name:40s} median {us:8.1f} us  {M * H * bpe / us / 1e6:6.2f} TB/s")
