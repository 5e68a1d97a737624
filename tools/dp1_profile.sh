#!/bin/bash
# rocprofv3 kernel statistics of the data-parallel step on one GPU (1-rank RCCL group, every collective running).
# Results under $OUT_DIR/dp1prof (default out/); bench.py --full: the probes after the timed region are in the trace too.
R="$(cd "$(dirname "$0")/.." && pwd)"; O=${OUT_DIR:-$R/out}; mkdir -p $O; cd /tmp; export TMPDIR=/tmp
export SLAM_DP_FORCE=1 RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29731
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/dp1prof -o dp1 -- \
  python $R/bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-extras --full > $O/dp1prof.log 2>&1
tail -2 $O/dp1prof.log; find $O/dp1prof -name "*kernel_stats.csv" | head
