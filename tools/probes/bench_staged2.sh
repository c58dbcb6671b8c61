#!/bin/bash
# Rehearsal of bench.py's multi-rank flow on one GPU: 2 ranks over torch.distributed.run with the
# host-staged gloo transport (RCCL refuses two ranks on one device); the driver's N-GPU runs use RCCL.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$ROOT/probe_out
cd "$ROOT" || exit 2
mkdir -p $OUT
FCG_DIST_BACKEND=gloo timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 5 --warmup 2 --no-cpu-baseline \
  > $OUT/bench_staged2.json 2> $OUT/bench_staged2.err
rc=$?; tail -c 1500 $OUT/bench_staged2.json; tail -3 $OUT/bench_staged2.err; exit $rc
