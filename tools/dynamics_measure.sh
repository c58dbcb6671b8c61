#!/bin/bash
# The three measurements of profiles/dynamics/README.md on one GPU, each step under its own time
# limit, a failed step ends the run.  usage: tools/dynamics_measure.sh [out_dir] [n]
set -o pipefail
here=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$here/bench_out}
n=${2:-100}
mkdir -p "$out"
cd "$here" &&
timeout -k 10 300 python tools/dynamics_bench.py efft --n "$n" | tee "$out/dynamics_efft.json" &&
timeout -k 10 300 python tools/dynamics_bench.py mass --n "$n" | tee "$out/dynamics_mass.json" &&
timeout -k 10 400 python tools/dynamics_bench.py newton --n "$n" | tee "$out/dynamics_newton.json"
