ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$ROOT/probe_out
cd $ROOT
mkdir -p $OUT
timeout -k 10 600 python bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err || { tail -20 $OUT/bench_full.err; exit 1; }
cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_r02 -o run --output-format csv -- python3 $ROOT/bench.py --full --no-newton --no-amg --no-hex27 --no-cpu-baseline --steps 20 --warmup 5 > $OUT/bench_prof.json 2> $OUT/bench_prof.err || { tail -20 $OUT/bench_prof.err; exit 1; }
ls $OUT/prof_r02
