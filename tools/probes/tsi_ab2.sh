# same-box A/B of the fused TSI sweep: FCG_LIB=base (lib/libfourc_gpu_base.so) vs the default build
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$ROOT/probe_out
cd $ROOT
mkdir -p $OUT
for rep in 1 2; do
for v in base default; do
if [ $v = base ]; then export FCG_LIB=base; else unset FCG_LIB; fi
timeout -k 10 300 python bench.py --full --steps 20 --warmup 10 --no-newton --no-amg --no-hex27 --no-optionb --no-host --no-gather --no-cpu-baseline > $OUT/tsi_ab.json 2> $OUT/tsi_ab.err || { tail -20 $OUT/tsi_ab.err; exit 1; }
python3 -c "
import json; d=json.load(open('$OUT/tsi_ab.json'))
print('$v', 'primary kernel', round(d['roofline']['ms_element_kernel'],4), 'tsi', [round(s['ms_per_step'],4) for s in d.get('secondary', [])])"
done; done
