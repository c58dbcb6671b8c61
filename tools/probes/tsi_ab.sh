# TSI fused sweep A/B helper: parity tests of the fused path, then the config-5 timing
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$ROOT/probe_out
cd $ROOT
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/test_tsi.py -q -x --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT/tsi_tests.log 2>&1 || { tail -30 $OUT/tsi_tests.log; exit 1; }
tail -1 $OUT/tsi_tests.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 10 --no-newton --no-amg --no-hex27 --no-optionb --no-host --no-gather --no-cpu-baseline > $OUT/tsi_ab.json 2> $OUT/tsi_ab.err || { tail -20 $OUT/tsi_ab.err; exit 1; }
python3 -c "
import json; d=json.load(open('$OUT/tsi_ab.json'))
print('primary ms', d['ms_per_step'], 'kernel', d['roofline']['ms_element_kernel'])
for s in d.get('secondary', []): print(s['workload'], s.get('ms_per_step'))"
