#!/bin/bash
OUT=${OUT:-out}   # where this script's outputs go
# round-2 evidence run: default bench line, stand-in workloads, kernel trace + timeline, sort solo/PMC for both sort paths
mkdir -p $OUT
python bench.py --full > $OUT/r02_bench_1600k.json 2> $OUT/r02_bench_1600k.err
python bench.py --full --workload aadhaar_standin --no-pmc --no-dropin > $OUT/r02_bench_aadhaar_standin.json 2> $OUT/r02_bench_aadhaar.err
python bench.py --full --workload keyless_standin --no-pmc --no-dropin > $OUT/r02_bench_keyless_standin.json 2> $OUT/r02_bench_keyless.err
python bench.py --full --workload 3200k --no-pmc --no-dropin --no-cpu-baseline > $OUT/r02_bench_3200k.json 2> $OUT/r02_bench_3200k.err
python bench.py --full --workload 100k --no-pmc --no-dropin > $OUT/r02_bench_100k.json 2> $OUT/r02_bench_100k.err
bash scratch/sort_solo.sh > $OUT/r02_pmc_sort_solo.txt 2>&1
bash scratch/profile_r02.sh r02 > /dev/null 2>&1
tail -c 3000 $OUT/r02_bench_1600k.json
for f in aadhaar_standin keyless_standin 3200k 100k; do python3 -c "
import json,sys
d=json.loads(open('$OUT/r02_bench_$f.json').read().strip().splitlines()[-1]); c=d['config']
print('$f', 'ms/step', round(d['ms_per_step'],3), 'host', c['prove_ms_host_witness'], 'resident', c['prove_ms_hbm_resident'], c['phase_ms'], d.get('cpu_baseline',{}).get('sample'))"; done
cat $OUT/r02_pmc_sort_solo.txt | grep -v "^    "
