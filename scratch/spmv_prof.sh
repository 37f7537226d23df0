REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof8 -- python3 $R/scratch/spmv_only.py > /dev/null 2>&1
cd $R; python profiles/summarize_rocpd.py $(ls $OUT/prof8/*/*_results.db | head -1) | grep -i "spmv\|ntt_pass\|coset\|final"; rm -rf $OUT/prof8
python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d[\"ms_per_step\"], d[\"config\"][\"phase_ms\"], d[\"roofline\"][\"launch_ms\"])"
