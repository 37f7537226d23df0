REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof7 -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $R/$OUT/prof7_bench.json 2>/dev/null
cd $R
python profiles/summarize_rocpd.py $(ls $OUT/prof7/*/*_results.db | head -1) > $OUT/prof7_summary.txt 2>&1
python profiles/timeline_rocpd.py $OUT/prof7 6 > $OUT/prof7_timeline.txt 2>&1
rm -rf $OUT/prof7
python bench.py --full --steps 10 --warmup 2 > $OUT/bench_r1e.json 2> $OUT/bench_r1e.err
cat $OUT/bench_r1e.json
