REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
# kernel trace + stats of the default bench command, one-prove timeline; outputs under $OUT/ (copied to profiles/ by hand)
cd /tmp && export TMPDIR=/tmp
R=$REPO
TAG=${1:-r02}
rocprofv3 --kernel-trace --memory-copy-trace --stats -d $R/$OUT/prof_$TAG -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-pmc --no-dropin > $R/$OUT/prof_${TAG}_bench.json 2>/dev/null
cd $R
python profiles/summarize_rocpd.py $(ls $OUT/prof_$TAG/*/*_results.db | head -1) > $OUT/${TAG}_kernel_trace_bench_1600k.txt 2>&1
python profiles/timeline_rocpd.py $OUT/prof_$TAG 6 > $OUT/${TAG}_timeline_one_prove_1600k.txt 2>&1
rm -rf $OUT/prof_$TAG
cat $OUT/${TAG}_timeline_one_prove_1600k.txt
head -40 $OUT/${TAG}_kernel_trace_bench_1600k.txt
