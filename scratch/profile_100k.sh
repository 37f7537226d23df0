REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof10 -- python3 $R/bench.py --full --constraints 100000 --steps 6 --warmup 2 --no-cpu-baseline > $R/$OUT/prof10_bench.json 2>/dev/null
cd $R
sed 's/(e - s) > 30_000/(e - s) > 4_000/' profiles/timeline_rocpd.py > /tmp/tl.py
python /tmp/tl.py $OUT/prof10 5 > $OUT/prof10_timeline.txt 2>&1
rm -rf $OUT/prof10
cat $OUT/prof10_timeline.txt
