REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof12 -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $R/$OUT/prof12_bench.json 2>/dev/null
cd $R
sed 's/(e - s) > 30_000/(e - s) > 0/' profiles/timeline_rocpd.py > /tmp/tl.py
python /tmp/tl.py $OUT/prof12 6 > $OUT/prof12_timeline.txt 2>&1
rm -rf $OUT/prof12
awk '$2 > 11.5' $OUT/prof12_timeline.txt | cut -c1-110
