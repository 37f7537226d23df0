REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof9 -- python3 $R/bench.py --full --constraints 200000 --steps 6 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
cd $R
python profiles/timeline_rocpd.py $OUT/prof9 5 > $OUT/prof9_timeline.txt 2>&1
rm -rf $OUT/prof9
sed -i 's/(e - s) > 30_000/(e - s) > 30_000/' profiles/timeline_rocpd.py
cat $OUT/prof9_timeline.txt
