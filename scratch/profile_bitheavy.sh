REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof10 -- python3 $R/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
cd $R
python profiles/timeline_rocpd.py $OUT/prof10 11 > $OUT/prof10_timeline.txt 2>&1
rm -rf $OUT/prof10
cat $OUT/prof10_timeline.txt
