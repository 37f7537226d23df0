REPO=$(pwd)   # run from the repository root
OUT=${OUT:-out}   # where this script's outputs go
# kernel trace + stats of the stand-in bench command; output → $OUT/r02_kernel_trace_bench_aadhaar_standin.txt
cd /tmp && export TMPDIR=/tmp
R=$REPO
rocprofv3 --kernel-trace --stats -d $R/$OUT/prof_standin -- python3 $R/bench.py --full --workload aadhaar_standin --steps 10 --warmup 2 --no-cpu-baseline --no-pmc --no-dropin > $R/$OUT/prof_standin_bench.json 2>/dev/null
cd $R
(echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py --full --workload aadhaar_standin --steps 10 --warmup 2 --no-cpu-baseline --no-pmc --no-dropin  (includes the key synthesis and the one-time cache build)"; python profiles/summarize_rocpd.py $(ls $OUT/prof_standin/*/*_results.db | head -1)) > $OUT/r02_kernel_trace_bench_aadhaar_standin.txt 2>&1
rm -rf $OUT/prof_standin
head -30 $OUT/r02_kernel_trace_bench_aadhaar_standin.txt | cut -c1-160
