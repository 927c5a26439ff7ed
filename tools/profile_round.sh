#!/bin/bash
# Collects the evidence files of a round on the GPU box (run through gpurun):
#   1. rocprofv3 --kernel-trace --stats of the default bench command (the N = 1 line: 100 Mb, -p 2)
#   2. / 3. separate --pmc FETCH_SIZE and --pmc WRITE_SIZE passes of the same command (HBM traffic per launch)
# Outputs under $OUT/<tag>_* (an absolute path; default profile_out/ in the repository); tools/pmc_traffic.py + the stats
# CSV are what gets copied to profiles/.  The bench runs with --full: the line keeps its per-kernel figures and the
# counters see the same launches as the line's.
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r05}
WORKLOAD=${2:-c4}
OUT=${OUT:-$R/profile_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats -o s -- python $R/bench.py --full --workload $WORKLOAD --no-cpu-baseline > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_stats.err
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc_fetch -o p -- python $R/bench.py --full --workload $WORKLOAD --no-cpu-baseline --no-kernel-timing > /dev/null 2> $OUT/${TAG}_pmc_fetch.err
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_pmc_write -o p -- python $R/bench.py --full --workload $WORKLOAD --no-cpu-baseline --no-kernel-timing > /dev/null 2> $OUT/${TAG}_pmc_write.err
F=$(find $OUT/${TAG}_pmc_fetch -name '*counter_collection.csv' | head -1)
W=$(find $OUT/${TAG}_pmc_write -name '*counter_collection.csv' | head -1)
# the default command = (2 warm-up + 2 timed) steps x 2 polishing rounds
# what the counters report for known byte counts on this box (streams, gathers, scattered stores)
bash $R/tools/pmc_calibrate.sh $OUT/${TAG}_pmc_calibration.json > $OUT/${TAG}_pmc_calibration.log 2>&1
python $R/tools/pmc_traffic.py "$F" "$W" $OUT/${TAG}_pmc_traffic.json 8 $OUT/${TAG}_pmc_calibration.json
S=$(find $OUT/${TAG}_stats -name '*kernel_stats.csv' | head -1)
cp "$S" $OUT/${TAG}_kernel_stats.csv
# the raw per-dispatch files are large: keep only the summaries
rm -rf $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write $OUT/${TAG}_stats
head -12 $OUT/${TAG}_kernel_stats.csv
tail -1 $OUT/${TAG}_bench_under_rocprof.json | cut -c1-300
